"""Hybrid TD3 agent of ``src/models/Hybrid_TD3_model_PER.py`` on the HIP kernels.

``Critic`` (111-183), ``hybrid_actors`` (185-251) and ``Hybrid_TD3_Model`` (254-393) with the
reference's constructor arguments, attribute names, submodule order (so ``torch.manual_seed(s)``
followed by construction gives its initial values bitwise) and ``state_dict`` keys, and
``Memory`` re-exported from ``replay_memory``: the module replaces the reference file.

Every Linear runs on the fused GEMM (``p_model._LinearAct``), every BatchNorm1d (+ReLU) is one
launch forward and one backward (``_BNAct`` on ctr_bn_forward / ctr_bn_backward), the critic's
``cat`` is the BatchNorm writing straight into the first columns of the [B, input_dims + 2A]
input, and the noise, the action heads, the target smoothing, the critic loss with its
gradients and both soft updates are one launch each (csrc/td3.hip). ``learn`` enqueues on the
current stream and, with ``return_tensor=True``, never copies to the host or waits for it.

What is kept from the reference, quirks included:
  * both target networks stay in training mode (deep copies that never see ``.eval()``): their
    BatchNorms normalise with batch statistics and update their own running statistics;
  * ``soft_update`` walks ``parameters()`` only, never a buffer;
  * every ``policy_freq``-th ``learn`` runs ``Critic.evaluate_q_1`` a second time in training
    mode, so ``bn_input`` and the ``mlp_1`` BatchNorms update their running statistics twice;
  * the discrete action is ``argsort(-d)[:, 0] + 1``. Tie rule: among equal values the LOWEST
    index wins (torch's unstable sort leaves it open; here it is fixed).
The actor loss's gradients for the critic's parameters, which the reference computes and then
zeroes before they are used, are not computed.

Extensions (keyword only, the defaults are the reference's behaviour): ``learn(sample=,
noise=, return_tensor=)``, ``choose_action(noise=)`` and ``store_step(features=, c_actions=,
d_values=, d_actions=, rewards=)``, the driver's pack-and-store as one launch. Generated noise is a stateless hash of
a seed taken from torch's CPU generator (as ``replay_memory._rng_sample_seed``), not torch's
device stream: after ``torch.manual_seed`` two runs are identical. One attribute beyond the
reference's: ``last``, the device tensors ``q1``, ``q2``, ``q_target``, ``td`` and ``loss`` of
the most recent ``learn`` (references, no copy), for monitoring and for the parity tests.

The eval-mode BatchNorm is forward only: ``choose_action`` / ``choose_best_action`` run under
``no_grad`` as in the reference, and differentiating through an eval-mode network raises.
``hybrid_actors.act`` returns tensors without an autograd graph.
"""
from __future__ import annotations

import copy

import torch
import torch.nn as nn

from . import hip_ops
from .optim import DenseAdam
from .p_model import _LinearAct
from .replay_memory import Memory, _rng_sample_seed

__all__ = ["Memory", "Critic", "hybrid_actors", "Hybrid_TD3_Model"]

NEURON_NUMS = [400, 300, 200]


class _BNAct(torch.autograd.Function):
    """Training-mode BatchNorm1d (+ReLU) as one launch each way."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu):
        r = hip_ops.bn_forward(x, gamma, beta, running_mean, running_var, eps=eps,
                               momentum=momentum, training=True, relu=relu)
        ctx.save_for_backward(x, r["y"], gamma, r["mean"], r["mean_lo"], r["invstd"],
                              r["invstd_lo"])
        ctx.relu = relu
        return r["y"]

    @staticmethod
    def backward(ctx, gy):
        x, y, gamma, mean, mean_lo, invstd, invstd_lo = ctx.saved_tensors
        if gy.dim() != 2 or (gy.shape[1] > 1 and gy.stride(1) != 1) or \
                (gy.shape[0] > 1 and gy.stride(0) < gy.shape[1]):
            gy = gy.contiguous()
        r = hip_ops.bn_backward(gy, x, mean, invstd, gamma, y=y, relu=ctx.relu, mean_lo=mean_lo,
                                invstd_lo=invstd_lo, want_dx=ctx.needs_input_grad[0])
        return (r["dx"], r["dgamma"] if ctx.needs_input_grad[1] else None,
                r["dbeta"] if ctx.needs_input_grad[2] else None, None, None, None, None, None)


class _BatchNorm1d(nn.BatchNorm1d):
    """nn.BatchNorm1d (same construction, parameters, buffers and state_dict keys) whose
    forward is the HIP kernel, optionally fused with the ReLU that follows it."""

    def forward(self, input, relu: bool = False, out=None):  # noqa: A002 (reference name)
        if input.dim() != 2 or input.shape[1] != self.num_features:
            raise ValueError(f"expected a [B, {self.num_features}] input, got {tuple(input.shape)}")
        if not (self.affine and self.track_running_stats) or self.momentum is None:
            raise NotImplementedError("BatchNorm1d: the agent's affine, tracking form only")
        if self.training:
            if input.shape[0] < 2:
                raise ValueError("Expected more than 1 value per channel when training, got "
                                 f"input size {tuple(input.shape)}")
            self.num_batches_tracked.add_(1)
            if torch.is_grad_enabled() and (input.requires_grad or self.weight.requires_grad):
                if out is not None:
                    raise RuntimeError("BatchNorm1d: out= is for calls under torch.no_grad()")
                return _BNAct.apply(input, self.weight, self.bias, self.running_mean,
                                    self.running_var, self.eps, self.momentum, relu)
            return hip_ops.bn_forward(input, self.weight, self.bias, self.running_mean,
                                      self.running_var, eps=self.eps, momentum=self.momentum,
                                      training=True, relu=relu, out=out, save=False)["y"]
        if torch.is_grad_enabled() and (input.requires_grad or self.weight.requires_grad):
            raise RuntimeError("BatchNorm1d: the eval-mode forward has no backward here; call "
                               "it under torch.no_grad()")
        return hip_ops.bn_forward(input, self.weight, self.bias, self.running_mean,
                                  self.running_var, eps=self.eps, training=False, relu=relu,
                                  out=out)["y"]


def _linear(lin: nn.Linear, h: torch.Tensor) -> torch.Tensor:
    return _LinearAct.apply(h, lin.weight, lin.bias, False, 0.0, 0)


def _run_mlp(mlp: nn.Sequential, h: torch.Tensor) -> torch.Tensor:
    """[Linear, BatchNorm1d, ReLU]* (+ Linear): a GEMM and one fused BN+ReLU launch per block."""
    mods = list(mlp)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Linear):
            h = _linear(m, h)
            i += 1
        elif isinstance(m, _BatchNorm1d):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            h = m(h, relu=relu)
            i += 1 + int(relu)
        else:
            raise TypeError(f"unsupported layer {type(m).__name__}")
    return h


def _mlp_blocks(dims_in: int, last: bool) -> nn.Sequential:
    layers = []
    for n in NEURON_NUMS:
        layers += [nn.Linear(dims_in, n), _BatchNorm1d(n), nn.ReLU()]
        dims_in = n
    if last:
        layers.append(nn.Linear(dims_in, 1))
    return nn.Sequential(*layers)


class _CriticInput(torch.autograd.Function):
    """cat([bn_input(state), c_actions, d_actions], 1) without the cat: the BatchNorm writes
    the first input_dims columns of the [B, input_dims + 2A] matrix, the actions are copied
    beside them. Backward: the columns' gradients, and bn_input's parameter gradients (dx for
    the state only when it asks for one: the agent's states are detached)."""

    @staticmethod
    def forward(ctx, state, c_actions, d_actions, gamma, beta, running_mean, running_var, eps,
                momentum):
        B, D = state.shape
        Ac, Ad = c_actions.shape[1], d_actions.shape[1]
        buf = torch.empty(B, D + Ac + Ad, dtype=torch.float32, device=state.device)
        r = hip_ops.bn_forward(state, gamma, beta, running_mean, running_var, eps=eps,
                               momentum=momentum, training=True, out=buf[:, :D])
        buf[:, D:D + Ac].copy_(c_actions)
        buf[:, D + Ac:].copy_(d_actions)
        ctx.save_for_backward(state, gamma, r["mean"], r["mean_lo"], r["invstd"], r["invstd_lo"])
        ctx.dims = (D, Ac, Ad)
        return buf

    @staticmethod
    def backward(ctx, g):
        state, gamma, mean, mean_lo, invstd, invstd_lo = ctx.saved_tensors
        D, Ac, Ad = ctx.dims
        g = g.contiguous()
        dx = dgamma = dbeta = None
        if any(ctx.needs_input_grad[i] for i in (0, 3, 4)):
            r = hip_ops.bn_backward(g[:, :D], state, mean, invstd, gamma, mean_lo=mean_lo,
                                    invstd_lo=invstd_lo, want_dx=ctx.needs_input_grad[0])
            dx, dgamma, dbeta = r["dx"], r["dgamma"], r["dbeta"]
        return (dx, g[:, D:D + Ac] if ctx.needs_input_grad[1] else None,
                g[:, D + Ac:] if ctx.needs_input_grad[2] else None,
                dgamma if ctx.needs_input_grad[3] else None,
                dbeta if ctx.needs_input_grad[4] else None, None, None, None, None)


class _TanhHeads(torch.autograd.Function):
    """tanh of both heads' pre-activations in one launch (ctr_td3_act without noise)."""

    @staticmethod
    def forward(ctx, pre_c, pre_d):
        r = hip_ops.td3_act(pre_c, pre_d, want_softmax=False, want_index=False)
        ctx.save_for_backward(r["c_actions"], r["d_actions"])
        return r["c_actions"], r["d_actions"]

    @staticmethod
    def backward(ctx, gc, gd):
        c, d = ctx.saved_tensors
        return gc * (1.0 - c * c), gd * (1.0 - d * d)


class Critic(nn.Module):
    def __init__(self, input_dims, c_action_nums, d_action_nums):
        super(Critic, self).__init__()
        self.input_dims = input_dims
        self.c_action_nums = c_action_nums
        self.d_action_nums = d_action_nums

        self.bn_input = _BatchNorm1d(self.input_dims)

        deep_input_dims = self.input_dims + self.c_action_nums + self.d_action_nums
        self.mlp_1 = _mlp_blocks(deep_input_dims, last=True)
        self.mlp_2 = _mlp_blocks(deep_input_dims, last=True)

    def _cat(self, input, c_actions, d_actions):  # noqa: A002
        bn = self.bn_input
        if not bn.training:
            obs = bn(input)
            return torch.cat([obs, c_actions, d_actions], dim=1)
        if input.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input "
                             f"size {tuple(input.shape)}")
        bn.num_batches_tracked.add_(1)
        return _CriticInput.apply(input, c_actions, d_actions, bn.weight, bn.bias,
                                  bn.running_mean, bn.running_var, bn.eps, bn.momentum)

    def _input_buffer(self, input):  # noqa: A002
        """The [B, input_dims + 2A] input with bn_input(state) in its first columns, for a
        caller that writes the action columns itself (the target smoothing). No autograd."""
        B, D = input.shape
        buf = torch.empty(B, D + self.c_action_nums + self.d_action_nums, dtype=torch.float32,
                          device=input.device)
        with torch.no_grad():
            self.bn_input(input, out=buf[:, :D])
        return buf

    def evaluate(self, input, c_actions, d_actions):  # noqa: A002
        cat = self._cat(input, c_actions, d_actions)
        return _run_mlp(self.mlp_1, cat), _run_mlp(self.mlp_2, cat)

    def evaluate_q_1(self, input, c_actions, d_actions):  # noqa: A002
        cat = self._cat(input, c_actions, d_actions)
        return _run_mlp(self.mlp_1, cat)


class hybrid_actors(nn.Module):  # noqa: N801 (reference name)
    def __init__(self, input_dims, action_nums):
        super(hybrid_actors, self).__init__()
        self.input_dims = input_dims
        self.c_action_dims = action_nums
        self.d_action_dims = action_nums
        if not 1 <= action_nums <= hip_ops.TD3_MAX_A:
            raise ValueError(f"hybrid_actors: action_nums outside [1, {hip_ops.TD3_MAX_A}]")

        self.bn_input = _BatchNorm1d(self.input_dims)
        self.mlp = _mlp_blocks(self.input_dims, last=False)
        self.c_action_layer = nn.Sequential(nn.Linear(NEURON_NUMS[2], self.c_action_dims),
                                            nn.Tanh())
        self.d_action_layer = nn.Sequential(nn.Linear(NEURON_NUMS[2], self.d_action_dims),
                                            nn.Tanh())

        # plain tensors in the reference (which hard-codes .cuda()); here they follow the module
        self.std = torch.ones(size=[1, self.c_action_dims])
        self.mean = torch.zeros(size=[1, self.c_action_dims])

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.std, self.mean = fn(self.std), fn(self.mean)
        return self

    def _pre(self, input):  # noqa: A002
        """Both heads' pre-activations [B, A]."""
        mlp_out = _run_mlp(self.mlp, self.bn_input(input))
        return _linear(self.c_action_layer[0], mlp_out), _linear(self.d_action_layer[0], mlp_out)

    def act(self, input, *, noise=None, seed=None):  # noqa: A002
        """(c_actions, softmax(c_actions), d_action, argmax(d_action) + 1 as [B, 1]) with the
        0.1-scaled exploration noise: noise=(n_c, n_d) unit normals, or seed=, or a seed drawn
        from torch's CPU generator."""
        with torch.no_grad():
            pre_c, pre_d = self._pre(input)
            if noise is None and seed is None:
                seed = _rng_sample_seed()
            r = hip_ops.td3_act(pre_c, pre_d, noise=noise, seed=seed, sigma=0.1)
        return r["c_actions"], r["c_softmax"], r["d_actions"], r["d_index"]

    def evaluate(self, input):  # noqa: A002
        pre_c, pre_d = self._pre(input)
        return _TanhHeads.apply(pre_c, pre_d)


class Hybrid_TD3_Model():  # noqa: N801 (reference name)
    def __init__(
            self,
            feature_nums,
            field_nums=15,
            latent_dims=5,
            action_nums=2,
            campaign_id='1458',
            lr_C_A=1e-3,
            lr_D_A=1e-3,
            lr_C=1e-2,
            reward_decay=1,
            memory_size=4096000,
            batch_size=256,
            tau=0.005,  # for target network soft update
            device='cuda:0',
    ):
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.c_action_nums = action_nums
        self.d_action_nums = action_nums
        self.campaign_id = campaign_id
        self.lr_C_A = lr_C_A
        self.lr_D_A = lr_D_A
        self.lr_C = lr_C
        self.gamma = reward_decay
        self.latent_dims = latent_dims
        self.memory_size = memory_size
        self.batch_size = batch_size
        self.tau = tau
        self.device = device

        self.memory_counter = 0

        self.input_dims = self.field_nums * (self.field_nums - 1) // 2 + self.field_nums * self.latent_dims

        self.memory = Memory(self.memory_size, self.field_nums + self.c_action_nums + self.d_action_nums + 2, self.device)

        self.Hybrid_Actor = hybrid_actors(self.input_dims, self.c_action_nums).to(self.device)
        self.Critic = Critic(self.input_dims, self.c_action_nums, self.d_action_nums).to(self.device)

        self.Hybrid_Actor_ = copy.deepcopy(self.Hybrid_Actor)
        self.Critic_ = copy.deepcopy(self.Critic)

        self.optimizer_a = DenseAdam(self.Hybrid_Actor.parameters(), lr=self.lr_C_A)
        self.optimizer_c = DenseAdam(self.Critic.parameters(), lr=self.lr_C)

        self.loss_func = nn.MSELoss(reduction='mean')

        self.action_mean = torch.zeros(size=[1, self.c_action_nums]).to(self.device)
        self.action_std = torch.ones(size=[1, self.c_action_nums]).to(self.device)

        self.learn_iter = 0
        self.policy_freq = 4

        # the soft updates' device tables, built once (rebuilt only if a parameter moved)
        self._soft_tables: dict = {}
        if next(self.Critic.parameters()).is_cuda:  # (a host model constructs, but cannot run)
            for net, tgt in ((self.Critic, self.Critic_), (self.Hybrid_Actor, self.Hybrid_Actor_)):
                self._soft_table(net, tgt)
        self.last: dict = {}  # device tensors of the last learn (q1, q2, q_target, td, loss)

    def store_transition(self, transitions):
        td_errors = torch.ones(size=[len(transitions), 1]).to(self.device)

        self.memory.add(td_errors, transitions)

    def store_step(self, *, features, c_actions, d_values, d_actions, rewards):
        """store_transition(cat([features.float(), c_actions, d_values, d_actions.float(),
        rewards], 1)) without the casts, the cat and the ones: one launch (Memory.add_step)."""
        self.memory.add_step(features, c_actions, d_values, d_actions, rewards)

    def choose_action(self, state, *, noise=None):
        self.Hybrid_Actor.eval()
        with torch.no_grad():
            c_actions, ensemble_c_actions, d_q_values, ensemble_d_actions = \
                self.Hybrid_Actor.act(state, noise=noise)

        self.Hybrid_Actor.train()
        return c_actions, ensemble_c_actions, d_q_values, ensemble_d_actions

    def choose_best_action(self, state):
        self.Hybrid_Actor.eval()
        with torch.no_grad():
            pre_c, pre_d = self.Hybrid_Actor._pre(state)
            r = hip_ops.td3_act(pre_c, pre_d)  # tanh, softmax and argmax + 1 in one launch
        # the reference never switches back here; this does, as choose_action does
        self.Hybrid_Actor.train()
        return r["d_index"], r["c_softmax"]

    def _soft_table(self, net, net_target):
        src = [p.data for p in net.parameters()]
        dst = [p.data for p in net_target.parameters()]
        key = (id(net), id(net_target))
        tab = self._soft_tables.get(key)
        if tab is None or not tab.matches(dst, src):
            tab = self._soft_tables[key] = hip_ops.SoftUpdateTable(dst, src)
        return tab

    def soft_update(self, net, net_target):
        hip_ops.soft_update_multi(self._soft_table(net, net_target), self.tau)

    def learn(self, embedding_layer, *, sample=None, noise=None, return_tensor=False):
        self.learn_iter += 1
        F_, A = self.field_nums, self.c_action_nums

        if sample is None:
            choose_idx, batch_memory, ISweights = self.memory.stochastic_sample(self.batch_size)
        else:
            choose_idx, batch_memory, ISweights = sample

        with torch.no_grad():
            b_s = embedding_layer.forward(batch_memory[:, :F_].long())
        b_s = b_s.detach()
        b_c_a = batch_memory[:, F_: F_ + A]
        b_d_a = batch_memory[:, F_ + A: F_ + 2 * A]
        b_r = batch_memory[:, -1]
        D = b_s.shape[1]

        with torch.no_grad():
            pre_c, pre_d = self.Hybrid_Actor_._pre(b_s)
            cat_t = self.Critic_._input_buffer(b_s)
            # tanh, the clipped 0.2-scaled noise and the clamp, into the action columns
            hip_ops.td3_smooth(pre_c, pre_d, cat_t[:, D:D + A], cat_t[:, D + A:], noise=noise,
                               seed=None if noise is not None else _rng_sample_seed(),
                               apply_tanh=True)
            q1_target = _run_mlp(self.Critic_.mlp_1, cat_t)
            q2_target = _run_mlp(self.Critic_.mlp_2, cat_t)

        q1, q2 = self.Critic.evaluate(b_s, b_c_a, b_d_a)

        out = hip_ops.td3_critic_loss(q1.detach(), q2.detach(), q1_target, q2_target, b_r,
                                      ISweights.contiguous(), float(self.gamma))
        self.optimizer_c.zero_grad()
        torch.autograd.backward([q1, q2], [out["dq1"], out["dq2"]])
        self.optimizer_c.step()

        self.memory.batch_update(choose_idx, out["td"])
        self.last = dict(q1=q1.detach(), q2=q2.detach(), q_target=out["q_target"], td=out["td"],
                         loss=out["loss"])

        if self.learn_iter % self.policy_freq == 0:
            # actor_loss = -q.mean(). Only the actor's parameters get gradients: the critic's
            # would be zeroed before they are used, so its parameters do not ask for any while
            # this graph is built and its weight-gradient GEMMs never run
            critic_params = list(self.Critic.parameters())
            for p in critic_params:
                p.requires_grad_(False)
            try:
                c_actions_means, d_actions_q_values = self.Hybrid_Actor.evaluate(b_s)
                q = self.Critic.evaluate_q_1(b_s, c_actions_means, d_actions_q_values)
            finally:
                for p in critic_params:
                    p.requires_grad_(True)
            params = list(self.Hybrid_Actor.parameters())
            B = q.shape[0]
            grads = torch.autograd.grad([q], params, [torch.full_like(q, -1.0 / B)])
            self.optimizer_a.zero_grad()
            for p, g in zip(params, grads):
                p.grad = g
            self.optimizer_a.step()

            self.soft_update(self.Critic, self.Critic_)
            self.soft_update(self.Hybrid_Actor, self.Hybrid_Actor_)

        return out["loss"] if return_tensor else out["loss"].item()
