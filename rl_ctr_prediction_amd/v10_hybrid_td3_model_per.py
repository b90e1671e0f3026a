"""The v10 hybrid TD3 agent of ``src/models/v10_Hybrid_TD3_model_PER.py`` on the HIP kernels.

``Memory`` (19-110), ``Hybrid_Critic`` (119-189), ``Hybrid_Actor`` (191-256),
``Hybrid_TD3_Model`` (288-560), ``gumbel_softmax_sample``, ``boltzmann_softmax`` and
``hidden_init`` with the reference's constructor arguments, attribute names, submodule order and
``state_dict`` keys: the module replaces the reference file. The constructor calls
``setup_seed(1)`` as line 323 does, so the initial values are the reference's bitwise. The
package's ``Hybrid_TD3_Model`` stays the base agent; v10 is reached through this module.

Every Linear runs on the fused GEMM (``p_model._LinearAct``, the ReLU in its epilogue),
``bn_input`` on the BatchNorm launches of csrc/td3.hip, the critic's ``cat`` is the BatchNorm
writing straight into the first columns of the [B, input_dims + 2A] input, and everything that
is not a Linear is one launch of csrc/td3_v10.hip: the action heads, the rank mask (the
reference's A^2 Python loops of ``nonzero()``), the actor loss's backward through the heads,
the two launches of the gradient clipping and the memory's max, store and update; the sampler
is the base memory's select (csrc/per.hip) with the priority transform applied where a priority
is read.

What is kept from the reference, quirks included:
  * transition = [F ids | A c_action_means | A d_action (soft) | discrete action | reward]; the
    memory is F + 2A + 2 wide, ``prioritys_`` is [N, 2] = (signed TD error, reward);
  * ``Memory.add(td_error[n, 2], transitions)`` OVERWRITES rows over the ring wrap (no max);
  * ``store_transition`` seeds column 0 of the new rows with 1 if ``max(prioritys_) == 0`` else
    ``max(prioritys_)``, the max over the WHOLE [N, 2] tensor (both columns, unfilled rows
    included); column 1 is the reward. Max and store run on the device, nothing is read back;
  * ``stochastic_sample``: priorities (|p0| + 1e-3)^0.6 of the filled rows, computed when
    sampling; k distinct indices by the project's Gumbel top-k (as ``replay_memory``; the seed
    comes from torch's CPU generator unless given); isw = (p_i / min p)^(-beta), beta = 1.0,
    which the stochastic sampler never increments;
  * ``batch_update(idx, td)`` writes the raw signed td into column 0;
  * ``greedy_sample`` is ill-formed in the reference (it sorts the two-column tensor and
    squeezes a [k, 2] index): it raises NotImplementedError. ``learn`` never calls it;
  * ``Hybrid_Actor.act``: c_means = tanh(.), ensemble_c = softmax(2 c_means + 0.2 n_c),
    d_action = softmax((2 d_q + 0.2 n_d + g) / T), g = -log(-log(u + 1e-20) + 1e-20),
    ensemble_d = argmax + 1, the LOWEST index among equal values;
  * ``choose_action(state, random)`` puts the actor in eval mode; with ``random`` true it
    returns clamp(n, -1, 1), its softmax, softmax(n') and its argmax + 1 AND LEAVES THE ACTOR
    IN EVAL MODE; otherwise it goes back to train mode;
  * ``choose_best_action``: eval mode, and it stays there; returns (d_actions [B, 1], c_means,
    softmax(c_means)) with d_actions = argmax(d_q + g) + 1 (the hard Gumbel sample's argmax at
    T = 0.1), lowest index on ties;
  * ``learn``, target step: the target actor (a deep copy, always in training mode, under
    no_grad); next_d = softmax((2 d_q' + 0.2 n_d + g) / T); next_c rank-masked: row b keeps
    column m if m is among the top argmax(next_d[b]) + 1 columns of c' by value (ties rank the
    lower index first), a kept element is 2 c' + 0.2 n, the others 0, then clamp(-1, 1);
    q_target = r + gamma min(q1', q2');
  * critic step: td = (2 q_target - q1 - q2) / 2; loss = mean(isw ((q1 - q_t)^2 +
    (q2 - q_t)^2)); the global gradient norm is clipped to 0.5 by torch's formula,
    0.5 / (norm + 1e-6) capped at 1; Adam; ``batch_update``. The loss kernel is the base
    agent's ``td3_critic_loss``; its td = 2 q_target - q1 - q2 is halved by a multiplication by
    0.5, a power of two, which is exact: this is relied on;
  * actor step, every 10th call, with the actor IN WHATEVER MODE IT IS IN: d_soft =
    softmax((d_q + g) / 0.1), c rank-masked without noise, loss = mean(isw (-q1(s, c, d_soft)))
    + 1e-2 (mean(c_means^2) + mean(d_q^2)); clip to 0.5; Adam; both soft updates with
    tau = 0.01 over ``parameters()`` only. The critic's bn_input runs in training mode there a
    second time, as in the reference;
  * the temperature anneals on the host as in lines 477-479: when (learn_iter + 1) % 1000 == 0
    it drops by (T - T_min) * learn_iter / (data_len // train_batch_size), not below T_min;
  * ``reset_parameters`` (never called by the reference) is not provided;
  * no BatchNorm inside the MLPs; both target networks stay in training mode.
The actor loss's gradients for the critic's parameters, which the reference computes and then
zeroes before they are used, are not computed.

Eval-mode gradients. After a ``choose_best_action`` or a random ``choose_action`` the actor's
``bn_input`` is in eval mode and the actor update differentiates through it: its weight and
bias get dgamma = sum dy x_hat and dbeta = sum dy from the running statistics
(``ctr_bn_eval_backward``). The states carry no gradient; an input that asks for one is refused.
The base agent's BatchNorm still refuses the eval-mode backward.

Extensions (keyword only; the defaults are the reference's behaviour): ``learn(sample=, noise=,
return_tensor=)``, ``choose_action(noise=)``, ``choose_best_action(noise=)``. ``noise`` for
``learn`` is a dict of [B, A] tensors: ``n_d`` and ``n_c`` (unit normals of the target step),
``u`` (the target step's uniforms) and ``u_actor`` (the actor step's, needed on every 10th
call); for ``choose_action`` (n_c, n_d, u), or (n_c, n_d) with ``random``; for
``choose_best_action`` u. Generated noise is the stateless hash ``td3_noise`` uses, normals
and uniforms in (0, 1) from disjoint ranges of one seed taken from torch's CPU generator:
after ``torch.manual_seed`` two runs are identical. ``last`` holds the device tensors ``q1``,
``q2``, ``q_target``, ``td``, ``loss`` of the most recent ``learn`` (and ``grad_norm_c`` /
``grad_norm_a``, the gradient norms before clipping). With ``return_tensor=True`` ``learn``
never copies to the host or waits for it. ``gumbel_softmax_sample`` returns a tensor without
an autograd graph.
"""
from __future__ import annotations

import copy
import random

import numpy as np
import torch
import torch.nn as nn

from . import hip_ops
from .hybrid_td3_model_per import _BatchNorm1d, _CriticInput
from .optim import DenseAdam
from .p_model import _LinearAct
from .replay_memory import _rng_sample_seed

__all__ = ["Memory", "Hybrid_Critic", "Hybrid_Actor", "Hybrid_TD3_Model",
           "gumbel_softmax_sample", "boltzmann_softmax", "hidden_init", "setup_seed"]

NEURON_NUMS = [400, 300]


def setup_seed(seed):
    """Seed every generator the constructor's initial values can depend on (torch's CPU and
    device generators, numpy, random)."""
    for seeder in (torch.manual_seed, np.random.seed, random.seed):
        seeder(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class Memory(object):
    def __init__(self, memory_size, transition_lens, device):
        memory_size, transition_lens = int(memory_size), int(transition_lens)
        if memory_size < 1 or transition_lens < 2:
            raise ValueError("Memory: memory_size must be positive and transition_lens >= 2")
        self.device = device
        self.transition_lens = transition_lens
        self.epsilon = 1e-3
        self.alpha = 0.6
        self.beta = 1.0
        self.beta_increment_per_sampling = 1e-4
        self.abs_err_upper = 1

        self.memory_size = memory_size
        self.memory_counter = 0

        self.prioritys_ = torch.zeros(size=[memory_size, 2], dtype=torch.float32, device=device)
        self.memory = torch.zeros(size=[memory_size, transition_lens], dtype=torch.float32,
                                  device=device)
        self._max_ws = None      # the memory max's per-block partials

    def get_priority(self, td_error):
        return torch.pow(torch.abs(td_error) + self.epsilon, self.alpha)

    def _check_rows(self, transitions, who):
        if not isinstance(transitions, torch.Tensor) or transitions.dim() != 2 or \
                transitions.shape[1] != self.transition_lens or transitions.dtype != torch.float32:
            raise ValueError(f"{who}: transitions must be float32 [n, {self.transition_lens}]")
        if transitions.shape[0] > self.memory_size:
            raise ValueError(f"{who}: {transitions.shape[0]} transitions do not fit a memory of "
                             f"{self.memory_size}")
        if transitions.shape[0] and transitions.stride(1) != 1:
            transitions = transitions.contiguous()
        return transitions

    def add(self, td_error, transitions):
        transitions = self._check_rows(transitions, "add")
        n = transitions.shape[0]
        if not isinstance(td_error, torch.Tensor) or td_error.dtype != torch.float32 or \
                tuple(td_error.shape) != (n, 2):
            raise ValueError(f"add: td errors must be float32 [{n}, 2]")
        hip_ops.td3v10_add(self.memory, self.prioritys_, self.memory_counter % self.memory_size,
                           transitions, td_error.contiguous())
        self.memory_counter += n

    def add_seeded(self, transitions):
        """store_transition's add: the new rows' priorities are (1 if max(prioritys_) == 0 else
        max(prioritys_), reward), the max taken on the device before the rows are written."""
        transitions = self._check_rows(transitions, "store_transition")
        if self._max_ws is None:
            self._max_ws = torch.empty(4096, dtype=torch.uint8, device=self.memory.device)
        hip_ops.td3v10_store_seeded(self.memory, self.prioritys_,
                                    self.memory_counter % self.memory_size, transitions,
                                    self._max_ws)
        self.memory_counter += transitions.shape[0]

    def stochastic_sample(self, batch_size, seed=None):
        k = int(batch_size)
        filled = min(self.memory_counter, self.memory_size)
        if k < 1 or k > filled:
            raise ValueError(f"stochastic_sample: batch_size {k} outside [1, {filled}] (the "
                             "filled slots)")
        if k > hip_ops.PER_MAX_K:
            raise ValueError(f"stochastic_sample: batch_size {k} > {hip_ops.PER_MAX_K}")
        if seed is None:
            seed = _rng_sample_seed()
        out = hip_ops.td3v10_sample(self.memory, self.prioritys_, filled, k, seed, self.beta,
                                    self.epsilon, self.alpha)
        return out["idx"], out["batch"], out["isw"]

    def greedy_sample(self, batch_size):
        raise NotImplementedError(
            "greedy_sample is ill-formed in the reference (it sorts the two-column prioritys_ "
            "along dim 0 and squeezes a [k, 2] index, lines 96-98); learn never calls it")

    def batch_update(self, choose_idx, td_errors):
        if not isinstance(choose_idx, torch.Tensor) or choose_idx.dtype != torch.int64:
            raise ValueError("batch_update: choose_idx must be an int64 tensor")
        idx = choose_idx.reshape(-1).contiguous()
        if not isinstance(td_errors, torch.Tensor) or td_errors.dtype != torch.float32 or \
                td_errors.numel() != idx.numel():
            raise ValueError(f"batch_update: td errors must be float32 [{idx.numel()}, 1]")
        hip_ops.td3v10_update(self.prioritys_, idx, td_errors.contiguous())


def hidden_init(layer):
    """(0, 1 / sqrt(n)) for a Linear, n being the FIRST dimension of its weight (out_features:
    the reference names it fan-in)."""
    return 0, float(layer.weight.shape[0]) ** -0.5


class _BNEvalParams(torch.autograd.Function):
    """Eval-mode BatchNorm1d whose weight and bias take gradients; the input takes none."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps):
        y = hip_ops.bn_forward(x, gamma, beta, running_mean, running_var, eps=eps,
                               training=False)["y"]
        ctx.save_for_backward(x, running_mean, running_var)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, gy):
        x, rm, rv = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise RuntimeError("BatchNorm1d: the eval-mode backward gives the parameters' "
                               "gradients only; the input must not require one")
        if gy.dim() != 2 or (gy.shape[1] > 1 and gy.stride(1) != 1) or \
                (gy.shape[0] > 1 and gy.stride(0) < gy.shape[1]):
            gy = gy.contiguous()
        dgamma, dbeta = hip_ops.bn_eval_backward(gy, x, rm, rv, ctx.eps)
        return None, dgamma, dbeta, None, None, None


class _BatchNorm1dV10(_BatchNorm1d):
    """The base agent's BatchNorm1d, plus the eval-mode parameter backward the v10 actor
    update needs."""

    def forward(self, input, relu: bool = False, out=None):  # noqa: A002 (reference name)
        if not self.training and not relu and out is None and torch.is_grad_enabled() and \
                self.weight.requires_grad and not input.requires_grad:
            if input.dim() != 2 or input.shape[1] != self.num_features:
                raise ValueError(f"expected a [B, {self.num_features}] input, got "
                                 f"{tuple(input.shape)}")
            return _BNEvalParams.apply(input, self.weight, self.bias, self.running_mean,
                                       self.running_var, self.eps)
        return super().forward(input, relu=relu, out=out)


def _linear(lin: nn.Linear, h: torch.Tensor, relu: bool) -> torch.Tensor:
    return _LinearAct.apply(h, lin.weight, lin.bias, relu, 0.0, 0)


def _run_mlp(mlp: nn.Sequential, h: torch.Tensor) -> torch.Tensor:
    """[Linear, ReLU]* (+ Linear): one GEMM per Linear, the ReLU in its epilogue."""
    mods = list(mlp)
    i = 0
    while i < len(mods):
        if not isinstance(mods[i], nn.Linear):
            raise TypeError(f"unsupported layer {type(mods[i]).__name__}")
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        h = _linear(mods[i], h, relu)
        i += 1 + int(relu)
    return h


def _critic_mlp(dims_in: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(dims_in, NEURON_NUMS[0]), nn.ReLU(),
                         nn.Linear(NEURON_NUMS[0], NEURON_NUMS[1]), nn.ReLU(),
                         nn.Linear(NEURON_NUMS[1], 1))


class Hybrid_Critic(nn.Module):  # noqa: N801 (reference name)
    def __init__(self, input_dims, action_nums):
        super(Hybrid_Critic, self).__init__()
        self.input_dims = input_dims
        self.action_nums = action_nums
        if not 1 <= action_nums <= hip_ops.TD3_MAX_A:
            raise ValueError(f"Hybrid_Critic: action_nums outside [1, {hip_ops.TD3_MAX_A}]")

        deep_input_dims = self.input_dims + self.action_nums * 2

        self.bn_input = _BatchNorm1dV10(self.input_dims)

        self.mlp_1 = _critic_mlp(deep_input_dims)
        self.mlp_2 = _critic_mlp(deep_input_dims)

    def _cat(self, input, c_actions, d_actions):  # noqa: A002
        """cat([bn_input(input), d_actions, c_actions]): d before c."""
        bn = self.bn_input
        if not bn.training:
            return torch.cat([bn(input), d_actions, c_actions], dim=-1)
        if input.shape[0] < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input "
                             f"size {tuple(input.shape)}")
        bn.num_batches_tracked.add_(1)
        return _CriticInput.apply(input, d_actions, c_actions, bn.weight, bn.bias,
                                  bn.running_mean, bn.running_var, bn.eps, bn.momentum)

    def _input_buffer(self, input):  # noqa: A002
        """The [B, input_dims + 2A] input with bn_input(state) in its first columns, for a
        caller that writes the action columns (d, then c) itself. No autograd."""
        B, D = input.shape
        buf = torch.empty(B, D + 2 * self.action_nums, dtype=torch.float32, device=input.device)
        with torch.no_grad():
            self.bn_input(input, out=buf[:, :D])
        return buf

    def evaluate(self, input, c_actions, d_actions):  # noqa: A002
        cat = self._cat(input, c_actions, d_actions)
        return _run_mlp(self.mlp_1, cat), _run_mlp(self.mlp_2, cat)

    def evaluate_q_1(self, input, c_actions, d_actions):  # noqa: A002
        cat = self._cat(input, c_actions, d_actions)
        return _run_mlp(self.mlp_1, cat)


def _draws(seed, B: int, A: int, normals: int, uniforms: int, device):
    """`normals` + `uniforms` [B, A] tensors of one seed: the normals are elements
    [0, normals B A) of td3_noise's stream, the uniforms come from the elements after them."""
    n = B * A
    out = []
    if normals:
        z = hip_ops.td3_noise(normals * n, seed, 0, device=device)
        out += [z[i * n:(i + 1) * n].view(B, A) for i in range(normals)]
    if uniforms:
        u = hip_ops.td3v10_uniform(uniforms * n, seed, normals * n, device=device)
        out += [u[i * n:(i + 1) * n].view(B, A) for i in range(uniforms)]
    return out


class Hybrid_Actor(nn.Module):  # noqa: N801 (reference name)
    def __init__(self, input_dims, action_nums):
        super(Hybrid_Actor, self).__init__()
        self.input_dims = input_dims
        self.action_dims = action_nums
        if not 1 <= action_nums <= hip_ops.TD3_MAX_A:
            raise ValueError(f"Hybrid_Actor: action_nums outside [1, {hip_ops.TD3_MAX_A}]")

        self.bn_input = _BatchNorm1dV10(self.input_dims)

        self.mlp = nn.Sequential(nn.Linear(self.input_dims, NEURON_NUMS[0]), nn.ReLU(),
                                 nn.Linear(NEURON_NUMS[0], NEURON_NUMS[1]), nn.ReLU())

        self.c_action_layer = nn.Sequential(nn.Linear(NEURON_NUMS[1], self.action_dims),
                                            nn.Tanh())
        self.d_action_layer = nn.Sequential(nn.Linear(NEURON_NUMS[1], self.action_dims))

    def _pre(self, input):  # noqa: A002
        """The c head's pre-activation and the d head's q values, [B, A] each."""
        feature_exact = _run_mlp(self.mlp, self.bn_input(input))
        return (_linear(self.c_action_layer[0], feature_exact, False),
                _linear(self.d_action_layer[0], feature_exact, False))

    def act(self, input, temprature, *, noise=None, seed=None):  # noqa: A002
        """(c_action_means, ensemble_c_actions, d_action, ensemble_d_actions [B, 1]); noise =
        (n_c, n_d, u), or seed=, or a seed drawn from torch's CPU generator. No autograd."""
        with torch.no_grad():
            pre_c, pre_d = self._pre(input)
            if noise is None:
                B, A = pre_c.shape
                noise = _draws(_rng_sample_seed() if seed is None else seed, B, A, 2, 1,
                               pre_c.device)
            n_c, n_d, u = noise
            r = hip_ops.td3v10_heads(hip_ops.V10_ACT, pre_c, pre_d, noise_c=n_c, noise_d=n_d,
                                     uniform=u, temperature=float(temprature))
        return r["c_means"], r["c_softmax"], r["d_action"], r["d_index"]

    def evaluate(self, input):  # noqa: A002
        """(tanh(c head), d head's q values), differentiable."""
        pre_c, pre_d = self._pre(input)
        return torch.tanh(pre_c), pre_d


def boltzmann_softmax(actions, temprature):
    return hip_ops.softmax_rows((actions / temprature).contiguous())


def gumbel_softmax_sample(logits, temprature=1.0, hard=False, eps=1e-20, uniform_seed=1.0, *,
                          uniform=None):
    """softmax((logits + g) / temprature) with g = -log(-log(u + 1e-20) + 1e-20) in one launch;
    uniform= gives u, else it is generated. hard: the one-hot of the row maximum, as the
    reference's straight-through form evaluates to. No autograd graph."""
    if eps != 1e-20:
        raise NotImplementedError("gumbel_softmax_sample: eps is fixed at the reference's 1e-20")
    with torch.no_grad():
        B, A = logits.shape
        if uniform is None:
            uniform, = _draws(_rng_sample_seed(), B, A, 0, 1, logits.device)
        y = hip_ops.td3v10_heads(hip_ops.V10_PLAIN, logits, logits, uniform=uniform,
                                 temperature=float(temprature), want_softmax=False,
                                 want_index=False)["d_action"]
        if hard:
            y_hard = (y == y.max(1, keepdim=True)[0]).float()
            y = (y_hard - y) + y
    return y


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
            data_len=10,
            train_batch_size=10,
            reward_decay=1.0,
            memory_size=4096000,
            batch_size=256,
            tau=0.01,  # for target network soft update
            device='cuda:0',
    ):
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.action_nums = action_nums
        self.campaign_id = campaign_id
        self.lr_C_A = lr_C_A
        self.lr_D_A = lr_D_A
        self.lr_C = lr_C
        self.data_len = data_len
        self.train_batch_size = train_batch_size
        self.gamma = reward_decay
        self.latent_dims = latent_dims
        self.memory_size = memory_size
        self.batch_size = batch_size
        self.tau = tau
        self.device = device

        setup_seed(1)

        self.memory_counter = 0

        self.input_dims = self.field_nums * (self.field_nums - 1) // 2 + self.field_nums * self.latent_dims

        self.memory = Memory(self.memory_size, self.field_nums + self.action_nums * 2 + 2, self.device)

        self.Hybrid_Actor = Hybrid_Actor(self.input_dims, self.action_nums).to(self.device)
        self.Hybrid_Critic = Hybrid_Critic(self.input_dims, self.action_nums).to(self.device)

        self.Hybrid_Actor_ = copy.deepcopy(self.Hybrid_Actor)
        self.Hybrid_Critic_ = copy.deepcopy(self.Hybrid_Critic)

        self.optimizer_a = DenseAdam(self.Hybrid_Actor.parameters(), lr=self.lr_C_A)
        self.optimizer_c = DenseAdam(self.Hybrid_Critic.parameters(), lr=self.lr_C)

        self.loss_func = nn.MSELoss(reduction='mean')

        self.learn_iter = 0
        self.policy_freq = 10

        self.temprature = 1.0
        self.temprature_min = 0.1
        self.anneal_rate = 1e-6

        self.max_grad_norm = 0.5  # clip_grad_norm_(…, 0.5), lines 516 and 550
        self.reg = 1e-2           # the actor loss's regulariser, line 546
        # the soft updates' device tables, built once (rebuilt only if a parameter moved)
        self._soft_tables: dict = {}
        if next(self.Hybrid_Critic.parameters()).is_cuda:  # (a host model constructs only)
            for net, tgt in ((self.Hybrid_Critic, self.Hybrid_Critic_),
                             (self.Hybrid_Actor, self.Hybrid_Actor_)):
                self._soft_table(net, tgt)
        self.last: dict = {}  # device tensors of the last learn

    def store_transition(self, transitions):
        self.memory.add_seeded(transitions)

    def choose_action(self, state, random, *, noise=None):  # noqa: A002 (reference name)
        self.Hybrid_Actor.eval()
        with torch.no_grad():
            if random:
                # the reference runs act first and discards it: an eval-mode forward without a
                # side effect, so it is not run
                B, A = state.shape[0], self.action_nums
                if noise is None:
                    noise = _draws(_rng_sample_seed(), B, A, 2, 0, state.device)
                n_c, n_d = noise
                r = hip_ops.td3v10_heads(hip_ops.V10_RANDOM, noise_c=n_c, noise_d=n_d)
                return r["c_means"], r["c_softmax"], r["d_action"], r["d_index"]
            out = self.Hybrid_Actor.act(state, self.temprature, noise=noise)

        self.Hybrid_Actor.train()
        return out

    def choose_best_action(self, state, *, noise=None):
        self.Hybrid_Actor.eval()
        with torch.no_grad():
            pre_c, pre_d = self.Hybrid_Actor._pre(state)
            B, A = pre_c.shape
            u = noise if noise is not None else \
                _draws(_rng_sample_seed(), B, A, 0, 1, pre_c.device)[0]
            r = hip_ops.td3v10_heads(hip_ops.V10_BEST, pre_c, pre_d, uniform=u,
                                     temperature=self.temprature_min)
        return r["d_index"], r["c_means"], r["c_softmax"]

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

    def to_next_state_c_actions(self, next_d_actions, next_c_actions, *, noise=None):
        """The rank mask with the 0.2-scaled noise (noise: [B, A] unit normals, or generated)."""
        if noise is None:
            B, A = next_c_actions.shape
            noise, = _draws(_rng_sample_seed(), B, A, 1, 0, next_c_actions.device)
        with torch.no_grad():
            return hip_ops.td3v10_rank_mask(next_d_actions, next_c_actions, noise=noise,
                                            want_keep=False)["c"]

    def to_current_state_c_actions(self, next_d_actions, next_c_actions):
        """The rank mask without noise. No autograd graph (learn differentiates it through
        ctr_td3v10_heads_backward)."""
        with torch.no_grad():
            return hip_ops.td3v10_rank_mask(next_d_actions, next_c_actions,
                                            want_keep=False)["c"]

    def learn(self, embedding_layer, *, sample=None, noise=None, return_tensor=False):
        self.learn_iter += 1

        if (self.learn_iter + 1) % 1000 == 0:
            # one linear step towards the floor: the distance left, times calls / batches per pass
            batches = self.data_len // self.train_batch_size
            gap = self.temprature - self.temprature_min
            self.temprature = max(self.temprature_min,
                                  self.temprature - gap * self.learn_iter / batches)

        F_, A = self.field_nums, self.action_nums
        actor_step = self.learn_iter % self.policy_freq == 0

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
        B, D = b_s.shape
        ISweights = ISweights.contiguous()

        if noise is None:
            n_d, n_c, u, u_actor = _draws(_rng_sample_seed(), B, A, 2, 2, b_s.device)
        else:
            n_d, n_c, u = noise["n_d"], noise["n_c"], noise["u"]
            u_actor = noise.get("u_actor")
            if actor_step and u_actor is None:
                raise ValueError("learn: this call updates the actor and needs noise['u_actor']")

        with torch.no_grad():
            pre_c, pre_d = self.Hybrid_Actor_._pre(b_s)
            cat_t = self.Hybrid_Critic_._input_buffer(b_s)
            # tanh, the noisy Gumbel softmax at the temperature and its argmax in one launch ...
            h = hip_ops.td3v10_heads(hip_ops.V10_ACT, pre_c, pre_d, noise_c=n_c, noise_d=n_d,
                                     uniform=u, temperature=float(self.temprature),
                                     want_softmax=False, want_index=False)
            # ... the rank mask with its noise and the clamp, into the action columns, in another
            hip_ops.td3v10_rank_mask(h["d_action"], h["c_means"], noise=n_c,
                                     out_c=cat_t[:, D + A:], out_d=cat_t[:, D:D + A],
                                     want_keep=False)
            q1_target = _run_mlp(self.Hybrid_Critic_.mlp_1, cat_t)
            q2_target = _run_mlp(self.Hybrid_Critic_.mlp_2, cat_t)

        q1, q2 = self.Hybrid_Critic.evaluate(b_s, b_c_a, b_d_a)

        out = hip_ops.td3_critic_loss(q1.detach(), q2.detach(), q1_target, q2_target, b_r,
                                      ISweights, float(self.gamma))
        critic_td_error = out["td"] * 0.5  # exact: a power of two
        c_params = list(self.Hybrid_Critic.parameters())
        grads = torch.autograd.grad([q1, q2], c_params, [out["dq1"], out["dq2"]])
        norm_c = hip_ops.clip_grad_norm_(grads, self.max_grad_norm)
        self.optimizer_c.zero_grad()
        for p, g in zip(c_params, grads):
            p.grad = g
        self.optimizer_c.step()

        self.memory.batch_update(choose_idx, critic_td_error)
        self.last = dict(q1=q1.detach(), q2=q2.detach(), q_target=out["q_target"],
                         td=critic_td_error, loss=out["loss"], grad_norm_c=norm_c)

        if actor_step:
            a_params = list(self.Hybrid_Actor.parameters())
            pre_c, d_q = self.Hybrid_Actor._pre(b_s)  # in whatever mode the actor is in
            with torch.no_grad():
                h = hip_ops.td3v10_heads(hip_ops.V10_PLAIN, pre_c.detach(), d_q.detach(),
                                         uniform=u_actor, temperature=self.temprature_min,
                                         want_softmax=False, want_index=False)
                cat = self.Hybrid_Critic._input_buffer(b_s)
                keep = hip_ops.td3v10_rank_mask(h["d_action"], h["c_means"],
                                                out_c=cat[:, D + A:], out_d=cat[:, D:D + A])["keep"]
            # only the actor's parameters get gradients: the critic's would be zeroed before
            # they are used, so its weight-gradient GEMMs never run
            for p in c_params:
                p.requires_grad_(False)
            try:
                cat.requires_grad_(True)
                q = _run_mlp(self.Hybrid_Critic.mlp_1, cat)
                # loss = mean(isw * (-q)): dq = -isw / B
                g_cat, = torch.autograd.grad([q], [cat], [ISweights.view_as(q) * (-1.0 / B)])
            finally:
                for p in c_params:
                    p.requires_grad_(True)
            d_pre_c, d_d_q = hip_ops.td3v10_heads_backward(
                g_cat[:, D + A:], g_cat[:, D:D + A], keep, h["c_means"], d_q.detach(),
                h["d_action"], self.temprature_min, self.reg)
            grads = torch.autograd.grad([pre_c, d_q], a_params, [d_pre_c, d_d_q])
            self.last["grad_norm_a"] = hip_ops.clip_grad_norm_(grads, self.max_grad_norm)
            self.optimizer_a.zero_grad()
            for p, g in zip(a_params, grads):
                p.grad = g
            self.optimizer_a.step()

            self.soft_update(self.Hybrid_Critic, self.Hybrid_Critic_)
            self.soft_update(self.Hybrid_Actor, self.Hybrid_Actor_)

        return out["loss"] if return_tensor else out["loss"].item()
