"""Plain-torch evaluation of the hybrid TD3 agent: the yardstick of the HIP path's tests, as
small_kernel_refs.py is for the small kernels. nn.BatchNorm1d, nn.Linear, torch ops and
torch.optim.Adam; any dtype, any device; the same ``sample=`` / ``noise=`` hooks as
rl_ctr_prediction_amd.hybrid_td3_model_per. Written from the agent's semantics:

  transition = [F ids | A c_actions | A d_actions | discrete action | reward]
  target actions = clamp(mean + clamp(0.2 n, -0.5, 0.5), -1, 1) of the TARGET actor's tanh heads
  q_target = r + gamma min(q1_t, q2_t);  td = 2 q_target - q1 - q2
  critic loss = mean(isw ((q1 - q_target)^2 + (q2 - q_target)^2)), Adam step on the critic
  every policy_freq-th learn: actor loss = -mean(q1(s, actor(s))), Adam step on the actor, then
    target = target (1 - tau) + net tau over parameters() (never the buffers)
  all four networks stay in training mode: batch statistics, running statistics updated at
    every forward (the critic's bn_input and mlp_1 twice in a learn with an actor update)
  discrete action = argmax + 1, the lowest index among equal values
"""
from __future__ import annotations

import copy
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

WIDTHS = (400, 300, 200)
GOLDEN = Path(__file__).resolve().parent / "golden"


# ------------------------------------------------- the recorded reference run ---------
def load_golden(names):
    """The arrays of several g_td3*.npz files in one dict (make_golden_td3.py)."""
    out = {}
    for n in names:
        with np.load(GOLDEN / n, allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out


def check_packed(gold, prefix, named, cmp, moments_rtol=1e-5):
    """Every (name, tensor) of `named` against gold[prefix/name]: vectors and small matrices in
    full, large matrices by their strided sample (@s) and their two fp64 moments (@m).
    cmp(actual, desired, what) compares; returns the number of entries seen.
    moments_rtol: for values that must be the recorded bytes pass 1e-12, which leaves room for
    nothing but the order of an fp64 sum (a changed element of size x moves the sum of squares
    by ~x^2, > 1e-8 of it for these matrices)."""
    seen = 0
    for k, t in named:
        a = t.detach().cpu().numpy()
        if f"{prefix}/{k}" in gold:
            cmp(a, gold[f"{prefix}/{k}"], f"{prefix}/{k}")
        else:
            cmp(a[::37, ::11], gold[f"{prefix}/{k}@s"], f"{prefix}/{k}@s")
            a64 = a.astype(np.float64)
            m = gold[f"{prefix}/{k}@m"]
            np.testing.assert_allclose([a64.sum(), (a64 * a64).sum()], m, rtol=moments_rtol,
                                       atol=moments_rtol * np.sqrt(m[1]),
                                       err_msg=f"{prefix}/{k}@m")
        seen += 1
    return seen


def _blocks(d, last):
    layers = []
    for n in WIDTHS:
        layers += [nn.Linear(d, n), nn.BatchNorm1d(n), nn.ReLU()]
        d = n
    if last:
        layers.append(nn.Linear(d, 1))
    return nn.Sequential(*layers)


class RefCritic(nn.Module):
    def __init__(self, input_dims, c_action_nums, d_action_nums):
        super().__init__()
        self.bn_input = nn.BatchNorm1d(input_dims)
        d = input_dims + c_action_nums + d_action_nums
        self.mlp_1 = _blocks(d, True)
        self.mlp_2 = _blocks(d, True)

    def cat(self, s, c, d):
        return torch.cat([self.bn_input(s), c, d], dim=1)

    def evaluate(self, s, c, d):
        x = self.cat(s, c, d)
        return self.mlp_1(x), self.mlp_2(x)

    def evaluate_q_1(self, s, c, d):
        return self.mlp_1(self.cat(s, c, d))


class RefActor(nn.Module):
    def __init__(self, input_dims, action_nums):
        super().__init__()
        self.bn_input = nn.BatchNorm1d(input_dims)
        self.mlp = _blocks(input_dims, False)
        self.c_action_layer = nn.Sequential(nn.Linear(WIDTHS[2], action_nums), nn.Tanh())
        self.d_action_layer = nn.Sequential(nn.Linear(WIDTHS[2], action_nums), nn.Tanh())

    def evaluate(self, s):
        h = self.mlp(self.bn_input(s))
        return self.c_action_layer(h), self.d_action_layer(h)


# ------------------------------------------------------------- elementwise pieces -----
def act_ref(c_mean, d_mean, noise=None, sigma=0.1):
    """From the tanh heads' outputs: (c_actions, softmax, d_actions, argmax + 1 [B, 1])."""
    if noise is not None:
        c = torch.clamp(c_mean + noise[0] * sigma, -1, 1)
        d = torch.clamp(d_mean + noise[1] * sigma, -1, 1)
    else:
        c, d = c_mean, d_mean
    return c, torch.softmax(c, dim=-1), d, (torch.argmax(d, dim=1) + 1).view(-1, 1)


def smooth_ref(c_mean, d_mean, noise):
    c = torch.clamp(c_mean + torch.clamp(noise[0] * 0.2, -0.5, 0.5), -1, 1)
    d = torch.clamp(d_mean + torch.clamp(noise[1] * 0.2, -0.5, 0.5), -1, 1)
    return c, d


def critic_loss_ref(q1, q2, q1_t, q2_t, r, isw, gamma):
    """dict(q_target, td, loss, dq1, dq2); q1 and q2 may carry an autograd graph."""
    q_target = r + gamma * torch.min(q1_t, q2_t)
    td = (2 * q_target - q1 - q2).detach()
    loss = (isw * (Fn.mse_loss(q1, q_target, reduction="none")
                   + Fn.mse_loss(q2, q_target, reduction="none"))).mean()
    n = q1.shape[0]
    return dict(q_target=q_target, td=td, loss=loss,
                dq1=(2 * isw * (q1 - q_target) / n).detach(),
                dq2=(2 * isw * (q2 - q_target) / n).detach())


def bn_ref(x, gamma, beta, rm, rv, eps, momentum, training, relu):
    """nn.BatchNorm1d's arithmetic in x's dtype: dict(y, mean, invstd, rm, rv)."""
    if training:
        n = x.shape[0]
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        rm = (1 - momentum) * rm + momentum * mean
        rv = (1 - momentum) * rv + momentum * var * n / (n - 1)
    else:
        mean, var = rm, rv
    invstd = 1 / torch.sqrt(var + eps)
    y = (x - mean) * invstd * gamma + beta
    return dict(y=torch.relu(y) if relu else y, mean=mean, invstd=invstd, rm=rm, rv=rv)


def embed_state(emb, ids):
    """The state encoder: pairwise inner products (i < j, row-major) ++ the flat embeddings."""
    e = emb[ids.long()]
    F = e.shape[1]
    row = [i for i in range(F - 1) for _ in range(i + 1, F)]
    col = [j for i in range(F - 1) for j in range(i + 1, F)]
    return torch.cat([(e[:, row] * e[:, col]).sum(2), e.reshape(e.shape[0], -1)], dim=1).detach()


def priority(td, eps=1e-3, alpha=0.6):
    return torch.pow(torch.abs(td) + eps, alpha)


# --------------------------------------------------------------------- the agent ------
class RefTD3:
    def __init__(self, input_dims, field_nums, action_nums, lr_a=1e-3, lr_c=1e-2, gamma=1,
                 tau=0.005, policy_freq=4, dtype=torch.float32, device="cpu", memory=None,
                 batch_size=256, instrument=True):
        """instrument: record what the parity tests compare (the gradients by name, the bias
        gradients' conditioning, dq1 / dq2). Off, learn runs the agent's own operations and
        nothing else and returns dict(loss): the form a timing takes as its baseline."""
        self.instrument = instrument
        self.F, self.A = field_nums, action_nums
        self.gamma, self.tau, self.policy_freq = gamma, tau, policy_freq
        self.dtype, self.device = dtype, device
        self.memory, self.batch_size = memory, batch_size
        self.Hybrid_Actor = RefActor(input_dims, action_nums).to(device=device, dtype=dtype)
        self.Critic = RefCritic(input_dims, action_nums, action_nums).to(device=device, dtype=dtype)
        self.Hybrid_Actor_ = copy.deepcopy(self.Hybrid_Actor)
        self.Critic_ = copy.deepcopy(self.Critic)
        self.optimizer_a = torch.optim.Adam(self.Hybrid_Actor.parameters(), lr=lr_a)
        self.optimizer_c = torch.optim.Adam(self.Critic.parameters(), lr=lr_c)
        self.learn_iter = 0
        # The conditioning of the bias gradients: a bias gradient is the column sum of the
        # gradient g at its module's output, and in front of a BatchNorm (every Linear but the
        # last ones, and bn_input) that sum is zero in exact arithmetic: what is left is
        # rounding noise, to be judged against sum_b |g[b, j]| (conftest.assert_grad_close's
        # `cond`), not against itself.
        self._cond = {}
        for tag, net in (("ga", self.Hybrid_Actor), ("gc", self.Critic)) if instrument else ():
            for name, mod in net.named_modules():
                before_bn = isinstance(mod, nn.Linear) and name.startswith("mlp") and \
                    mod.out_features > 1
                if before_bn or name == "bn_input":
                    mod.register_forward_hook(self._cond_hook((tag, f"{name}.bias")))

    def _cond_hook(self, key):
        def fwd(mod, inp, out):
            if out.requires_grad:
                out.register_hook(
                    lambda g: self._cond.__setitem__(key, g.detach().abs().sum(0)))
        return fwd

    def _conds(self, tag):
        return {k: v for (t, k), v in self._cond.items() if t == tag}

    def nets(self):
        return {n: getattr(self, n) for n in ("Hybrid_Actor", "Hybrid_Actor_", "Critic", "Critic_")}

    def load_from(self, agent):
        """Copy another agent's four networks and both Adam states (any dtype / device)."""
        for n, net in self.nets().items():
            sd = {k: v.detach().to(self.device) for k, v in getattr(agent, n).state_dict().items()}
            net.load_state_dict({k: v.to(self.dtype) if v.is_floating_point() else v
                                 for k, v in sd.items()}, strict=True)
        for mine, theirs, net, onet in ((self.optimizer_a, agent.optimizer_a, self.Hybrid_Actor,
                                         agent.Hybrid_Actor),
                                        (self.optimizer_c, agent.optimizer_c, self.Critic,
                                         agent.Critic)):
            mine.state.clear()
            for p, q in zip(net.parameters(), onet.parameters()):
                st = theirs.state.get(q)
                if st:
                    mine.state[p] = {
                        "step": torch.tensor(float(st["step"])),
                        "exp_avg": st["exp_avg"].detach().to(device=self.device, dtype=self.dtype).clone(),
                        "exp_avg_sq": st["exp_avg_sq"].detach().to(device=self.device,
                                                                   dtype=self.dtype).clone()}
        self.learn_iter = agent.learn_iter

    def soft_update(self, net, net_target):
        for pt, p in zip(net_target.parameters(), net.parameters()):
            pt.data.copy_(pt.data * (1.0 - self.tau) + p.data * self.tau)

    def choose_action(self, state, noise):
        self.Hybrid_Actor.eval()
        with torch.no_grad():
            out = act_ref(*self.Hybrid_Actor.evaluate(state), noise=noise)
        self.Hybrid_Actor.train()
        return out

    def choose_best_action(self, state):
        self.Hybrid_Actor.eval()
        with torch.no_grad():
            c, sm, d, ix = act_ref(*self.Hybrid_Actor.evaluate(state))
        self.Hybrid_Actor.train()
        return ix, sm

    def learn(self, embedding_layer, *, sample=None, noise=None, after_critic_step=None):
        """One learn. embedding_layer: ids [B, F] (long) -> state. Returns every intermediate:
        dict(q1, q2, q1_t, q2_t, q_target, td, loss, and gc / ga: the gradients by name).
        after_critic_step(): called right after the critic's Adam step (a teacher-forced
        comparison puts the other implementation's stepped parameters in here)."""
        self.learn_iter += 1
        F, A = self.F, self.A
        if sample is None:
            sample = self.memory.stochastic_sample(self.batch_size)
        idx, batch, isw = sample
        s = embedding_layer(batch[:, :F].long()).detach().to(self.dtype)
        batch, isw = batch.to(self.dtype), isw.to(self.dtype)
        c_a, d_a, r = batch[:, F:F + A], batch[:, F + A:F + 2 * A], batch[:, -1:]
        with torch.no_grad():
            c_m, d_m = self.Hybrid_Actor_.evaluate(s)
            if noise is None:
                noise = (torch.randn_like(c_m), torch.randn_like(d_m))
            noise = tuple(n.to(self.dtype) for n in noise)
            q1_t, q2_t = self.Critic_.evaluate(s, *smooth_ref(c_m, d_m, noise))
        q1, q2 = self.Critic.evaluate(s, c_a, d_a)
        if not self.instrument:
            return self._learn_bare(s, idx, q1, q2, q1_t, q2_t, r, isw)
        o = critic_loss_ref(q1, q2, q1_t, q2_t, r, isw, self.gamma)
        self.optimizer_c.zero_grad()
        o["loss"].backward()
        out = dict(q1=q1.detach(), q2=q2.detach(), q1_t=q1_t, q2_t=q2_t, q_target=o["q_target"],
                   td=o["td"], loss=o["loss"].detach(), dq1=o["dq1"], dq2=o["dq2"],
                   gc={n: p.grad.clone() for n, p in self.Critic.named_parameters()},
                   gc_cond=self._conds("gc"))
        self.optimizer_c.step()
        if after_critic_step is not None:
            after_critic_step()
        if self.memory is not None:
            self.memory.batch_update(idx, o["td"].float())
        if self.learn_iter % self.policy_freq == 0:
            c, d = self.Hybrid_Actor.evaluate(s)
            actor_loss = -self.Critic.evaluate_q_1(s, c, d).mean()
            self.optimizer_a.zero_grad()
            actor_loss.backward()
            out["ga"] = {n: p.grad.clone() for n, p in self.Hybrid_Actor.named_parameters()}
            out["ga_cond"] = self._conds("ga")
            self.optimizer_a.step()
            self.soft_update(self.Critic, self.Critic_)
            self.soft_update(self.Hybrid_Actor, self.Hybrid_Actor_)
        return out

    def _learn_bare(self, s, idx, q1, q2, q1_t, q2_t, r, isw):
        """The rest of a learn without any recording: the same operations in the same order."""
        q_target = r + self.gamma * torch.min(q1_t, q2_t)
        td = (2 * q_target - q1 - q2).detach()
        loss = (isw * (Fn.mse_loss(q1, q_target, reduction="none")
                       + Fn.mse_loss(q2, q_target, reduction="none"))).mean()
        self.optimizer_c.zero_grad()
        loss.backward()
        self.optimizer_c.step()
        if self.memory is not None:
            self.memory.batch_update(idx, td)
        if self.learn_iter % self.policy_freq == 0:
            c, d = self.Hybrid_Actor.evaluate(s)
            actor_loss = -self.Critic.evaluate_q_1(s, c, d).mean()
            self.optimizer_a.zero_grad()
            actor_loss.backward()
            self.optimizer_a.step()
            self.soft_update(self.Critic, self.Critic_)
            self.soft_update(self.Hybrid_Actor, self.Hybrid_Actor_)
        return dict(loss=loss.detach())
