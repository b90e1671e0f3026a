"""Capture the hybrid TD3 agent's golden record from the reference (survey container only),
like make_golden_dcn.py / make_golden_per.py.

Imports jqsl2012/RL_CTR_Prediction from /root/reference (read-only, never copied) and runs
src/models/Hybrid_TD3_model_PER.Hybrid_TD3_Model with src/models/Feature_embedding on CPU
(``torch.Tensor.cuda`` is made the identity in this process: hybrid_actors hard-codes .cuda()).
The fixtures are data: inputs, the draws the reference made and what it computed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_td3.py

Shapes: V, F, K, A, B = 200, 6, 4, 3, 16 (input_dims 39, transition length 14), memory 64.
Script: torch.manual_seed(0), construction; 40 transitions stored, then 40 more (the ring
wraps); np.random.seed(0); eight learns (the 4th and 8th include the actor update and the soft
updates); one choose_action and one choose_best_action on five states.
The script wraps torch.randn_like, memory.stochastic_sample and both optimizers' step in its
own process and records, per learn i:
  c{i}/idx, batch, isw        the sample;  c{i}/n_c, n_d  the two unit-normal noise tensors
  c{i}/q1, q2, q1_t, q2_t, q_target, td, loss
  c{i}/gc/<param>             Critic gradients at optimizer_c.step (every call)
  c{i}/ga/<param>             Hybrid_Actor gradients at optimizer_a.step (calls 3 and 7)
  c{i}/<net>/<key>            the four networks' state_dicts after the call; c{i}/prio
The same script runs a second time with every network in .double(), the same samples and the
same noise: the same names under f64/ (float64). The distance between the two runs is the
reference's own rounding error, the yardstick of the free-running parity test.
Every vector is recorded in full. A matrix of more than 4096 elements is recorded as the
strided sample [::37, ::11] (<key>@s) with its fp64 sum and sum of squares (<key>@m); seeded
construction reproduces the initial matrices.
Files (each under the repository's 1 MiB limit):
  g_td3.npz                 shapes, emb, transitions, states5, keys/*, seeded_init/*, the
                            samples, noise, q's and losses of both runs, act/*, best/*
  g_td3_f32_{a,b}.npz       gradients and states of calls 0-3 / 4-7, fp32 run
  g_td3_f64_{a,b,c,d}.npz   the same of calls 0-1 / 2-3 / 4-5 / 6-7, fp64 run
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path(os.environ.get("CTR_REFERENCE", "/root/reference"))
V, F, K, A, B = 200, 6, 4, 3, 16
MEM, CALLS = 64, 8
NETS = ("Hybrid_Actor", "Hybrid_Actor_", "Critic", "Critic_")


def _import_reference():
    if not REF.exists():
        raise SystemExit(f"{REF} not found: goldens are generated in the survey container only")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    torch.Tensor.cuda = lambda self, *a, **k: self  # this process only: the reference on CPU
    import src.models.Feature_embedding as FE  # noqa: E402
    import src.models.Hybrid_TD3_model_PER as M  # noqa: E402
    return M, FE


def _np(t):
    return t.detach().cpu().numpy().copy()


def pack(out, prefix, named):
    """Vectors and small matrices in full, large matrices as a sample and two moments."""
    for k, t in named:
        a = _np(t)
        if a.ndim == 2 and a.size > 4096:
            out[f"{prefix}/{k}@s"] = a[::37, ::11].copy()
            a64 = a.astype(np.float64)
            out[f"{prefix}/{k}@m"] = np.array([a64.sum(), (a64 * a64).sum()])
        else:
            out[f"{prefix}/{k}"] = a


def inputs():
    g = torch.Generator().manual_seed(5)
    emb = torch.randn(V, K, generator=g) * 0.5
    ids = torch.randint(0, V, (80, F), generator=g).float()
    c_a = torch.rand(80, A, generator=g) * 2 - 1
    d_a = torch.rand(80, A, generator=g) * 2 - 1
    disc = torch.randint(1, A + 1, (80, 1), generator=g).float()
    rew = (torch.rand(80, 1, generator=g) < 0.3).float() - 0.1 * torch.rand(80, 1, generator=g)
    trans = torch.cat([ids, c_a, d_a, disc, rew], dim=1)
    states5 = torch.randint(0, V, (5, F), generator=g)
    return emb, trans, states5


def run(M, FE, dtype, emb, trans, states5, replay):
    """One pass of the script. replay None: the fp32 run, which draws; else the fp32 run's
    record, whose samples and noise this run re-uses."""
    rec, big = {}, {}
    torch.manual_seed(0)
    agent = M.Hybrid_TD3_Model(V, field_nums=F, latent_dims=K, action_nums=A, memory_size=MEM,
                               batch_size=B, device="cpu")
    if replay is None:
        for n in ("Hybrid_Actor", "Critic"):
            sd = getattr(agent, n).state_dict()
            rec[f"keys/{n}"] = np.array(list(sd))
            pack(rec, f"seeded_init/{n}", sd.items())
    fe = FE.Feature_Embedding(V, F, K)
    fe.feature_embedding.weight.data.copy_(emb)
    if dtype == torch.float64:
        for n in NETS:
            getattr(agent, n).double()
        fe.double()
    agent.store_transition(trans[:40])
    agent.store_transition(trans[40:])
    np.random.seed(0)

    cur = {"i": 0, "noise": [], "q": None, "qt": None}
    real_randn_like = torch.randn_like

    def randn_like(t, *a, **k):
        j = len(cur["noise"])
        if replay is None:
            n = real_randn_like(t, *a, **k)
        else:
            n = torch.from_numpy(replay[cur["tag"] + ("/n_c", "/n_d")[j]]).to(t.dtype)
        cur["noise"].append(n)
        return n

    real_sample = agent.memory.stochastic_sample

    def sample(bs):
        if replay is None:
            idx, batch, isw = real_sample(bs)
        else:
            idx, batch, isw = (torch.from_numpy(replay[f"{cur['tag']}/{k}"])
                               for k in ("idx", "batch", "isw"))
            batch, isw = batch.to(dtype), isw.to(dtype)
        cur["sample"] = (idx, batch, isw)
        return idx, batch, isw

    agent.memory.stochastic_sample = sample
    real_update = agent.memory.batch_update
    agent.memory.batch_update = lambda idx, td: real_update(idx, td.float())

    def wrap_eval(net, slot):
        real = net.evaluate

        def ev(*a):
            o = real(*a)
            cur[slot] = o
            return o
        net.evaluate = ev

    wrap_eval(agent.Critic, "q")
    wrap_eval(agent.Critic_, "qt")

    def wrap_step(opt, net, tag):
        real = opt.step

        def step(*a, **k):
            pack(big, f"{cur['tag']}/{tag}", [(n, p.grad) for n, p in net.named_parameters()])
            return real(*a, **k)
        opt.step = step

    wrap_step(agent.optimizer_c, agent.Critic, "gc")
    wrap_step(agent.optimizer_a, agent.Hybrid_Actor, "ga")

    torch.randn_like = randn_like
    try:
        for i in range(CALLS):
            cur["tag"], cur["noise"] = f"c{i}", []
            loss = agent.learn(fe)
            t = f"c{i}"
            idx, batch, isw = cur["sample"]
            if replay is None:
                rec[f"{t}/idx"], rec[f"{t}/batch"], rec[f"{t}/isw"] = _np(idx), _np(batch), _np(isw)
                rec[f"{t}/n_c"], rec[f"{t}/n_d"] = _np(cur["noise"][0]), _np(cur["noise"][1])
            assert len(cur["noise"]) == 2
            q1, q2 = cur["q"]
            q1_t, q2_t = cur["qt"]
            q_target = batch[:, -1:] + agent.gamma * torch.min(q1_t, q2_t)  # lines 358-359
            td = 2 * q_target - q1 - q2                                      # line 363
            for k, v in (("q1", q1), ("q2", q2), ("q1_t", q1_t), ("q2_t", q2_t),
                         ("q_target", q_target), ("td", td)):
                rec[f"{t}/{k}"] = _np(v)
            rec[f"{t}/loss"] = np.float64(loss)
            for n in NETS:
                pack(big, f"{t}/{n}", getattr(agent, n).state_dict().items())
            rec[f"{t}/prio"] = _np(agent.memory.prioritys_)
        s5 = fe.forward(states5)
        cur["tag"], cur["noise"] = "act", []
        c, sm, d, ix = agent.choose_action(s5)
        if replay is None:
            rec["act/n_c"], rec["act/n_d"] = _np(cur["noise"][0]), _np(cur["noise"][1])
        rec["act/c_actions"], rec["act/c_softmax"] = _np(c), _np(sm)
        rec["act/d_actions"], rec["act/d_index"] = _np(d), _np(ix)
        assert agent.Hybrid_Actor.training
        ix, sm = agent.choose_best_action(s5)
        rec["best/d_index"], rec["best/c_softmax"] = _np(ix), _np(sm)
    finally:
        torch.randn_like = real_randn_like
    return rec, big


def main():
    M, FE = _import_reference()
    torch.set_num_threads(1)
    emb, trans, states5 = inputs()
    rec32, big32 = run(M, FE, torch.float32, emb, trans, states5, None)
    rec64, big64 = run(M, FE, torch.float64, emb, trans, states5, rec32)
    base = dict(rec32)
    base.update({f"f64/{k}": v for k, v in rec64.items()})
    base["shapes"] = np.array([V, F, K, A, B, MEM, CALLS])
    base["emb"], base["transitions"], base["states5"] = _np(emb), _np(trans), _np(states5)
    files = {"g_td3.npz": base}
    for name, lo, hi in (("g_td3_f32_a.npz", 0, 4), ("g_td3_f32_b.npz", 4, 8)):
        files[name] = {k: v for k, v in big32.items() if lo <= int(k.split("/")[0][1:]) < hi}
    for j, name in enumerate("abcd"):
        files[f"g_td3_f64_{name}.npz"] = {
            f"f64/{k}": v for k, v in big64.items() if 2 * j <= int(k.split("/")[0][1:]) < 2 * j + 2}
    for name, d in files.items():
        np.savez_compressed(HERE / name, **d)
        size = (HERE / name).stat().st_size
        assert size < (1 << 20), f"{name}: {size} bytes"
        print(f"wrote {name} ({size} bytes, {len(d)} arrays)")


if __name__ == "__main__":
    main()
