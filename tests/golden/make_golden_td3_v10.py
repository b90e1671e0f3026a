"""Capture the v10 hybrid TD3 agent's golden record from the reference (survey container only),
in the style of make_golden_td3.py.

Imports jqsl2012/RL_CTR_Prediction from /root/reference (read-only, never copied) and runs
src/models/v10_Hybrid_TD3_model_PER.Hybrid_TD3_Model with src/models/Feature_embedding on CPU
(``torch.Tensor.cuda`` is made the identity in this process). The fixtures are data: inputs,
the draws the reference consumed and what it computed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_td3_v10.py

Shapes: V, F, K, A, B = 200, 6, 4, 3, 16 (input_dims 39, transition length 14), memory 64,
data_len 80, train_batch_size 40.
Script: construction (the constructor seeds itself with 1); 40 transitions stored from a random
choose_action ("ra"); 40 more from a non-random one ("na"); 10 learns c0..c9 (c9 updates the
actor); one choose_best_action on five states ("best"), which leaves the actor in eval mode; 10
more learns c10..c19 (c19 updates the actor with bn_input in eval mode); 40 more transitions from
a non-random choose_action ("nb"): the ring wraps and the new rows' priority is a memory max
other than 1.

Every draw reaches the reference as a recorded full [B, A] tensor, from this script's own
generator (seeded with the input seed): torch.normal(mean, std) is replaced by
mean + std * n with n the next recorded unit normals, torch.randn_like by the next recorded
normals, and the uniforms of gumbel_softmax_sample (the module's ``Variable``) by the next
recorded uniforms, in the run's dtype. Inside the rank mask the reference calls torch.normal
once per (choice, column) group; the stand-in gives element (b, m) the draw n_c[b, m] whatever
group it lands in, by locating each value in the full c' tensor (whose values are asserted
unique). The sample indices are the reference's own (np.random.choice after its seed).
The same script runs a second time with every network in .double(), on the same draws and the
same samples (idx, batch, isw): the same names under f64/. The distance between the two runs
is the reference's own rounding error, the yardstick of the free-running parity test.

Recorded per learn i: c{i}/idx, batch, isw; n_d, n_c, u (target step), u_actor (actor steps);
c_next, next_d (the target actor's c' and the noisy Gumbel softmax), c_cur, d_soft (actor steps);
q1, q2, q1_t, q2_t, q_target, td, loss; gnorm_c / gnorm_a (the gradient norm before clipping);
temperature; gc/<param>, ga/<param> (the CLIPPED gradients at the optimizer step); the four
state_dicts and prio after the call. Per action call: its draws, states and four outputs.
A matrix of more than 4096 elements is recorded as the strided sample [::37, ::11] (<key>@s)
with its fp64 sum and sum of squares (<key>@m), td3_ref.check_packed's format.

Decision margin. In the recorded run every argmax (of next_d, d_soft, the actions' d values,
the best action's d_q + g) and every rank decision (the order of each row of c') is clear of the
fp32-versus-fp64 distance of the values it compares by at least 100 x (the bar of
tests/rl_driver_ref.py). Input seeds are tried in order until one holds; the seed is recorded.
The parity tests therefore exclude no example.
Files (each under the repository's 1 MiB limit; named g_v10_td3*, not g_td3v10*: test_td3_cpu.py
counts the base agent's fixtures by the glob g_td3*): g_v10_td3.npz (inputs, draws, samples, q's,
actions of both runs, keys/*, seeded_init/*), g_v10_td3_f32_{a,b}.npz and
g_v10_td3_f64_{a,b,c,d}.npz (gradients and states).
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
MEM, CALLS, DATA_LEN, TRAIN_BATCH = 64, 20, 80, 40
NETS = ("Hybrid_Actor", "Hybrid_Actor_", "Hybrid_Critic", "Hybrid_Critic_")
MARGIN = 100.0


def _import_reference():
    if not REF.exists():
        raise SystemExit(f"{REF} not found: goldens are generated in the survey container only")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    torch.Tensor.cuda = lambda self, *a, **k: self  # this process only: the reference on CPU
    import src.models.Feature_embedding as FE  # noqa: E402
    import src.models.v10_Hybrid_TD3_model_PER as M  # noqa: E402
    return M, FE


def _np(t):
    return t.detach().cpu().numpy().copy()


def pack(out, prefix, named):
    for k, t in named:
        a = _np(t)
        if a.ndim == 2 and a.size > 4096:
            out[f"{prefix}/{k}@s"] = a[::37, ::11].copy()
            a64 = a.astype(np.float64)
            out[f"{prefix}/{k}@m"] = np.array([a64.sum(), (a64 * a64).sum()])
        else:
            out[f"{prefix}/{k}"] = a


def inputs(seed):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(V, K, generator=g) * 0.5
    ids = torch.randint(0, V, (120, F), generator=g)
    # not only 0 / 1: the memory-wide max, which seeds new rows, then comes from this column
    rew = (torch.rand(120, 1, generator=g) < 0.3).float() + 0.25 * torch.rand(120, 1, generator=g)
    states5 = torch.randint(0, V, (5, F), generator=g)
    return emb, ids, rew, states5, g


class Draws:
    """The draws of one run: generated (fp32 run) or replayed from its record (fp64 run)."""

    def __init__(self, gen, replay, rec, dtype):
        self.gen, self.replay, self.rec, self.dtype = gen, replay, rec, dtype
        self.tag = None

    def get(self, name, shape, kind):
        key = f"{self.tag}/{name}"
        if self.replay is None:
            assert key not in self.rec, key
            if kind == "normal":
                t = torch.randn(*shape, generator=self.gen)
            else:  # (0, 1): the kernels' generated uniforms never reach 0
                t = torch.rand(*shape, generator=self.gen).clamp_(2.0 ** -25, 1 - 2.0 ** -24)
            self.rec[key] = _np(t)
        else:
            t = torch.from_numpy(self.replay[key])
            assert tuple(t.shape) == tuple(shape), key
        return t.to(self.dtype)


def run(M, FE, dtype, emb, ids, rew, states5, gen, replay):
    rec, big = {}, {}
    agent = M.Hybrid_TD3_Model(V, field_nums=F, latent_dims=K, action_nums=A, memory_size=MEM,
                               batch_size=B, data_len=DATA_LEN, train_batch_size=TRAIN_BATCH,
                               device="cpu")
    if replay is None:
        for n in ("Hybrid_Actor", "Hybrid_Critic"):
            sd = getattr(agent, n).state_dict()
            rec[f"keys/{n}"] = np.array(list(sd))
            pack(rec, f"seeded_init/{n}", sd.items())
    fe = FE.Feature_Embedding(V, F, K)
    fe.feature_embedding.weight.data.copy_(emb)
    if dtype == torch.float64:
        for n in NETS:
            getattr(agent, n).double()
        fe.double()
    dr = Draws(gen, replay, rec, dtype)
    cur = {"order": [], "mask": None, "uni": []}

    # ---- stand-ins for the reference's random sources ----------------------------------
    def normal(mean, std, *a, **k):
        if cur["mask"] is not None:  # a (choice, column) group of the rank mask: [g, 1]
            cfull, nfull = cur["mask"]
            out = torch.empty_like(mean)
            for r in range(mean.shape[0]):
                hit = (cfull == mean[r, 0]).nonzero()
                assert hit.shape[0] == 1, "values of c' are not unique"
                out[r, 0] = mean[r, 0] + std * nfull[hit[0, 0], hit[0, 1]]
            return out
        name = cur["order"].pop(0)
        return mean + std * dr.get(name, mean.shape, "normal")

    def randn_like(t, *a, **k):
        return dr.get(cur["order"].pop(0), t.shape, "normal")

    def variable(t, requires_grad=False):  # the uniforms of gumbel_softmax_sample
        return dr.get(cur["uni"].pop(0), t.shape, "uniform")

    real = dict(normal=torch.normal, randn_like=torch.randn_like, variable=M.Variable,
                clip=torch.nn.utils.clip_grad_norm_)

    def clip(params, max_norm, *a, **k):
        total = real["clip"](params, max_norm, *a, **k)
        cur["gnorm"].append(float(total))
        return total

    real_next, real_cur = agent.to_next_state_c_actions, agent.to_current_state_c_actions

    def to_next(next_d, next_c):
        n_c = dr.get("n_c", next_c.shape, "normal")
        assert np.unique(_np(next_c)).size == next_c.numel(), "values of c' are not unique"
        cur["mask"] = (next_c, n_c)
        try:
            out = real_next(next_d, next_c)
        finally:
            cur["mask"] = None
        rec[f"{dr.tag}/c_next"], rec[f"{dr.tag}/next_d"] = _np(next_c), _np(next_d)
        rec[f"{dr.tag}/c_masked"] = _np(out)
        return out

    def to_cur(d_soft, c_means):
        rec[f"{dr.tag}/c_cur"], rec[f"{dr.tag}/d_soft"] = _np(c_means), _np(d_soft)
        return real_cur(d_soft, c_means)

    agent.to_next_state_c_actions, agent.to_current_state_c_actions = to_next, to_cur

    real_sample = agent.memory.stochastic_sample

    def sample(bs):
        if replay is None:
            out = real_sample(bs)
        else:
            out = tuple(torch.from_numpy(replay[f"{dr.tag}/{k}"]) for k in ("idx", "batch", "isw"))
            out = (out[0], out[1].to(dtype), out[2].to(dtype))
        cur["sample"] = out
        return out

    agent.memory.stochastic_sample = sample
    real_update = agent.memory.batch_update
    agent.memory.batch_update = lambda idx, td: real_update(idx, td.float())

    def wrap_eval(net, slot):
        real_ev = net.evaluate

        def ev(*a):
            o = real_ev(*a)
            cur[slot] = o
            return o
        net.evaluate = ev

    wrap_eval(agent.Hybrid_Critic, "q")
    wrap_eval(agent.Hybrid_Critic_, "qt")

    def wrap_step(opt, net, tag):
        real_st = opt.step

        def step(*a, **k):
            pack(big, f"{dr.tag}/{tag}", [(n, p.grad) for n, p in net.named_parameters()])
            return real_st(*a, **k)
        opt.step = step

    wrap_step(agent.optimizer_c, agent.Hybrid_Critic, "gc")
    wrap_step(agent.optimizer_a, agent.Hybrid_Actor, "ga")

    def act_store(tag, rows, random):
        dr.tag = tag
        s = fe.forward(ids[rows])
        # act always runs (its draws are consumed), the random branch then draws twice more
        cur["order"], cur["uni"] = ["n_c", "n_d"] + (["r_c", "r_d"] if random else []), ["u"]
        c, sm, d, ix = agent.choose_action(s, random)
        assert not cur["order"] and not cur["uni"]
        assert agent.Hybrid_Actor.training == (not random)
        for k, v in (("c", c), ("softmax", sm), ("d", d), ("index", ix)):
            rec[f"{tag}/{k}"] = _np(v)
        trans = torch.cat([ids[rows].float(), c.float(), d.float(), ix.float(), rew[rows]], dim=1)
        rec[f"{tag}/transitions"] = _np(trans)
        agent.store_transition(trans)
        rec[f"{tag}/prio"] = _np(agent.memory.prioritys_)
        rec[f"{tag}/memory"] = _np(agent.memory.memory)

    def learns(lo, hi):
        for i in range(lo, hi):
            t = dr.tag = f"c{i}"
            actor = (i + 1) % agent.policy_freq == 0
            cur["order"], cur["uni"] = ["n_d"], ["u"] + (["u_actor"] if actor else [])
            cur["gnorm"] = []
            # the rank mask builds its result with torch.zeros: in the run's dtype
            torch.set_default_dtype(dtype)
            try:
                loss = agent.learn(fe)
            finally:
                torch.set_default_dtype(torch.float32)
            assert not cur["order"] and not cur["uni"] and len(cur["gnorm"]) == 1 + int(actor)
            idx, batch, isw = cur["sample"]
            if replay is None:
                rec[f"{t}/idx"], rec[f"{t}/batch"], rec[f"{t}/isw"] = _np(idx), _np(batch), _np(isw)
            q1, q2 = cur["q"]
            q1_t, q2_t = cur["qt"]
            q_target = batch[:, -1:] + agent.gamma * torch.min(q1_t, q2_t)
            td = (q_target * 2 - q1 - q2) / 2
            for k, v in (("q1", q1), ("q2", q2), ("q1_t", q1_t), ("q2_t", q2_t),
                         ("q_target", q_target), ("td", td)):
                rec[f"{t}/{k}"] = _np(v)
            rec[f"{t}/loss"] = np.float64(loss)
            rec[f"{t}/gnorm_c"] = np.float64(cur["gnorm"][0])
            if actor:
                rec[f"{t}/gnorm_a"] = np.float64(cur["gnorm"][1])
            rec[f"{t}/temperature"] = np.float64(agent.temprature)
            for n in NETS:
                pack(big, f"{t}/{n}", getattr(agent, n).state_dict().items())
            rec[f"{t}/prio"] = _np(agent.memory.prioritys_)

    torch.normal, torch.randn_like, M.Variable = normal, randn_like, variable
    torch.nn.utils.clip_grad_norm_ = clip
    try:
        act_store("ra", slice(0, 40), True)
        act_store("na", slice(40, 80), False)
        learns(0, 10)
        dr.tag = "best"
        cur["uni"] = ["u"]
        s5 = fe.forward(states5)
        ix, cm, sm = agent.choose_best_action(s5)
        with torch.no_grad():
            rec["best/d_q"] = _np(agent.Hybrid_Actor.evaluate(s5)[1])
        assert not cur["uni"] and not agent.Hybrid_Actor.training
        rec["best/index"], rec["best/c_means"], rec["best/softmax"] = _np(ix), _np(cm), _np(sm)
        learns(10, 20)
        assert not agent.Hybrid_Actor.training  # c19's actor update ran in eval mode
        act_store("nb", slice(80, 120), False)
    finally:
        torch.normal, torch.randn_like, M.Variable = real["normal"], real["randn_like"], \
            real["variable"]
        torch.nn.utils.clip_grad_norm_ = real["clip"]
    return rec, big


def _top2(v):
    s = np.sort(np.asarray(v, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def margins_hold(r32, r64):
    """Every argmax and rank decision clear of the fp32-vs-fp64 distance by MARGIN x."""
    worst = np.inf
    checks = []
    for i in range(CALLS):
        checks += [(f"c{i}/next_d", "argmax"), (f"c{i}/c_next", "rank")]
        if f"c{i}/d_soft" in r32:
            checks += [(f"c{i}/d_soft", "argmax"), (f"c{i}/c_cur", "rank")]
    checks += [("ra/d", "argmax"), ("na/d", "argmax"), ("nb/d", "argmax")]
    for key, kind in checks:
        a32, a64 = r32[key].astype(np.float64), r64[key].astype(np.float64)
        gap = float(np.max(np.abs(a32 - a64)))
        if kind == "argmax":
            clear = float(_top2(a64).min())
            same = np.array_equal(a32.argmax(1), a64.argmax(1))
        else:
            clear = float(np.min(np.diff(np.sort(a64, axis=1), axis=1)))
            same = np.array_equal(np.argsort(-a32, axis=1, kind="stable"),
                                  np.argsort(-a64, axis=1, kind="stable"))
        if not same or not clear > MARGIN * gap:
            print(f"  margin fails at {key}: clear {clear:.3g}, gap {gap:.3g}, same {same}")
            return False, 0.0
        worst = min(worst, clear / max(gap, 1e-300))
    # the best action: argmax(d_q + g) of the eval-mode actor
    u = r32["best/u"].astype(np.float64)
    g = -np.log(-np.log(u + 1e-20) + 1e-20)
    gap = float(np.max(np.abs(r32["best/d_q"].astype(np.float64) - r64["best/d_q"])))
    clear = float(_top2(r64["best/d_q"] + g).min())
    if not clear > MARGIN * gap or not np.array_equal(r32["best/index"], r64["best/index"]):
        print(f"  margin fails at best: clear {clear:.3g}, gap {gap:.3g}")
        return False, 0.0
    return True, min(worst, clear / max(gap, 1e-300))


def main():
    M, FE = _import_reference()
    torch.set_num_threads(1)
    for seed in range(5, 40):
        emb, ids, rew, states5, gen = inputs(seed)
        try:
            rec32, big32 = run(M, FE, torch.float32, emb, ids, rew, states5, gen, None)
        except AssertionError as e:
            print(f"input seed {seed}: {e}")
            continue
        rec64, big64 = run(M, FE, torch.float64, emb, ids, rew, states5, None, rec32)
        ok, worst = margins_hold(rec32, rec64)
        print(f"input seed {seed}: margin {'holds' if ok else 'fails'} (smallest clearance / "
              f"distance {worst:.3g})")
        if ok:
            break
    else:
        raise SystemExit("no input seed satisfies the decision margin")
    assert all(np.array_equal(rec32[k], rec64[k]) for k in rec32
               if k.split("/")[-1] in ("index",)), "discrete outputs differ between the runs"
    base = dict(rec32)
    base.update({f"f64/{k}": v for k, v in rec64.items()
                 if not k.startswith(("keys/", "seeded_init/"))})
    base["shapes"] = np.array([V, F, K, A, B, MEM, CALLS, DATA_LEN, TRAIN_BATCH])
    base["input_seed"] = np.array(seed)
    base["margin"] = np.array([MARGIN, worst])
    base["emb"], base["ids"], base["rewards"], base["states5"] = _np(emb), _np(ids), _np(rew), \
        _np(states5)
    files = {"g_v10_td3.npz": base}

    def calls(d, lo, hi, pre=""):
        return {pre + k: v for k, v in d.items() if lo <= int(k.split("/")[0][1:]) < hi}

    files["g_v10_td3_f32_a.npz"] = calls(big32, 0, 10)
    files["g_v10_td3_f32_b.npz"] = calls(big32, 10, 20)
    for j, name in enumerate("abcd"):
        files[f"g_v10_td3_f64_{name}.npz"] = calls(big64, 5 * j, 5 * j + 5, "f64/")
    for name, d in files.items():
        np.savez_compressed(HERE / name, **d)
        size = (HERE / name).stat().st_size
        assert size < (1 << 20), f"{name}: {size} bytes"
        print(f"wrote {name} ({size} bytes, {len(d)} arrays)")


if __name__ == "__main__":
    main()
