"""Capture the golden records of LR, the base driver's generate_preds and the hybrid TD3
ensemble driver from the reference (survey container only), like make_golden_td3.py.

Imports jqsl2012/RL_CTR_Prediction from /root/reference (read-only, never copied) and runs it on
CPU (``torch.Tensor.cuda`` is made the identity in this process: hybrid_actors hard-codes
.cuda()). The fixtures are data: inputs, the draws the reference made and what it computed.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rl.py

g_lr.npz             p_model.LR(1508): seeded_init/* after torch.manual_seed(0), init/* (the
                     table scaled to N(0, 0.1), bias -0.1), then per step s of two Adam steps
                     (lr 1e-3, weight decay 1e-5) on toy rows [64 s, 64 s + 64): x, y, p, loss,
                     grad{s}/*, step{s+1}/* (make_golden_dcn.py's protocol).
g_ensemble_base.npz  src/all_main/hybrid_td3_main_per.generate_preds on (B, M) = (40, 1),
                     (64, 3), (257, 5) with stand-in models that return fixed pCTR columns:
                     c{i}_preds, actions, pw, labels, y, r. Every action value occurs. Rows
                     [0, 4 M) of a case have equal predictions in every model and alternate
                     a == 1 (y is that prediction) and a == M under uniform weights (y = sum p /
                     M): y ties with the models' mean as far as fp32 lets it, and the recorded
                     reward is the reference's; M = 1 ties on every row.
g_rl_driver*.npz     the driver on the toy set (F = 39, V = 1508), K = 4, models LR / FM / FFM
                     built after torch.manual_seed(11) in that order with every table
                     multiplied by 0.1 (not pretrained), Feature_Embedding.load_embedding given
                     the FM state, the agent built by the driver's get_model after
                     torch.manual_seed(0) with memory_size 1024. Recorded, in this order:
                     the reference's own test() and submission() on the 200 test rows at batch
                     64 (test/*, sub/*, per batch t{i}/*), then np.random.seed(0) and its own
                     train() on the 800 train rows at batch 256 (batches of 256, 256, 256, 32;
                     four learns, the fourth with the actor update), per batch b{i}/*:
                       act_n_c, act_n_d      choose_action's two unit-normal draws
                       c_actions, prob_weights, d_values, d_action, preds, y, rewards
                       rows                  the transitions stored
                       idx, batch, isw       learn's sample;  n_c, n_d  its two draws
                       loss                  the critic loss
                       d_gap, w_gap          top-two gap of d_values, smallest gap between
                                             adjacent sorted prob_weights
                     and train/* (its return values), b3/prio, b3/<net>/<key> (large matrices
                     as the strided sample @s and two fp64 moments @m).
                     train() runs through a two-method adapter subclass that drops the two
                     arguments the reference's loop passes and its model does not take.
                     Everything a second time in float64 with the same draws under f64/.
                     The script asserts that both runs agree on every example that
                     tests/rl_driver_ref.keep_masks keeps and that it keeps >= 98 % of each
                     batch.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path(os.environ.get("CTR_REFERENCE", "/root/reference"))
sys.path.insert(0, str(HERE.parent))
import rl_driver_ref as R  # noqa: E402

NETS = ("Hybrid_Actor", "Hybrid_Actor_", "Critic", "Critic_")


def _import_reference():
    if not REF.exists():
        raise SystemExit(f"{REF} not found: goldens are generated in the survey container only")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    torch.Tensor.cuda = lambda self, *a, **k: self  # this process only: the reference on CPU
    import src.all_main.hybrid_td3_main_per as D  # noqa: E402
    import src.models.Feature_embedding as FE  # noqa: E402
    import src.models.Hybrid_TD3_model_PER as M  # noqa: E402
    import src.models.creat_data as Data  # noqa: E402
    import src.models.p_model as P  # noqa: E402
    np.seterr(all="warn")  # the driver's module sets 'raise' process-wide at import
    return D, FE, M, Data, P


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


def toy():
    import pandas as pd
    tr = pd.read_csv(HERE / "toy" / "train_.txt", header=None).values.astype(int)
    te = pd.read_csv(HERE / "toy" / "test_.txt", header=None).values.astype(int)
    return tr, te


# ------------------------------------------------------------------------------ LR -----
def gen_lr(P):
    out = {}
    V = 1508
    tr, _ = toy()
    torch.manual_seed(0)
    m = P.LR(V)
    keys = list(m.state_dict())
    out["keys"] = np.array(keys)
    for k, v in m.state_dict().items():
        out[f"seeded_init/{k}"] = _np(v)
    with torch.no_grad():
        m.linear.weight.normal_(0, 0.1)
        m.bias.fill_(-0.1)
    for k, v in m.state_dict().items():
        out[f"init/{k}"] = _np(v)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    crit = torch.nn.BCELoss()
    for s in range(2):
        x = torch.from_numpy(tr[64 * s:64 * s + 64, 1:]).long()
        y = torch.from_numpy(tr[64 * s:64 * s + 64, :1]).float()
        p = m(x)
        loss = crit(p, y)
        m.zero_grad()
        loss.backward()
        out[f"x{s}"], out[f"y{s}"], out[f"p{s}"] = _np(x), _np(y), _np(p)
        out[f"loss{s}"] = np.float32(loss.item())
        named = dict(m.named_parameters())
        for k in keys:
            out[f"grad{s}/{k}"] = _np(named[k].grad)
        opt.step()
        for k, v in m.state_dict().items():
            out[f"step{s + 1}/{k}"] = _np(v)
    np.savez_compressed(HERE / "g_lr.npz", **out)


# ------------------------------------------------------------------- generate_preds -----
def gen_ensemble_base(D):
    out = {}
    g = torch.Generator().manual_seed(9)
    for case, (B, M) in enumerate([(40, 1), (64, 3), (257, 5)]):
        T = 4 * M  # tie rows: equal predictions in every model, every action, both labels
        preds = torch.rand(B, M, generator=g)
        actions = torch.randint(1, M + 1, (B, 1), generator=g)
        pw = torch.softmax(torch.randn(B, M, generator=g), dim=1)
        labels = torch.randint(0, 2, (B, 1), generator=g)
        for t in range(min(T, B)):
            # a == 1: y is the one prediction; a == M under uniform weights: y = sum p / M.
            # (1 < a < M would tie or not by the last bit of exp: no exact tie to build.)
            preds[t, :] = preds[t, 0]
            actions[t, 0] = 1 if t % 2 == 0 else M
            labels[t, 0] = (t // 2) % 2
            if t % 2 == 1:
                pw[t, :] = 1.0 / M  # uniform weights over equal predictions
        assert set(actions.reshape(-1).tolist()) == set(range(1, M + 1))
        model_dict = {i: (lambda x, i=i: preds[:, i:i + 1]) for i in range(M)}
        feats = torch.zeros(B, 2, dtype=torch.long)
        y, r = D.generate_preds(model_dict, feats, actions, pw, labels, "cpu", "train")
        for k, v in dict(preds=preds, actions=actions, pw=pw, labels=labels, y=y, r=r).items():
            out[f"c{case}_{k}"] = _np(v)
        out[f"c{case}_ties"] = np.int64(min(T, B))
    np.savez_compressed(HERE / "g_ensemble_base.npz", **out)


# ------------------------------------------------------------------------- the driver ---
def run_driver(mods, f64, replay):
    D, FE, M, Data, P = mods
    rec, big = {}, {}
    tr, te = toy()
    F, V, K = tr.shape[1] - 1, 1508, R.K
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(R.SEED_MODELS)
    models = [P.LR(V), P.FM(V, K), P.FFM(V, F, K)]
    with torch.no_grad():
        for m in models:
            for n, p in m.named_parameters():
                if n != "bias":
                    p.mul_(R.SCALE)
    model_dict = {i: m.eval() for i, m in enumerate(models)}

    class Agent(M.Hybrid_TD3_Model):  # the two calls of the reference's train() that do not run
        def choose_action(self, state, exploration_rate):
            return super().choose_action(state)

        def store_transition(self, transitions, embedding_layer):
            return super().store_transition(transitions)

    torch.manual_seed(R.SEED_AGENT)
    real_cls = D.td3_model.Hybrid_TD3_Model
    D.td3_model.Hybrid_TD3_Model = Agent
    try:
        agent = D.get_model(R.ACTIONS, V, F, K, 1e-3, 1e-3, 4096, R.MEMORY, "cpu", "toy/")
    finally:
        D.td3_model.Hybrid_TD3_Model = real_cls
    assert agent.batch_size == 256
    fe = FE.Feature_Embedding(V, F, K)
    fe.load_embedding(models[1].state_dict())
    if f64:
        for n in NETS:
            getattr(agent, n).double()
        for m in models:
            m.double()
        fe.double()
        agent.memory.memory = agent.memory.memory.double()
        agent.memory.prioritys_ = agent.memory.prioritys_.double()
        torch.set_default_dtype(torch.float64)

    cur = {"tag": None, "noise": [], "eval": None}
    real_randn_like = torch.randn_like

    def randn_like(t, *a, **k):
        j = len(cur["noise"])
        if replay is None:
            n = real_randn_like(t, *a, **k)
        else:
            n = torch.from_numpy(replay[cur["tag"] + cur["names"][j]]).to(t.dtype)
        cur["noise"].append(n)
        return n

    real_sample = agent.memory.stochastic_sample

    def sample(bs):
        mem = agent.memory
        if replay is None:
            idx, batch, isw = real_sample(bs)
        else:  # the fp32 run's indices into this run's own memory (lines 65-84)
            idx = torch.from_numpy(replay[f"{cur['tag']}/idx"])
            filled = min(mem.memory_counter, mem.memory_size)
            min_prob = torch.min(mem.prioritys_[:filled, :])
            mem.beta = torch.min(torch.FloatTensor(
                [1., mem.beta + mem.beta_increment_per_sampling])).item()
            batch = mem.memory[idx]
            isw = torch.pow(torch.div(mem.prioritys_[idx], min_prob), -mem.beta)
        cur["sample"] = (idx, batch, isw)
        return idx, batch, isw

    agent.memory.stochastic_sample = sample
    real_update = agent.memory.batch_update
    real_add = agent.memory.add

    def add(td, transitions):
        cur["rows"] = transitions
        return real_add(td.to(agent.memory.prioritys_.dtype), transitions)

    agent.memory.add = add
    real_eval = agent.Hybrid_Actor.evaluate

    def evaluate(state):
        o = real_eval(state)
        cur["eval"] = o
        return o

    agent.Hybrid_Actor.evaluate = evaluate
    real_choose = agent.choose_action

    def choose_action(state, exploration_rate):
        cur["names"], cur["tag"] = ("/act_n_c", "/act_n_d"), f"b{count['b']}"
        cur["noise"] = []
        o = real_choose(state, exploration_rate)
        cur["act"], cur["act_noise"] = o, list(cur["noise"])
        cur["names"], cur["noise"] = ("/n_c", "/n_d"), []
        return o

    agent.choose_action = choose_action
    real_gen = D.generate_preds
    count = {"t": 0, "b": 0}

    def generate_preds(model_dict_, features, actions, prob_weights, labels, device, mode):
        y, r = real_gen(model_dict_, features, actions, prob_weights, labels, device, mode)
        preds = torch.cat([model_dict_[i](features).detach() for i in range(len(model_dict_))], 1)
        if mode == "test":
            t = f"{cur['phase']}{count['t']}"
            count["t"] += 1
            rec[f"{t}/d_values"] = _np(cur["eval"][1])
        else:
            t = f"b{count['b']}"
        cur["tag"] = t
        for k, v in dict(preds=preds, y=y, rewards=r, prob_weights=prob_weights,
                         d_action=actions).items():
            rec[f"{t}/{k}"] = _np(v)
        return y, r

    D.generate_preds = generate_preds
    real_learn = agent.learn

    def learn(embedding_layer):
        t = f"b{count['b']}"
        cur["tag"] = t
        c, _, d, _ = cur["act"]
        rec[f"{t}/c_actions"], rec[f"{t}/d_values"] = _np(c), _np(d)
        rec[f"{t}/rows"] = _np(cur["rows"])
        if replay is None:
            rec[f"{t}/act_n_c"], rec[f"{t}/act_n_d"] = (_np(n) for n in cur["act_noise"])
        loss = real_learn(embedding_layer)
        idx, batch, isw = cur["sample"]
        rec[f"{t}/idx"], rec[f"{t}/batch"], rec[f"{t}/isw"] = _np(idx), _np(batch), _np(isw)
        if replay is None:
            assert len(cur["noise"]) == 2
            rec[f"{t}/n_c"], rec[f"{t}/n_d"] = _np(cur["noise"][0]), _np(cur["noise"][1])
        rec[f"{t}/loss"] = np.float64(loss)
        rec[f"{t}/d_gap"] = R.top2_gap(rec[f"{t}/d_values"])
        rec[f"{t}/w_gap"] = R.min_sorted_gap(rec[f"{t}/prob_weights"])
        count["b"] += 1
        return loss

    agent.learn = learn
    agent.memory.batch_update = lambda idx, td: real_update(
        idx, td.to(agent.memory.prioritys_.dtype))

    def loader(data, bs):
        return torch.utils.data.DataLoader(Data.libsvm_dataset(data[:, 1:], data[:, 0]),
                                           batch_size=bs, num_workers=0)

    torch.randn_like = randn_like
    try:
        cur["phase"] = "t"
        bce = torch.nn.BCELoss()  # test() hands it labels.float(): cast for the float64 run
        auc, loss, rew = D.test(agent, model_dict, fe, loader(te, R.TEST_BATCH),
                                lambda y, t: bce(y, t.to(y.dtype)), "cpu")
        rec["test/auc"], rec["test/loss"], rec["test/rewards"] = (np.float64(v) for v in
                                                                  (auc, loss, rew))
        cur["phase"], count["t"] = "s", 0
        preds, auc, acts, weights = D.submission(agent, model_dict, fe, loader(te, R.TEST_BATCH),
                                                 "cpu")
        rec["sub/y"], rec["sub/auc"] = np.array(preds, dtype=np.float64), np.float64(auc)
        rec["sub/actions"], rec["sub/prob_weights"] = acts, weights
        np.random.seed(0)
        closs, rew, auc, steps = D.train(agent, model_dict, loader(tr, R.TRAIN_BATCH), fe, 1.0,
                                         "cpu")
        rec["train/loss"], rec["train/rewards"], rec["train/auc"], rec["train/steps"] = \
            np.float64(closs), np.float64(rew), np.float64(auc), np.int64(steps)
        assert steps == 4 and count["b"] == 4 and agent.learn_iter == 4
        for n in NETS:
            pack(big, f"b3/{n}", getattr(agent, n).state_dict().items())
        rec["b3/prio"] = _np(agent.memory.prioritys_)
    finally:
        torch.randn_like = real_randn_like
        D.generate_preds = real_gen
        torch.set_default_dtype(torch.float32)
    return rec, big


def check_margins(g):
    for tag in [f"t{i}" for i in range(4)] + [f"b{i}" for i in range(4)]:
        keep_a, keep_y, keep_r = R.keep_masks(g, tag)
        n = keep_a.size
        for name, k in (("action", keep_a), ("order", keep_y), ("reward", keep_r)):
            kept = int(k.sum())
            print(f"  {tag}: {name} kept {kept}/{n}")
            assert n - kept <= R.MAX_DROPPED * n, (tag, name, kept, n)
        a32, a64 = g[f"{tag}/d_action"].reshape(-1), g[f"f64/{tag}/d_action"].reshape(-1)
        assert np.array_equal(a32[keep_a], a64[keep_a]), tag
        r32, r64 = g[f"{tag}/rewards"].reshape(-1), g[f"f64/{tag}/rewards"].reshape(-1)
        assert np.array_equal(r32[keep_r], r64[keep_r]), tag


def gen_driver(mods):
    rec32, big32 = run_driver(mods, False, None)
    rec64, big64 = run_driver(mods, True, rec32)
    base = dict(rec32)
    base.update({f"f64/{k}": v for k, v in rec64.items()})
    check_margins(base)
    rows = {k: base.pop(k) for k in list(base) if k.split("/")[-1] in ("rows", "batch")}
    nets = dict(big32)
    nets.update({f"f64/{k}": v for k, v in big64.items()})
    for name, d in (("g_rl_driver.npz", base), ("g_rl_driver_b.npz", rows),
                    ("g_rl_driver_c.npz", nets)):
        np.savez_compressed(HERE / name, **d)


def main():
    mods = _import_reference()
    D, FE, M, Data, P = mods
    torch.set_num_threads(1)
    which = sys.argv[1:] or ["lr", "ensemble", "driver"]
    if "lr" in which:
        gen_lr(P)
    if "ensemble" in which:
        gen_ensemble_base(D)
    if "driver" in which:
        gen_driver(mods)
    for f in sorted(list(HERE.glob("g_lr.npz")) + list(HERE.glob("g_ensemble_base.npz"))
                    + list(HERE.glob("g_rl_driver*.npz"))):
        size = f.stat().st_size
        assert size < (1 << 20), f"{f.name}: {size} bytes"
        print(f"wrote {f.name} ({size} bytes)")


if __name__ == "__main__":
    main()
