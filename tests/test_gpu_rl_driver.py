"""GPU tests of the hybrid TD3 ensemble driver and its new kernels: ctr_lr_forward (and LR
through autograd), ctr_per_store_step, ctr_ensemble_preds_ex, and
rl_ctr_prediction_amd.hybrid_td3_main_per against the reference's recorded run
(tests/golden/make_golden_rl.py; the margin rule is in tests/rl_driver_ref.py)."""
from __future__ import annotations

import shutil

import numpy as np
import pytest
import torch

import rl_driver_ref as R
from conftest import GOLDEN, AdamBound, assert_grad_close, grad_bound, load_golden, pred_deviation

pytestmark = pytest.mark.gpu

V_TOY, F_TOY = 1508, 39


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _hip():
    from rl_ctr_prediction_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------ lr_forward ---
@pytest.mark.parametrize("dt", [torch.int32, torch.int64])
@pytest.mark.parametrize("F", [1, 2, 39, 64])
def test_lr_forward(cuda, F, dt):
    """z against a float64 sum within 1e-5 |z| + 1e-6 x (the L1 norm of the summands), the bar
    of tests/small_kernel_refs.py's logits; p = sigmoid(z); a row's bits do not depend on B."""
    H = _hip()
    for V in (1, 1508):
        g = torch.Generator().manual_seed(100 * F + V)
        lin = torch.randn(V, 1, generator=g)
        bias = torch.tensor([0.37])
        x_all = torch.randint(0, V, (257, F), generator=g).to(dt)
        z_full = None
        for B in (257, 1, 63, 64, 65):
            x = x_all[:B]
            r = H.lr_forward(x.to(cuda), lin.to(cuda), bias.to(cuda))
            w = lin.double().numpy()[x.numpy().astype(np.int64), 0]
            z_ref = 0.37 + w.sum(1)
            mag = 0.37 + np.abs(w).sum(1)
            z = _np(r["z"]).astype(np.float64)
            assert z.shape == (B,)
            assert (np.abs(z - z_ref) <= 1e-5 * np.abs(z_ref) + 1e-6 * mag).all(), (V, B)
            np.testing.assert_allclose(_np(r["p"]), 1 / (1 + np.exp(-z)), rtol=1e-6, atol=1e-7)
            assert r["loss_elem"] is None and r["gz"] is None
            if z_full is None:
                z_full = _np(r["z"])
                seq = np.float32(0.37) + _seq_sum32(lin.numpy()[x.numpy().astype(np.int64), 0])
                np.testing.assert_array_equal(z_full, seq)  # the field-order sum, to the bit
            else:
                np.testing.assert_array_equal(_np(r["z"]), z_full[:B])


def _seq_sum32(w):
    acc = w[:, 0].astype(np.float32).copy()
    for f in range(1, w.shape[1]):
        acc = (acc + w[:, f].astype(np.float32)).astype(np.float32)
    return acc


def test_lr_forward_bce_head_at_saturation(cuda, golden):
    """z = lin[b] exactly (F = 1, bias 0): the fused head against g_bce.npz under the rule of
    test_fm_forward_saturated_gradient_is_exactly_zero."""
    H = _hip()
    g = golden("g_bce.npz")
    n = g["z"].size
    lin = torch.tensor(g["z"], device=cuda).view(n, 1)
    x = torch.arange(n, device=cuda).view(n, 1)
    r = H.lr_forward(x, lin, torch.zeros(1, device=cuda), labels=torch.tensor(g["y"], device=cuda))
    np.testing.assert_array_equal(_np(r["z"]), g["z"])
    np.testing.assert_allclose(_np(r["p"]), g["p"], rtol=1e-6, atol=0)
    gz = _np(r["gz"])
    assert (gz[g["gz"] == 0] == 0).all(), "saturated sigmoid must give a 0 gradient"
    np.testing.assert_allclose(gz, g["gz"], rtol=2e-5, atol=0)
    assert float(r["loss_elem"].mean()) == pytest.approx(float(g["loss"]), rel=1e-5)


@pytest.mark.parametrize("F", [3, 39])
def test_lr_forward_out_of_range_ids_flag_and_guards(cuda, F):
    """An id outside [0, V) raises the flag, reads row 0, and nothing but z / p is written:
    both live inside one buffer whose other words keep their pattern."""
    H = _hip()
    from rl_ctr_prediction_amd._lib import lib
    V, B, G = 50, 70, 64
    lin = torch.randn(V, 1, device=cuda)
    bias = torch.zeros(1, device=cuda)
    x = torch.randint(0, V, (B, F), device=cuda)
    x[3, F - 1] = V + 5
    x[B - 1, 0] = -1
    buf = torch.full((G + B + G + B + G,), -7.25, device=cuda)
    z, p = buf[G:G + B], buf[2 * G + B:2 * G + 2 * B]
    err = torch.zeros(1, dtype=torch.int32, device=cuda)
    lib.ctr_lr_forward(x.data_ptr(), 1, B, F, V, lin.data_ptr(), bias.data_ptr(), z.data_ptr(),
                       p.data_ptr(), None, 1.0, None, None, err.data_ptr(),
                       torch.cuda.current_stream().cuda_stream)
    xs = x.clone()
    xs[3, F - 1] = 0
    xs[B - 1, 0] = 0
    want = _np(lin)[_np(xs), 0].astype(np.float64).sum(1)
    np.testing.assert_allclose(_np(z), want, rtol=1e-5, atol=1e-5)
    guards = torch.cat([buf[:G], buf[G + B:2 * G + B], buf[2 * G + 2 * B:]])
    assert bool((guards == -7.25).all())
    with pytest.raises(IndexError):
        H.check_index_error(err)
    H.check_index_error(err)  # the flag was cleared


def test_lr_against_the_reference_record(cuda, golden):
    """The forward, the gradients and the parameters after two Adam steps through autograd
    (AutogradTrainer) against g_lr.npz, at conftest's bars."""
    from rl_ctr_prediction_amd import pretrain_main as PM
    g = golden("g_lr.npz")
    keys = [str(k) for k in g["keys"]]
    m = PM.get_model("LR", V_TOY, F_TOY, R.K)
    m.load_state_dict({k: torch.from_numpy(np.array(g[f"init/{k}"])) for k in keys})
    m = m.to(cuda)
    tr = PM.make_trainer("LR", m, 1e-3, 1e-5)
    assert isinstance(tr, PM.AutogradTrainer)
    bounds = {k: AdamBound(g[f"init/{k}"], 1e-3, 1e-5) for k in keys}
    for s in range(2):
        x = torch.from_numpy(g[f"x{s}"]).to(cuda)
        y = torch.from_numpy(g[f"y{s}"]).to(cuda)
        with torch.no_grad():
            p_eval = m(x)  # the inference path (one launch, fused sigmoid)
        assert pred_deviation(_np(p_eval), g[f"p{s}"]) <= 1e-5
        loss = tr.step(x, y.view(-1))
        assert float(loss) == pytest.approx(float(g[f"loss{s}"]), rel=1e-5)
        named = dict(m.named_parameters())
        for k in keys:
            tol = assert_grad_close(_np(named[k].grad), g[f"grad{s}/{k}"], err_msg=f"grad{s}/{k}")
            bounds[k].step(g[f"grad{s}/{k}"], tol)
            bounds[k].check(_np(named[k]), g[f"step{s + 1}/{k}"], err_msg=f"step{s + 1}/{k}")


def test_lr_backward_is_bitwise_repeatable(cuda):
    from rl_ctr_prediction_amd import LR
    torch.manual_seed(3)
    m = LR(200).to(cuda)
    x = torch.randint(0, 200, (257, 39), device=cuda)
    x[:, 0] = 7  # one row that owns 257 slots
    y = (torch.rand(257, 1, device=cuda) < 0.3).float()
    grads = []
    for _ in range(2):
        m.zero_grad()
        torch.nn.BCELoss()(m(x), y).backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    assert float(grads[0][1].abs().sum()) > 0


# -------------------------------------------------------------------- per_store_step ---
N_MEM, F_MEM, A_MEM = 64, 6, 3
T_MEM = F_MEM + 2 * A_MEM + 2


def _step_inputs(n, gen, idt=torch.int64, strided=False, dev="cpu"):
    ids = torch.randint(0, 5000, (n, F_MEM), generator=gen).to(idt)
    wide = torch.rand(n, 2 * A_MEM + 5, generator=gen) * 2 - 1
    c, d = wide[:, 1:1 + A_MEM], wide[:, 2 + A_MEM:2 + 2 * A_MEM]
    act = torch.randint(1, A_MEM + 1, (n, 1), generator=gen).to(idt)
    rw = torch.rand(n, 3, generator=gen)
    r = (rw[:, 1:2] < 0.5).float()
    if strided:
        wide, rw = wide.to(dev), (rw < 0.5).float().to(dev)
        c, d = wide[:, 1:1 + A_MEM], wide[:, 2 + A_MEM:2 + 2 * A_MEM]
        r = rw[:, 1:2]
        assert n < 2 or (not c.is_contiguous() and r.stride(0) == 3)
    else:
        c, d, r = c.contiguous().to(dev), d.contiguous().to(dev), r.to(dev)
    return ids.to(dev), c, d, act.to(dev), r


def _two_memories(cuda):
    """Two memories inside guarded buffers: (fused, composed, check_guards)."""
    from rl_ctr_prediction_amd import PrioritizedMemory
    G = 2 * T_MEM
    mems, bufs = [], []
    for _ in range(2):
        m = PrioritizedMemory(N_MEM, T_MEM, cuda)
        bm = torch.full((G + N_MEM * T_MEM + G,), -3.5, device=cuda)
        bp = torch.full((G + N_MEM + G,), -3.5, device=cuda)
        bm[G:-G] = 0
        bp[G:-G] = 0
        m.memory = bm[G:-G].view(N_MEM, T_MEM)
        m.prioritys_ = bp[G:-G].view(N_MEM, 1)
        mems.append(m)
        bufs += [(bm, G), (bp, G)]

    def guards_ok():
        return all(bool((b[:g] == -3.5).all()) and bool((b[-g:] == -3.5).all()) for b, g in bufs)
    return mems[0], mems[1], guards_ok


def _composed_add(mem, ids, c, d, act, r):
    trans = torch.cat([ids.float(), c, d, act.float(), r], dim=1)
    mem.add(torch.ones(len(trans), 1, device=trans.device), trans)


@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
@pytest.mark.parametrize("strided", [False, True])
def test_per_store_step_is_bitwise_the_composed_store(cuda, idt, strided):
    """add_step on one memory, casts + cat + add(ones) on a second: the same bits in memory and
    priorities after every call, the ring wrapping (40 + 40 > 64), n = 64, n = 0, start = 63."""
    fused, composed, guards_ok = _two_memories(cuda)
    gen = torch.Generator().manual_seed(17)
    composed.prioritys_[5] = 3.0  # larger than (1 + eps)^alpha: kept by the max
    fused.prioritys_[5] = 3.0
    for n in (40, 40, 64, 0, 47, 1, 40):  # 40 + 40 wraps; after 191 rows start = 63, then 0
        if n == 1:
            assert fused.memory_counter % N_MEM == 63
        args = _step_inputs(n, gen, idt, strided, cuda)
        fused.add_step(*args)
        _composed_add(composed, *args)
        assert fused.memory_counter == composed.memory_counter
        assert torch.equal(fused.memory, composed.memory), n
        assert torch.equal(fused.prioritys_, composed.prioritys_), n
        if n == 40 and fused.memory_counter == 40:
            assert float(fused.prioritys_[5]) == 3.0
    assert guards_ok()
    with pytest.raises(ValueError, match="do not fit"):
        fused.add_step(*_step_inputs(65, gen, idt, strided, cuda))
    with pytest.raises(ValueError, match=r"F \+ 2A \+ 2"):
        ids, c, d, act, r = _step_inputs(4, gen, idt, False, cuda)
        fused.add_step(ids[:, :5].contiguous(), c, d, act, r)


def test_per_store_step_converts_ids_as_torch_does(cuda):
    """Ids at and above 2^24 round to nearest even, the bits of torch's cast."""
    fused, composed, guards_ok = _two_memories(cuda)
    vals = [16777215, 16777216, 16777217, 16777218, 16777219, 33554431, 33554433, 2 ** 31 - 1,
            2 ** 40 + 2 ** 16 + 1, 0, 1, 5]
    ids = torch.tensor(vals, dtype=torch.int64, device=cuda).view(2, F_MEM)
    gen = torch.Generator().manual_seed(2)
    _, c, d, act, r = _step_inputs(2, gen, torch.int64, False, cuda)
    fused.add_step(ids, c, d, act, r)
    _composed_add(composed, ids, c, d, act, r)
    assert torch.equal(fused.memory, composed.memory)
    got = _np(fused.memory[:2, :F_MEM]).reshape(-1)
    assert got[0] == 16777215 and got[2] == 16777216 and got[4] == 16777220
    assert got[5] == 33554432
    ids32 = ids.clamp(max=2 ** 31 - 1).int()
    fused.add_step(ids32, c, d, act.int(), r)
    _composed_add(composed, ids32, c, d, act.int(), r)
    assert torch.equal(fused.memory, composed.memory) and guards_ok()


def test_store_step_is_store_transition(cuda):
    from rl_ctr_prediction_amd import Hybrid_TD3_Model
    agents = [Hybrid_TD3_Model(5000, field_nums=F_MEM, latent_dims=4, action_nums=A_MEM,
                               memory_size=N_MEM, batch_size=16, device=cuda) for _ in range(2)]
    ids, c, d, act, r = _step_inputs(50, torch.Generator().manual_seed(1), dev=cuda)
    agents[0].store_step(features=ids, c_actions=c, d_values=d, d_actions=act, rewards=r)
    agents[1].store_transition(torch.cat([ids.float(), c, d, act.float(), r], dim=1))
    assert torch.equal(agents[0].memory.memory, agents[1].memory.memory)
    assert torch.equal(agents[0].memory.prioritys_, agents[1].memory.prioritys_)
    assert agents[0].memory.memory_counter == 50


# ----------------------------------------------------------------- ensemble_preds_ex ---
@pytest.mark.parametrize("case", range(3))
def test_ensemble_preds_ex_vs_the_base_record(cuda, golden, case):
    """The base driver's generate_preds: y within the bar of test_ensemble_preds_vs_golden,
    the rewards exactly, the built ties included."""
    H = _hip()
    g = golden("g_ensemble_base.npz")
    k = lambda n: torch.tensor(g[f"c{case}_{n}"], device=cuda)  # noqa: E731
    y, r, rc = H.ensemble_preds_ex(k("preds"), k("actions"), k("pw"), k("labels"),
                                   tie_rewards=True, want_c_actions=False)
    assert rc is None
    np.testing.assert_allclose(_np(y), g[f"c{case}_y"], rtol=1e-6, atol=1e-7)
    np.testing.assert_array_equal(_np(r), g[f"c{case}_r"])
    # the returned c_actions are optional, and asking for them changes nothing else
    y2, r2, rc2 = H.ensemble_preds_ex(k("preds"), k("actions"), k("pw"), k("labels"),
                                      tie_rewards=True)
    assert torch.equal(y, y2) and torch.equal(r, r2) and tuple(rc2.shape) == tuple(k("pw").shape)
    # int32 actions and labels
    y3, r3, _ = H.ensemble_preds_ex(k("preds"), k("actions").int(), k("pw"), k("labels").int(),
                                    tie_rewards=True, want_c_actions=False)
    assert torch.equal(y, y3) and torch.equal(r, r3)


@pytest.mark.parametrize("case", range(4))
def test_ensemble_preds_ex_without_flags_is_the_old_entry_point(cuda, golden, case):
    H = _hip()
    g = golden("g_ensemble.npz")
    k = lambda n: torch.tensor(g[f"c{case}_{n}"], device=cuda)  # noqa: E731
    old = H.ensemble_preds(k("preds"), k("actions"), k("pw"), k("ca"), k("labels"))
    new = H.ensemble_preds_ex(k("preds"), k("actions"), k("pw"), k("labels"), k("ca"))
    assert all(torch.equal(a, b) for a, b in zip(old, new))
    np.testing.assert_array_equal(_np(new[1]), g[f"c{case}_r"])
    # the tie rule alone separates the two reward conventions
    _, r_tie, _ = H.ensemble_preds_ex(k("preds"), k("actions"), k("pw"), k("labels"), k("ca"),
                                      tie_rewards=True)
    mean = g[f"c{case}_preds"].mean(1)
    differ = _np(r_tie).ravel() != g[f"c{case}_r"].ravel()
    assert (np.abs(_np(new[0]).ravel()[differ] - mean[differ]) < 1e-6).all()
    if g[f"c{case}_preds"].shape[1] == 1:
        assert differ.any() and (_np(r_tie) == 1).all()  # M = 1: y is the mean on every row


# ------------------------------------------------------------------------ the driver ---
@pytest.fixture(scope="module")
def rec():
    return R.load()


@pytest.fixture(scope="module")
def toy():
    import pandas as pd
    tr = pd.read_csv(GOLDEN / "toy" / "train_.txt", header=None).values.astype(int)
    te = pd.read_csv(GOLDEN / "toy" / "test_.txt", header=None).values.astype(int)
    return tr, te


def seeded_models():
    from rl_ctr_prediction_amd import FFM, FM, LR
    torch.manual_seed(R.SEED_MODELS)
    models = [LR(V_TOY), FM(V_TOY, R.K), FFM(V_TOY, F_TOY, R.K)]
    with torch.no_grad():
        for m in models:
            for n, p in m.named_parameters():
                if n != "bias":
                    p.mul_(R.SCALE)
    return models


def setup(cuda, toy, seed=R.SEED_AGENT):
    """(driver module, agent, model_dict, state encoder, train loader, test loader) of the
    recorded run: make_golden_rl.py's construction on the device."""
    from rl_ctr_prediction_amd import Feature_Embedding
    from rl_ctr_prediction_amd import creat_data as Data
    from rl_ctr_prediction_amd import hybrid_td3_main_per as D
    tr, te = toy
    models = seeded_models()
    fm_state = {k: v.clone() for k, v in models[1].state_dict().items()}
    model_dict = {i: m.to(cuda).eval() for i, m in enumerate(models)}
    torch.manual_seed(seed)
    agent = D.get_model(R.ACTIONS, V_TOY, F_TOY, R.K, 1e-3, 1e-3, 4096, R.MEMORY, cuda, "toy/")
    assert agent.batch_size == 256
    fe = Feature_Embedding(V_TOY, F_TOY, R.K).to(cuda)
    fe.load_embedding(fm_state)
    train_loader = D.DeviceBatches(Data.libsvm_dataset(tr[:, 1:], tr[:, 0]), R.TRAIN_BATCH, cuda)
    test_loader = D.DeviceBatches(Data.libsvm_dataset(te[:, 1:], te[:, 0]), R.TEST_BATCH, cuda)
    return D, agent, model_dict, fe, train_loader, test_loader


class Judge:
    """tests/test_gpu_td3.py's rule: a quantity passes within max(10 x the reference's own
    fp32-to-fp64 gap, the gradient bar) of the fp64 record."""

    def __init__(self):
        self.rows = []

    def __call__(self, what, got, f32, f64, rows=None):
        got, f32, f64 = (np.asarray(a, dtype=np.float64) for a in (got, f32, f64))
        assert got.shape == f64.shape == f32.shape, (what, got.shape, f64.shape)
        if rows is not None:
            got, f32, f64 = got[rows], f32[rows], f64[rows]
        if not f64.size:
            return True
        gap = float(np.max(np.abs(f32 - f64)))
        bar = np.maximum(10.0 * gap, grad_bound(f64))
        frac = float(np.max(np.abs(got - f64) / bar))
        self.rows.append((what, gap, float(np.max(np.abs(got - f64))), frac))
        return frac <= 1.0

    def report(self, title):
        print(title + ": quantity, reference fp32-vs-fp64 gap, HIP distance to fp64, distance / bar")
        for what, gap, dist, frac in self.rows:
            print(f"  {what:44s} {gap:10.3g} {dist:10.3g} {frac:8.3g}")

    def failed(self):
        return [r for r in self.rows if r[3] > 1]


def capture_generate_preds(D, monkeypatch):
    calls = []
    real = D.generate_preds

    def gen(model_dict, features, actions, prob_weights, labels, device, mode=None):
        y, r = real(model_dict, features, actions, prob_weights, labels, device, mode)
        calls.append(dict(y=y, rewards=r, d_action=actions, prob_weights=prob_weights))
        return y, r
    monkeypatch.setattr(D, "generate_preds", gen)
    return calls


def check_batch(judge, g, tag, got, what):
    """One recorded batch: y and the weights under the judge rule, the actions and rewards where
    the margin rule keeps them; returns the number of examples left out."""
    keep_a, keep_y, keep_r = R.keep_masks(g, tag)
    n = keep_a.size
    assert n - int(keep_r.sum()) <= R.MAX_DROPPED * n, (tag, int(keep_r.sum()), n)
    f = lambda k: g[f"{tag}/{k}"]        # noqa: E731
    d = lambda k: g[f"f64/{tag}/{k}"]    # noqa: E731
    ok = judge(f"{what} {tag}/prob_weights", _np(got["prob_weights"]), f("prob_weights"),
               d("prob_weights"))
    acts = _np(got["d_action"]).reshape(-1)
    assert np.array_equal(acts[keep_a], f("d_action").reshape(-1)[keep_a]), f"{what} {tag} actions"
    same = keep_y & (acts == f("d_action").reshape(-1))
    ok &= judge(f"{what} {tag}/y", _np(got["y"]).reshape(-1), f("y").reshape(-1),
                d("y").reshape(-1), rows=same)
    rew = _np(got["rewards"]).reshape(-1)
    assert np.array_equal(rew[keep_r], f("rewards").reshape(-1)[keep_r]), f"{what} {tag} rewards"
    return ok, n - int(keep_r.sum())


def test_driver_test_and_submission_against_the_record(cuda, toy, rec, monkeypatch):
    D, agent, model_dict, fe, _, test_loader = setup(cuda, toy)
    calls = capture_generate_preds(D, monkeypatch)
    judge = Judge()
    for metrics in ("host", "device"):
        del calls[:]
        auc, loss, rewards = D.test(agent, model_dict, fe, test_loader, torch.nn.BCELoss(), cuda,
                                    metrics=metrics)
        assert len(calls) == 4 and agent.Hybrid_Actor.training
        ok, dropped = True, 0
        for i, got in enumerate(calls):
            o, n = check_batch(judge, rec, f"t{i}", got, metrics)
            ok &= o
            dropped += n
        assert abs(auc - float(rec["f64/test/auc"])) <= 1e-6
        ok &= judge(f"{metrics} test/loss", [loss], [rec["test/loss"]], [rec["f64/test/loss"]])
        mine = sum(float(c["rewards"].sum()) for c in calls) / 4
        assert rewards == pytest.approx(mine, abs=1e-9)
        assert abs(rewards - float(rec["f64/test/rewards"])) <= dropped / 4 + 1e-9
    del calls[:]
    preds, auc, actions, weights = D.submission(agent, model_dict, fe, test_loader, cuda)
    preds_d, auc_d, actions_d, weights_d = D.submission(agent, model_dict, fe, test_loader, cuda,
                                                        metrics="device")
    assert np.array_equal(np.array(preds), np.array(preds_d)) and abs(auc - auc_d) <= 1e-12
    assert np.array_equal(actions, actions_d) and np.array_equal(weights, weights_d)
    assert abs(auc - float(rec["f64/sub/auc"])) <= 1e-6
    assert actions.shape == (200, 1) and weights.shape == (200, R.ACTIONS)
    ok &= judge("sub/y", np.array(preds), rec["sub/y"], rec["f64/sub/y"])
    ok &= judge("sub/prob_weights", weights, rec["sub/prob_weights"], rec["f64/sub/prob_weights"])
    keep = np.concatenate([R.keep_masks(rec, f"t{i}")[0] for i in range(4)])
    assert np.array_equal(actions.reshape(-1)[keep], rec["sub/actions"].reshape(-1)[keep])
    judge.report("driver test / submission")
    assert ok, judge.failed()


def recorded_draws(rec, cuda):
    t = lambda k: torch.from_numpy(np.array(rec[k])).to(cuda)  # noqa: E731
    for i in range(4):
        b = f"b{i}"
        yield dict(act_noise=(t(f"{b}/act_n_c"), t(f"{b}/act_n_d")),
                   sample=(t(f"{b}/idx"), t(f"{b}/batch"), t(f"{b}/isw")),
                   learn_noise=(t(f"{b}/n_c"), t(f"{b}/n_d")))


def test_driver_train_against_the_record(cuda, toy, rec, monkeypatch):
    """One epoch on the recorded draws: per batch the actions, y, rewards, the stored rows and
    the critic loss; after the fourth the priorities and the four networks."""
    D, agent, model_dict, fe, train_loader, _ = setup(cuda, toy)
    calls = capture_generate_preds(D, monkeypatch)
    stored, losses = [], []
    real_learn = agent.learn

    def learn(embedding_layer, **kw):
        n = calls[-1]["y"].shape[0]
        c = agent.memory.memory_counter
        stored.append(agent.memory.memory[c - n:c].clone())
        losses.append(real_learn(embedding_layer, **kw))
        return losses[-1]
    agent.learn = learn
    closs, rewards, auc, steps = D.train(agent, model_dict, train_loader, fe, 1.0, cuda,
                                         replay=recorded_draws(rec, cuda))
    assert steps == 4 and agent.learn_iter == 4 and len(calls) == 4
    assert [c["y"].shape[0] for c in calls] == [256, 256, 256, 32]
    judge = Judge()
    ok, dropped = True, 0
    A, F = R.ACTIONS, F_TOY
    for i, got in enumerate(calls):
        b = f"b{i}"
        o, n = check_batch(judge, rec, b, got, "train")
        ok &= o
        dropped += n
        rows, r32, r64 = _np(stored[i]), rec[f"{b}/rows"], rec[f"f64/{b}/rows"]
        keep_a, _, keep_r = R.keep_masks(rec, b)
        assert np.array_equal(rows[:, :F], r32[:, :F]), f"{b} stored ids"
        ok &= judge(f"{b}/rows c_actions, d_values", rows[:, F:F + 2 * A], r32[:, F:F + 2 * A],
                    r64[:, F:F + 2 * A])
        assert np.array_equal(rows[keep_a, F + 2 * A], r32[keep_a, F + 2 * A]), f"{b} stored action"
        assert np.array_equal(rows[keep_r, -1], r32[keep_r, -1]), f"{b} stored reward"
        assert np.array_equal(rows[:, F + 2 * A], _np(got["d_action"]).reshape(-1))
        assert np.array_equal(rows[:, -1], _np(got["rewards"]).reshape(-1))
        ok &= judge(f"{b}/loss", [losses[i]], [rec[f"{b}/loss"]], [rec[f"f64/{b}/loss"]])
    assert closs == losses[-1]
    assert abs(rewards - float(rec["f64/train/rewards"])) <= dropped / 4 + 1e-9
    assert abs(auc - float(rec["f64/train/auc"])) <= 1e-6
    ok &= judge("b3/prio", _np(agent.memory.prioritys_), rec["b3/prio"], rec["f64/b3/prio"])
    for n in ("Hybrid_Actor", "Hybrid_Actor_", "Critic", "Critic_"):
        for k, v in getattr(agent, n).state_dict().items():
            a, key = _np(v), f"b3/{n}/{k}"
            if key not in rec:
                a, key = a[::37, ::11], key + "@s"
            ok &= judge(key, a, rec[key], rec["f64/" + key])
    shown = Judge()
    shown.rows = [r for r in judge.rows if r[0].count("/") < 2 or r[3] > 0.5]
    shown.report("driver train")
    nets = [r for r in judge.rows if r[0].count("/") == 2]
    print(f"  networks: {len(nets)} entries, largest distance / bar {max(r[3] for r in nets):.3g}")
    assert ok, judge.failed()


def _epoch(cuda, toy, metrics, seed):
    D, agent, model_dict, fe, train_loader, _ = setup(cuda, toy, seed=seed)
    out = D.train(agent, model_dict, train_loader, fe, 1.0, cuda, metrics=metrics)
    state = [v.clone() for n in ("Hybrid_Actor", "Hybrid_Actor_", "Critic", "Critic_")
             for v in getattr(agent, n).state_dict().values()]
    return out, state + [agent.memory.memory.clone(), agent.memory.prioritys_.clone()]


def test_device_metrics_epoch_is_the_host_epoch_and_seeded_runs_repeat(cuda, toy):
    """metrics="device" (DeviceMetrics, store_step, tensor losses) leaves the bits of
    metrics="host" in the memory and the networks, and its AUC and rewards to 1e-12; two seeded
    free runs are bitwise equal."""
    (l_h, r_h, a_h, s_h), host = _epoch(cuda, toy, "host", 5)
    (l_d, r_d, a_d, s_d), dev = _epoch(cuda, toy, "device", 5)
    assert len(host) == len(dev) and all(torch.equal(a, b) for a, b in zip(host, dev))
    assert l_h == l_d and s_h == s_d == 4
    assert abs(r_h - r_d) <= 1e-12 and abs(a_h - a_d) <= 1e-12
    (l_2, r_2, a_2, _), again = _epoch(cuda, toy, "device", 5)
    assert all(torch.equal(a, b) for a, b in zip(dev, again))
    assert (l_2, r_2, a_2) == (l_d, r_d, a_d)
    _, other = _epoch(cuda, toy, "device", 6)
    assert not all(torch.equal(a, b) for a, b in zip(dev, other))  # the seed moves the draws


def test_device_metrics_epoch_makes_no_host_wait_before_compute(cuda, toy, monkeypatch):
    """One train epoch and one test under metrics="device": nothing waits for the device until
    DeviceMetrics.compute() (the technique of test_learn_makes_no_host_synchronisation)."""
    from rl_ctr_prediction_amd.metrics import DeviceMetrics
    D, agent, model_dict, fe, train_loader, test_loader = setup(cuda, toy)
    bce = torch.nn.BCELoss()
    for _ in range(2):  # warm-up: workspaces, the actor update and both soft updates
        D.train(agent, model_dict, train_loader, fe, 1.0, cuda, metrics="device")
    D.test(agent, model_dict, fe, test_loader, bce, cuda, metrics="device")
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    real_compute = DeviceMetrics.compute
    computes = []

    def compute(self):
        torch.cuda.set_sync_debug_mode(mode)  # the one wait the epoch is allowed
        computes.append(self.count)
        return real_compute(self)
    monkeypatch.setattr(DeviceMetrics, "compute", compute)
    try:
        torch.cuda.set_sync_debug_mode("error")
        out = D.train(agent, model_dict, train_loader, fe, 1.0, cuda, metrics="device")
        assert torch.cuda.get_sync_debug_mode() == mode
        torch.cuda.set_sync_debug_mode("error")
        res = D.test(agent, model_dict, fe, test_loader, bce, cuda, metrics="device")
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert computes == [800, 200]
    assert out[3] == 4 and np.isfinite(out[0]) and 0 <= res[0] <= 1


def test_main_end_to_end(cuda, tmp_path):
    """main on the toy set, two epochs, from *best.pth files of seeded models: the six outputs;
    and the ValueError for ids fp32 cannot hold."""
    from rl_ctr_prediction_amd import hybrid_td3_main_per as D
    data = tmp_path / "data" / "toy" / "c1"
    data.mkdir(parents=True)
    for f in ("train_.txt", "test_.txt", "featindex.txt"):
        shutil.copy(GOLDEN / "toy" / f, data / f)
    params = tmp_path / "params"
    (params / "c1").mkdir(parents=True)
    for name, m in zip(("LR", "FM", "FFM"), seeded_models()):
        torch.save(m.state_dict(), params / "c1" / f"{name}best.pth")
    D.setup_seed(1)
    out = D.main(str(tmp_path / "data") + "/", "toy/", "c1/", R.K, "Hybrid_TD3_V1", 1e-3, 1e-4,
                 1e-3, 3e-4, 1, 0.1, 2, 256, "cuda:0", str(params) + "/", metrics="device",
                 memory_size=4096, verbose=False)
    sub = data / "Hybrid_TD3_V1"
    import pandas as pd
    shapes = {"test_prob_weights.csv": (200, 4), "test_actions.csv": (200, 2),
              "test_submission.csv": (200, 2), "day_aucs.csv": (1, 2), "train_rewards.csv": (2, 2)}
    for f, shape in shapes.items():
        assert pd.read_csv(sub / f, header=None).shape == shape, f
    actor = torch.load(params / "c1" / "actor_modelbest.pth", weights_only=True)
    assert set(actor) == set(out["agent"].Hybrid_Actor.state_dict())
    assert len(out["history"]) == 2 and out["agent"].learn_iter == 8
    assert float(pd.read_csv(sub / "day_aucs.csv", header=None).values[0, 1]) == \
        pytest.approx(out["submission_auc"])
    assert 0.0 <= out["test_auc"] <= 1.0 and np.isfinite(out["test_loss"])

    big = tmp_path / "data" / "toy" / "big"
    big.mkdir()
    for f in ("train_.txt", "test_.txt"):
        shutil.copy(GOLDEN / "toy" / f, big / f)
    (big / "featindex.txt").write_text("0:v0\t0\n38:vbig\t%d\n" % (2 ** 24 + 1))
    with pytest.raises(ValueError, match=r"2\*\*24"):
        D.main(str(tmp_path / "data") + "/", "toy/", "big/", R.K, "Hybrid_TD3_V1", 1e-3, 1e-4,
               1e-3, 3e-4, 1, 0.1, 1, 256, "cuda:0", str(params) + "/")
