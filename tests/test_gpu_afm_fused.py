"""The fused AFM step on the GPU: ctr_afm_head bit for bit against the two launches it replaces
(ctr_lr_forward + ctr_deepfm_head), the step-seeded dropout of ctr_afm_forward_step /
ctr_afm_backward_step against the plain entry points at a seed computed here, and
FusedAFMTrainer against the reference implementation's run (tests/golden/g_afm.npz), against
its own dense mode, against an ungraphed run, and through the toy driver.

Bars: bitwise wherever two paths of this project are compared; against the reference's run the
bars of tests/test_gpu_afm.py::test_two_autograd_trainer_steps_vs_reference (loss 1e-5
relative, conftest.assert_grad_close with the afm_refs L1 scales, conftest.AdamBound)."""
from __future__ import annotations

import functools
import shutil

import numpy as np
import pytest
import torch

import afm_refs as R
import gemm_refs as G
from conftest import GOLDEN, AdamBound, assert_grad_close, fused_grads, load_golden

pytestmark = pytest.mark.gpu

# (B, F, K): one pair and one column; the drivers' K = 10 with F below and at 15 (four rows a
# wave, G = 16); more rows than one block's waves hold; the C3 width (G = 32, two rows a
# wave); the largest F and K (G = 64, both columns of every dot lane)
SHAPES = [(1, 2, 1), (7, 3, 10), (5, 15, 10), (67, 8, 16), (4, 26, 64), (3, 64, 128)]
DROP_SHAPES = [(7, 3, 10), (4, 26, 64)]
V = 50
SEED = 0x1234_5678_9ABC_DEF1
GAMMA = 0x9E3779B97F4A7C15


def _hip():
    from rl_ctr_prediction_amd import hip_ops
    return hip_ops


@functools.lru_cache(maxsize=None)
def _case(shape):
    """The case() inputs of one shape (A = K) and the head's own operands, made once on the
    host and never written to."""
    B, F, K = shape
    c = R.case(B, F, K, K, V)
    g = torch.Generator().manual_seed(97 + 7 * B + 13 * F + 17 * K)
    c.lin = 0.3 * torch.randn(V, 1, generator=g)
    c.bias = 0.1 * torch.randn(1, generator=g)
    c.fc_w = torch.randn(1, K, generator=g) / K ** 0.5
    c.fc_b = 0.1 * torch.randn(1, generator=g)
    c.labels = (torch.rand(B, generator=g) < 0.4).float()
    return c


def _pooled(c, dev):
    hip = _hip()
    pooled, _ = hip.afm_forward(c.x.to(dev), c.E.to(dev), c.W1.to(dev), c.b1.to(dev),
                                c.w2.to(dev), c.b2.to(dev))
    return pooled


def _reference_head(c, dev, x, pooled, labels, mean_div):
    """The composition AFM.forward's no-grad path runs, with the BCE head."""
    hip = _hip()
    lin, bias, fc_w, fc_b = (t.to(dev) for t in (c.lin, c.bias, c.fc_w, c.fc_b))
    z_lr = hip.lr_forward(x, lin, bias, want_p=False)["z"]
    ref = hip.deepfm_head(pooled.contiguous(), fc_w, fc_b, z_lr, labels, mean_div)
    ref["dpooled"] = ref["gz"].view(-1, 1) * fc_w.view(1, -1)
    return ref


def _same_head(got, ref, B, K, what=""):
    for k in ("z", "p", "loss_elem", "gz"):
        assert torch.equal(got[k][:B], ref[k]), (what, k)
    assert torch.equal(got["dpooled"][:B, :K], ref["dpooled"]), (what, "dpooled")


# --------------------------------------------------------------------- head ----------
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_head_is_lr_forward_plus_deepfm_head_bitwise(cuda, shape, dtype):
    hip = _hip()
    c = _case(shape)
    B, F, K = shape
    x, labels = c.x.to(cuda).to(dtype), c.labels.to(cuda)
    pooled = _pooled(c, cuda)
    for mean_div in (float(B), 3.0 * B + 1.0):
        ref = _reference_head(c, cuda, x, pooled, labels, mean_div)
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        got = hip.afm_head(x, c.lin.to(cuda), c.bias.to(cuda), pooled, c.fc_w.to(cuda),
                           c.fc_b.to(cuda), labels, mean_div, err_flag=err)
        assert int(err.item()) == 0
        _same_head(got, ref, B, K, mean_div)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_head_strides_and_alignment_select_no_result(cuda, shape):
    """ldp = ldg = K + 3 and every operand one float off a 16-byte boundary: the same bits,
    and nothing outside the outputs' extents is written."""
    hip = _hip()
    c = _case(shape)
    B, F, K = shape
    x, labels = c.x.to(cuda), c.labels.to(cuda)
    pooled = _pooled(c, cuda)
    ref = _reference_head(c, cuda, x, pooled, labels, float(B))
    put = lambda t: G.carve(1, t.numel(), t.numel(), 1, cuda, values=t.reshape(1, -1)).view  # noqa: E731
    pl = G.carve(B, K, K + 3, 1, cuda, values=pooled.cpu())
    slabs = {k: G.carve(1, B, B, 1, cuda, fill=G.SENTINEL) for k in ("z", "p", "loss_elem", "gz")}
    slabs["dpooled"] = G.carve(B, K, K + 3, 1, cuda, fill=G.SENTINEL)
    out = {k: (s.view if k == "dpooled" else s.view.reshape(-1)) for k, s in slabs.items()}
    for t in (pl.view, out["dpooled"]):
        assert t.data_ptr() % 16 == 4
    hip.afm_head(x, put(c.lin).reshape(V, 1), put(c.bias).reshape(1), pl.view,
                 put(c.fc_w), put(c.fc_b).reshape(1), put(labels.cpu()).reshape(-1), float(B),
                 out=out)
    torch.cuda.synchronize()
    for k, s in slabs.items():
        assert s.pad_intact(), k
    _same_head(out, ref, B, K)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_head_rows_do_not_depend_on_the_batch(cuda, shape):
    hip = _hip()
    c = _case(shape)
    B, F, K = shape
    dev = lambda t: t.to(cuda)  # noqa: E731
    x, labels, pooled = dev(c.x), dev(c.labels), _pooled(c, cuda)
    args = (dev(c.lin), dev(c.bias))
    fc = (dev(c.fc_w), dev(c.fc_b))
    full = hip.afm_head(x, *args, pooled, *fc, labels, float(B))
    for r in sorted({0, B // 2, B - 1}):
        one = hip.afm_head(x[r:r + 1], *args, pooled[r:r + 1], *fc, labels[r:r + 1], float(B))
        for k in ("z", "p", "loss_elem", "gz", "dpooled"):
            assert torch.equal(one[k], full[k][r:r + 1]), (r, k)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["i64", "i32"])
def test_head_out_of_range_ids_read_row_zero_and_raise_the_flag(cuda, dtype):
    from rl_ctr_prediction_amd._lib import CTR_EFLAG_INDEX
    hip = _hip()
    c = _case((5, 15, 10))
    B, F, K = 5, 15, 10
    dev = lambda t: t.to(cuda)  # noqa: E731
    bad, fixed = c.x.clone().to(dtype), c.x.clone().to(dtype)
    bad[B - 1, 1], bad[0, 0] = V + 5, -1
    fixed[B - 1, 1], fixed[0, 0] = 0, 0
    pooled, labels = _pooled(c, cuda), dev(c.labels)
    res = []
    for x in (bad, fixed):
        err = torch.zeros(1, dtype=torch.int32, device=cuda)
        res.append((hip.afm_head(dev(x), dev(c.lin), dev(c.bias), pooled, dev(c.fc_w),
                                 dev(c.fc_b), labels, err_flag=err), int(err.item())))
    assert res[0][1] & CTR_EFLAG_INDEX and res[1][1] == 0
    for k in ("z", "p", "loss_elem", "gz", "dpooled"):
        assert torch.equal(res[0][0][k], res[1][0][k]), k


def test_head_empty_batch_writes_nothing(cuda):
    hip = _hip()
    c = _case((7, 3, 10))
    dev = lambda t: t.to(cuda)  # noqa: E731
    out = dict(z=torch.full((4,), 3.0, device=cuda), p=torch.full((4,), 3.0, device=cuda),
               loss_elem=torch.full((4,), 3.0, device=cuda), gz=torch.full((4,), 3.0, device=cuda),
               dpooled=torch.full((4, 10), 3.0, device=cuda))
    hip.afm_head(torch.empty(0, 3, dtype=torch.int64, device=cuda), dev(c.lin), dev(c.bias),
                 torch.empty(0, 10, device=cuda), dev(c.fc_w), dev(c.fc_b),
                 torch.empty(0, device=cuda), 1.0, out=out)
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t == 3.0).all()), k


# ------------------------------------------------------------ step-seeded dropout ----
def _fwd_bwd(c, dev, seed, step_dev=None, plain=False):
    hip = _hip()
    a = [t.to(dev) for t in (c.x, c.E, c.W1, c.b1, c.w2, c.b2)]
    kw = {} if plain else dict(step_dev=step_dev)
    pooled, attn = hip.afm_forward(*a, 0.2, seed, **kw)
    r = hip.afm_backward(*a, attn, c.dpooled.to(dev), 0.2, seed, **kw)
    return dict(pooled=pooled, attn=attn, **r)


@pytest.mark.parametrize("shape", DROP_SHAPES, ids=str)
def test_step_seeded_dropout_is_the_plain_entry_point_at_the_derived_seed(cuda, shape):
    c = _case(shape)
    keys = ("pooled", "attn", "dslot", "dW1", "db1", "dw2", "db2")
    step = torch.zeros(1, dtype=torch.int32, device=cuda)
    got = {}
    for t in (0, 1, 7):
        step.fill_(t)
        got[t] = _fwd_bwd(c, cuda, SEED, step_dev=step)
        want = _fwd_bwd(c, cuda, (SEED + t * GAMMA) % 2**64, plain=True)
        for k in keys:
            assert torch.equal(got[t][k], want[k]), (t, k)
    none = _fwd_bwd(c, cuda, SEED, step_dev=None)
    plain = _fwd_bwd(c, cuda, SEED, plain=True)
    for k in keys:
        assert torch.equal(none[k], plain[k]), k
        assert torch.equal(got[0][k], plain[k]), k  # t = 0 is the seed itself
    assert not torch.equal(got[0]["pooled"], got[1]["pooled"]), "the masks must move with t"
    assert not torch.equal(got[0]["dslot"], got[1]["dslot"])
    assert torch.equal(got[0]["attn"], got[1]["attn"])  # the softmax before dropout


# ------------------------------------------------------------------- trainer ---------
def _golden_model(g, dev, head="init"):
    from rl_ctr_prediction_amd import AFM
    Vg, K = g["init/feature_embedding.weight"].shape
    m = AFM(Vg, g["x0"].shape[1], K).to(dev)
    m.load_state_dict({k: torch.tensor(g[f"{head}/{k}"]) for k in R.KEYS}, strict=True)
    m.drop_p = 0.0  # the fixture was captured with the reference's dropouts switched off
    return m


def _trainer_grads(tr):
    """The last step's gradients of every parameter by state_dict key, the two tables'
    densified from the trainer's per-row sums (conftest.fused_grads)."""
    gE, gw, dense = fused_grads(tr)
    return {"feature_embedding.weight": gE, "linear.weight": gw, **dense}


def _check_grads(g, s, head, grads, what):
    """test_gpu_afm._check_grads on a dict of numpy gradients: every parameter gradient of
    step s against the recorded one; the attention sums and the table with the L1 scales of
    the fp64 reference at the same parameters. Returns the per-element bounds checked."""
    x, y = torch.tensor(g[f"x{s}"]), torch.tensor(g[f"y{s}"])
    _, _, _, r = R.model_grads({k: torch.tensor(g[f"{head}/{k}"]) for k in R.KEYS}, x, y)
    B, F = x.shape
    Vg, K = g["init/feature_embedding.weight"].shape
    scale_E = torch.zeros(Vg, K, dtype=torch.float64)
    scale_E.index_add_(0, x.reshape(-1), r["dslot_scale"].reshape(B * F, K))
    counts = torch.bincount(x.reshape(-1), minlength=Vg).clamp(min=1).numpy()
    conds = {"feature_embedding.weight": (scale_E.numpy(), counts),
             "attention_net.weight": (r["dW1_scale"].numpy(), None),
             "attention_net.bias": (r["db1_scale"].numpy(), None),
             "attention_softmax.weight": (r["dw2_scale"].reshape(1, -1).numpy(), None),
             "attention_softmax.bias": (r["db2_scale"].numpy(), None)}
    tols = {}
    for k in R.KEYS:
        cond, n_terms = conds.get(k, (None, None))
        tols[k] = assert_grad_close(np.asarray(grads[k]).reshape(g[f"grad{s}/{k}"].shape),
                                    g[f"grad{s}/{k}"], cond=cond, n_terms=n_terms,
                                    err_msg=f"{what} grad{s} {k}")
    return tols


def test_two_fused_steps_vs_reference(cuda):
    from rl_ctr_prediction_amd import FusedAFMTrainer
    from rl_ctr_prediction_amd.pretrain_main import make_trainer
    g = load_golden("g_afm.npz")
    m = _golden_model(g, cuda)
    m.train()
    tr = make_trainer("AFM", m, 1e-3, 1e-5, fused_afm=True)
    assert type(tr) is FusedAFMTrainer and tr.kind == "AFM" and tr.optimizer_mode == "deferred"
    tr.keep_grads = True
    named = dict(m.named_parameters())
    assert list(named) == list(R.KEYS)
    bounds = {k: AdamBound(g[f"init/{k}"], 1e-3, 1e-5) for k in R.KEYS}
    for s, head in ((0, "init"), (1, "step1")):
        x, y = torch.tensor(g[f"x{s}"], device=cuda), torch.tensor(g[f"y{s}"], device=cuda)
        loss = tr.step(x, y)
        assert float(loss) == pytest.approx(float(g[f"loss{s}"]), rel=1e-5)
        tols = _check_grads(g, s, head, _trainer_grads(tr), "fused")
        tr.flush()  # every row of both tables at step s + 1, as the reference's dense Adam
        for k in R.KEYS:
            bounds[k].step(g[f"grad{s}/{k}"], tols[k])
            bounds[k].check(named[k].detach().cpu().numpy(), g[f"step{s + 1}/{k}"],
                            err_msg=f"step{s + 1}/{k}")
    tr.check_errors()
    assert tr.step_count == 2 and tr.captures == 1


def test_optimizer_state_dict_loads_into_torch_adam(cuda):
    """optimizer_state_dict() lists the nine parameters in named_parameters() order, so
    torch.optim.Adam loads it and keeps stepping: after one more step with the fused step's
    gradients, torch's parameters equal the fused trainer's. Bar: both sides evaluate one Adam
    step in fp32 from the same state and gradients, a handful of roundings apart — 1e-6
    relative (16 ulp) with 1e-9 absolute, the bar of the FFM trainer's twin test."""
    from rl_ctr_prediction_amd import AFM, FusedAFMTrainer
    g = load_golden("g_afm.npz")
    m = _golden_model(g, cuda)
    m.train()
    tr = FusedAFMTrainer(m, lr=1e-3, weight_decay=1e-5)
    tr.keep_grads = True
    data = [(torch.tensor(g[f"x{s}"], device=cuda), torch.tensor(g[f"y{s}"], device=cuda))
            for s in (0, 1, 0)]
    for x, y in data[:2]:
        tr.step(x, y)
    st = tr.optimizer_state_dict()
    names = [n for n, _ in m.named_parameters()]
    assert names == list(R.KEYS) and sorted(st["state"]) == list(range(9))
    assert st["param_groups"][0]["params"] == list(range(9))
    for i, p in enumerate(m.parameters()):
        assert st["state"][i]["exp_avg"].shape == p.shape, names[i]
        assert st["state"][i]["exp_avg_sq"].shape == p.shape, names[i]
        assert float(st["state"][i]["step"]) == 2.0
    clone = AFM(m.feature_nums, m.field_nums, m.latent_dims).to(cuda)
    clone.load_state_dict(m.state_dict())
    opt = torch.optim.Adam(clone.parameters(), lr=1e-3, weight_decay=1e-5)
    opt.load_state_dict(st)
    tr.step(*data[2])
    grads = _trainer_grads(tr)
    for n, p in clone.named_parameters():
        p.grad = torch.tensor(grads[n], device=cuda).reshape(p.shape)
    opt.step()
    sd = m.state_dict()  # flushes
    for n, p in clone.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), sd[n].cpu().numpy(), rtol=1e-6,
                                   atol=1e-9, err_msg=n)


def _run_steps(cuda, K, mode="deferred", drop_p=0.0, use_graphs=True, seed=7):
    """6 fused steps at V, F, B = 2000, 4, 64 on ids drawn from 40 rows, 12 of them per step,
    so rows recur and skip steps (tests/test_gpu_wd.py::_run_steps)."""
    import rl_ctr_prediction_amd as P
    Vt, F, B = 2000, 4, 64
    gen = torch.Generator().manual_seed(21)
    pool = torch.randperm(Vt, generator=gen)[:40]
    batches = []
    for _ in range(6):
        sub = pool[torch.randperm(40, generator=gen)[:12]]
        batches.append((sub[torch.randint(0, 12, (B, F), generator=gen)].to(cuda),
                        (torch.rand(B, generator=gen) < 0.3).float().to(cuda)))
    torch.manual_seed(8)
    m = P.AFM(Vt, F, K).to(cuda)
    m.drop_p = drop_p
    m.train()
    with torch.no_grad():
        m.linear.weight.mul_(0.1)
    tr = P.FusedAFMTrainer(m, lr=1e-3, weight_decay=1e-5, seed=seed, optimizer_mode=mode)
    tr.use_graphs = use_graphs
    losses, captures = [], []
    for x, y in batches:
        losses.append(tr.step(x, y).item())
        captures.append(tr.captures)
    if use_graphs:  # the first step runs eagerly and captures, every later one replays
        assert captures[0] == 1 and captures[-1] == 1, captures
    else:
        assert captures[-1] == 0
    assert tr.step_count == 6
    tr.flush()
    tr.check_errors()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return losses, sd, tr.optimizer_state_dict()["state"]


def _same(a, b):
    (la, sa, oa), (lb, sb, ob) = a, b
    ok = la == lb and all(torch.equal(sa[k], sb[k]) for k in sa)
    return ok and all(torch.equal(oa[i][k], ob[i][k]) for i in oa
                      for k in ("exp_avg", "exp_avg_sq"))


@pytest.mark.parametrize("K", [16, 10])
def test_fused_step_modes_bitwise(cuda, K, monkeypatch):
    """optimizer_mode "deferred" == "dense" bitwise; two trainers from one state are bitwise
    identical; step 0 captures and 1-5 replay (asserted in _run_steps). K = 16 takes the fused
    scatter + apply — and the unfused pair with CTR_FUSE_APPLY=0, the same bits —, K = 10 the
    unfused pair."""
    deferred = _run_steps(cuda, K, "deferred")
    assert len(set(deferred[0])) == 6 and all(np.isfinite(deferred[0]))
    assert _same(deferred, _run_steps(cuda, K, "dense")), "deferred != dense"
    assert _same(deferred, _run_steps(cuda, K, "deferred")), "not deterministic"
    if K == 16:
        monkeypatch.setenv("CTR_FUSE_APPLY", "0")
        assert _same(deferred, _run_steps(cuda, K, "deferred")), "fused apply != unfused"


@pytest.mark.parametrize("K", [16, 10])
def test_dropout_advances_inside_the_replayed_graph(cuda, K):
    """drop_p = 0.2: two trainers with one seed are bitwise equal, another seed is not; the
    replayed graph gives the bits of the ungraphed launches, whose dropout seed is the same
    device step counter — a seed frozen at capture would replay step 0's masks instead."""
    a = _run_steps(cuda, K, drop_p=0.2)
    assert len(set(a[0])) == 6 and all(np.isfinite(a[0]))
    assert _same(a, _run_steps(cuda, K, drop_p=0.2)), "one seed, two results"
    assert _same(a, _run_steps(cuda, K, drop_p=0.2, use_graphs=False)), "graph != eager"
    assert not _same(a, _run_steps(cuda, K, drop_p=0.2, seed=8)), "the seed is ignored"
    assert not _same(a, _run_steps(cuda, K, drop_p=0.0)), "no dropout was applied"


def test_the_replay_does_not_repeat_step_zero_masks(cuda):
    """The same batch twice through one trainer (the second step is a replay): at a learning
    rate of 0 the parameters stay put, so the two losses differ only through the masks."""
    import rl_ctr_prediction_amd as P
    torch.manual_seed(5)
    m = P.AFM(300, 6, 8).to(cuda)
    m.train()
    tr = P.FusedAFMTrainer(m, lr=0.0, weight_decay=0.0, seed=3)
    x = torch.randint(0, 300, (96, 6), device=cuda)
    y = (torch.rand(96, device=cuda) < 0.3).float()
    losses = [tr.step(x, y).item() for _ in range(3)]
    assert tr.captures == 1 and len(set(losses)) == 3, losses
    m.eval()  # eval(): no dropout, so the steps repeat
    losses = [tr.step(x, y).item() for _ in range(2)]
    assert losses[0] == losses[1]


def test_index_error_and_reset(cuda):
    import rl_ctr_prediction_amd as P
    torch.manual_seed(2)
    m = P.AFM(100, 4, 8).to(cuda)
    tr = P.FusedAFMTrainer(m, lr=1e-3, weight_decay=1e-5)
    x = torch.randint(0, 100, (16, 4), device=cuda)
    y = torch.zeros(16, device=cuda)
    tr.step(x, y)
    tr.check_errors()  # nothing raised yet
    bad = x.clone()
    bad[3, 2] = 100
    tr.step(bad, y)
    with pytest.raises(IndexError):
        tr.check_errors()
    tr.check_errors()  # the flag was cleared
    assert tr.step_count == 2 and bool(tr.m_E.any()) and bool(tr.m_w.any())
    tr.reset_optimizer(lr=2e-3)
    assert tr.step_count == 0 and tr.lr == 2e-3
    for t in (tr.m_E, tr.v_E, tr.m_w, tr.v_w, tr.m_flat, tr.v_flat, tr.last):
        assert not bool(t.any())
    assert tr.step_ctr.tolist() == [0, 1]
    assert tr.optimizer_state_dict()["state"] == {}
    loss = tr.step(x, y)
    assert np.isfinite(loss.item()) and tr.step_count == 1 and tr.captures == 1


# -------------------------------------------------------------------- driver ---------
def test_toy_driver_afm_fused(cuda, tmp_path):
    """pretrain_main.main with --model_name AFM --afm_trainer fused on the toy files, 2 epochs
    (dropout on): its per-epoch training losses are bitwise a hand loop of FusedAFMTrainer.step
    over the same batches from the same seeded model; AFMbest.pth loads strict into a fresh AFM
    and reproduces the written test predictions."""
    import rl_ctr_prediction_amd as P
    from rl_ctr_prediction_amd import creat_data as Data
    from rl_ctr_prediction_amd import pretrain_main as PM
    (tmp_path / "data" / "toy").mkdir(parents=True)
    for f in (GOLDEN / "toy").iterdir():
        shutil.copy(f, tmp_path / "data" / "toy" / f.name)
    (tmp_path / "params").mkdir()
    data, params = str(tmp_path / "data") + "/", str(tmp_path / "params") + "/"
    K, EPOCHS, BATCH = 10, 2, 256
    args = PM._parser().parse_args(["--model_name", "AFM", "--afm_trainer", "fused"])
    assert args.afm_trainer == "fused"
    PM.setup_seed(1)
    res = PM.main(data, "toy/", "", K, args.model_name, EPOCHS, 1e-3, 1e-5, "loss", BATCH,
                  "cuda:0", params, verbose=False, afm_trainer=args.afm_trainer)
    assert isinstance(res["model"], P.AFM)
    # the hand loop
    _, train_data, test_data, field_nums, feature_nums = PM.get_dataset(data, "toy/", "")
    PM.setup_seed(1)
    m = PM.build_model("AFM", feature_nums, field_nums, K).to(cuda)
    tr = PM.make_trainer("AFM", m, 1e-3, 1e-5, fused_afm=True)
    assert type(tr) is P.FusedAFMTrainer
    batches = list(PM.DeviceBatches(Data.libsvm_dataset(train_data[:, 1:], train_data[:, 0]),
                                    BATCH, cuda))
    for e in range(EPOCHS):
        m.train()
        tr.reset_optimizer()
        total = 0.0
        for x, y in batches:
            total += tr.step(x, y).item()
        assert total / len(batches) == res["history"][e]["train_loss"], e
        assert np.isfinite(res["history"][e]["train_loss"])
    assert res["history"][1]["train_loss"] < res["history"][0]["train_loss"], "it must train"
    # the checkpoint
    fresh = P.AFM(feature_nums, field_nums, K)
    fresh.load_state_dict(torch.load(params + "AFMbest.pth", map_location="cpu",
                                     weights_only=True), strict=True)
    fresh = fresh.to(cuda).eval()
    loader = PM.DeviceBatches(Data.libsvm_dataset(test_data[:, 1:], test_data[:, 0]), BATCH, cuda)
    with torch.no_grad():
        preds = torch.cat([fresh(x) for x, _ in loader]).cpu().numpy()
    np.testing.assert_array_equal(preds, np.asarray(res["test_preds"], dtype=np.float32))
    with pytest.raises(ValueError, match="afm_trainer"):
        PM.main(data, "toy/", "", K, "AFM", 1, 1e-3, 1e-5, "loss", BATCH, "cuda:0", params,
                verbose=False, afm_trainer="other")
