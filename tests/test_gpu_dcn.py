"""GPU checks of the DCN cross-network kernels (csrc/dcn.hip) against an fp64 evaluation of
the formulas written here, and of the FNN / DCN models against the reference's recorded run
(tests/golden/g_{fnn,dcn}*.npz), in the ensemble and through the pretraining driver.

Bars (the project's own): predictions rtol 1e-5 / atol 1e-7; gradients and kernel arrays
1e-5 relative + 1e-6 x max|expected| (conftest.assert_grad_close)."""
from __future__ import annotations

import functools
import shutil

import numpy as np
import pytest
import torch

from conftest import GOLDEN, assert_grad_close, load_golden

pytestmark = pytest.mark.gpu

# (B, D, L): D < wave and D % 4 != 0; one layer; B no multiple of a block; the C3 width
# (specialised); max L, wide (generic path); beyond every specialisation (1792); more rows
# than one pass of the backward's grid (strided batch loop + partial reduction)
SHAPES = [(7, 15, 5), (5, 416, 1), (259, 416, 5), (33, 1664, 5), (9, 2560, 8), (3, 4100, 5),
          (2500, 416, 5)]
FORMS = ["gL", "rank1", "both"]
PAD = 203
SENTINEL = -777.25


@functools.lru_cache(maxsize=None)
def _case(B, D, L):
    """Seeded fp32 inputs and the fp64 evaluation of forward and backward (all three forms)."""
    g = torch.Generator().manual_seed(1000 * B + D + L)
    r = 1.0 / np.sqrt(D)
    inp = dict(x0=torch.randn(B, D, generator=g) * 0.1,
               W=(torch.rand(L, D, generator=g) * 2 - 1) * r,
               b=torch.randn(L, D, generator=g) * 0.05,
               wt=(torch.rand(D, generator=g) * 2 - 1) * r,
               gL=torch.randn(B, D, generator=g) / B,
               gz=torch.randn(B, generator=g) / B)
    x0, W, b, wt, gL, gz = (v.double() for v in inp.values())
    xs, s, x = [x0], [], x0
    for i in range(L):
        si = (x * W[i]).sum(1)
        s.append(si)
        x = (x0 * si[:, None] + b[i]) + x
        xs.append(x)
    ref = dict(s=torch.stack(s, 1), xL=x, z=x @ wt)
    for form in FORMS:
        gg = torch.zeros_like(x0)
        if form in ("gL", "both"):
            gg = gg + gL
        if form in ("rank1", "both"):
            gg = gg + gz[:, None] * wt
        dx0, dW, db = torch.zeros_like(x0), torch.zeros_like(W), torch.zeros_like(W)
        for i in range(L - 1, -1, -1):
            db[i] = gg.sum(0)
            t = (gg * x0).sum(1)
            dx0 = dx0 + gg * s[i][:, None]
            dW[i] = (t[:, None] * xs[i]).sum(0)
            gg = gg + t[:, None] * W[i]
        dx0 = dx0 + gg
        ref[form] = dict(dx0=dx0, dW=dW, dbias=db, dw_tail=(gz[:, None] * x).sum(0))
    return inp, {k: ({kk: vv.numpy() for kk, vv in v.items()} if isinstance(v, dict)
                     else v.numpy()) for k, v in ref.items()}


def _dev(inp, cuda):
    return {k: v.to(cuda) for k, v in inp.items()}


def _close(actual, desired, what):
    a = actual.detach().cpu().numpy()
    d = np.asarray(desired).reshape(a.shape)
    err = np.abs(a - d).max() if a.size else 0.0
    print(f"[dcn] {what}: max err {err:.3g}, max |ref| {np.abs(d).max() if d.size else 0:.3g}")
    assert_grad_close(a, d, err_msg=what)


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


def _backward(ops, d, s, form, out=None, gL=None):
    gL = d["gL"] if gL is None else gL
    return ops.dcn_cross_backward(d["x0"], d["W"], d["b"], s,
                                  gL=gL if form in ("gL", "both") else None,
                                  gz=d["gz"] if form in ("rank1", "both") else None,
                                  w_tail=d["wt"] if form in ("rank1", "both") else None, out=out)


@pytest.mark.parametrize("B,D,L", SHAPES)
def test_cross_forward_vs_fp64(cuda, B, D, L):
    from rl_ctr_prediction_amd import hip_ops as ops
    inp, ref = _case(B, D, L)
    d = _dev(inp, cuda)
    both = ops.dcn_cross_forward(d["x0"], d["W"], d["b"], d["wt"], want_xl=True)
    for k in ("s", "xL", "z"):
        _close(both[k], ref[k], f"{(B, D, L)} {k}")
    xl_only = ops.dcn_cross_forward(d["x0"], d["W"], d["b"])
    assert xl_only["z"] is None and _bits(xl_only["xL"]) == _bits(both["xL"])
    assert _bits(xl_only["s"]) == _bits(both["s"])
    z_only = ops.dcn_cross_forward(d["x0"], d["W"], d["b"], d["wt"], want_xl=False)
    assert z_only["xL"] is None and _bits(z_only["z"]) == _bits(both["z"])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,D,L", SHAPES)
def test_cross_backward_vs_fp64(cuda, B, D, L, form):
    from rl_ctr_prediction_amd import hip_ops as ops
    inp, ref = _case(B, D, L)
    d = _dev(inp, cuda)
    s = ops.dcn_cross_forward(d["x0"], d["W"], d["b"], d["wt"], want_xl=False)["s"]
    r = _backward(ops, d, s, form)
    for k in ("dx0", "dW", "dbias"):
        _close(r[k], ref[form][k], f"{(B, D, L)} {form} {k}")
    if form == "gL":
        assert r["dw_tail"] is None
    else:
        _close(r["dw_tail"], ref[form]["dw_tail"], f"{(B, D, L)} {form} dw_tail")


@pytest.mark.parametrize("B,D,L", SHAPES)
def test_cross_strided_operands(cuda, B, D, L):
    """Row strides D + 203 (no multiple of 4: the scalar path) everywhere; the pad columns
    keep their sentinel bits."""
    from rl_ctr_prediction_amd import hip_ops as ops
    inp, ref = _case(B, D, L)
    d = _dev(inp, cuda)
    ld = D + PAD

    def padded(src=None):
        buf = torch.full((B, ld), SENTINEL, device=cuda)
        if src is not None:
            buf[:, :D] = src
        return buf

    xb, gb, ob, db = padded(d["x0"]), padded(d["gL"]), padded(), padded()
    ds = dict(d, x0=xb[:, :D])
    out = dict(s=torch.empty(B, L, device=cuda), xL=ob[:, :D], z=torch.empty(B, device=cuda))
    ops.dcn_cross_forward(ds["x0"], d["W"], d["b"], d["wt"], out=out)
    for k in ("s", "xL", "z"):
        _close(out[k], ref[k], f"strided {(B, D, L)} {k}")
    xl_only = dict(s=torch.empty(B, L, device=cuda), xL=padded()[:, :D], z=None)
    ops.dcn_cross_forward(ds["x0"], d["W"], d["b"], out=xl_only)
    assert _bits(xl_only["xL"]) == _bits(out["xL"])
    bo = dict(dx0=db[:, :D], dW=torch.empty(L, D, device=cuda),
              dbias=torch.empty(L, D, device=cuda), dw_tail=torch.empty(D, device=cuda))
    _backward(ops, ds, out["s"], "both", out=bo, gL=gb[:, :D])
    for k in ("dx0", "dW", "dbias", "dw_tail"):
        _close(bo[k], ref["both"][k], f"strided {(B, D, L)} {k}")
    want = torch.full((B, PAD), SENTINEL)
    for name, buf in (("x0", xb), ("gL", gb), ("xL", ob), ("dx0", db)):
        assert _bits(buf[:, D:]) == _bits(want), f"{name}: pad columns touched"


def test_cross_rows_do_not_depend_on_the_batch(cuda):
    """Rows 0, 1 and B-1 run alone at B = 1 give the bits they have inside the batch."""
    from rl_ctr_prediction_amd import hip_ops as ops
    B, D, L = 259, 416, 5
    inp, _ = _case(B, D, L)
    d = _dev(inp, cuda)
    full = ops.dcn_cross_forward(d["x0"], d["W"], d["b"], d["wt"], want_xl=True)
    bfull = _backward(ops, d, full["s"], "both")
    for r in (0, 1, B - 1):
        one = dict(d, x0=d["x0"][r:r + 1], gL=d["gL"][r:r + 1], gz=d["gz"][r:r + 1])
        f1 = ops.dcn_cross_forward(one["x0"], d["W"], d["b"], d["wt"], want_xl=True)
        for k in ("s", "xL", "z"):
            assert _bits(f1[k]) == _bits(full[k][r:r + 1]), (r, k)
        b1 = _backward(ops, one, full["s"][r:r + 1].contiguous(), "both")
        assert _bits(b1["dx0"]) == _bits(bfull["dx0"][r:r + 1]), r


def test_cross_backward_is_deterministic(cuda):
    from rl_ctr_prediction_amd import hip_ops as ops
    inp, _ = _case(2500, 416, 5)
    d = _dev(inp, cuda)
    s = ops.dcn_cross_forward(d["x0"], d["W"], d["b"], d["wt"], want_xl=False)["s"]
    a = {k: _bits(v) for k, v in _backward(ops, d, s, "both").items()}
    torch.cuda.synchronize()
    b = {k: _bits(v) for k, v in _backward(ops, d, s, "both").items()}
    assert a == b


def test_cross_generic_path_at_a_specialised_width(cuda, monkeypatch):
    """CTR_DCN_GENERIC forces the any-D kernels: several rows per block, so their batch loop
    and their in-workspace column sums run, at a shape the fp64 evaluation already covers."""
    from rl_ctr_prediction_amd import hip_ops as ops
    B, D, L = 259, 416, 5
    inp, ref = _case(B, D, L)
    d = _dev(inp, cuda)
    monkeypatch.setenv("CTR_DCN_GENERIC", "1")
    f = ops.dcn_cross_forward(d["x0"], d["W"], d["b"], d["wt"], want_xl=True)
    for k in ("s", "xL", "z"):
        _close(f[k], ref[k], f"generic {k}")
    r = _backward(ops, d, f["s"], "both")
    torch.cuda.synchronize()
    for k in ("dx0", "dW", "dbias", "dw_tail"):
        _close(r[k], ref["both"][k], f"generic {k}")


def test_cross_empty_batch_zero_fills(cuda):
    from rl_ctr_prediction_amd import hip_ops as ops
    D, L = 40, 3
    W, b, wt = torch.randn(L, D, device=cuda), torch.randn(L, D, device=cuda), torch.randn(D, device=cuda)
    x0 = torch.empty(0, D, device=cuda)
    f = ops.dcn_cross_forward(x0, W, b, wt, want_xl=True)
    assert f["s"].shape == (0, L) and f["xL"].shape == (0, D) and f["z"].shape == (0,)
    out = dict(dx0=torch.empty(0, D, device=cuda), dW=torch.full((L, D), 3.0, device=cuda),
               dbias=torch.full((L, D), 3.0, device=cuda), dw_tail=torch.full((D,), 3.0, device=cuda))
    ops.dcn_cross_backward(x0, W, b, f["s"], gz=torch.empty(0, device=cuda), w_tail=wt, out=out)
    for k in ("dW", "dbias", "dw_tail"):
        assert not out[k].any(), k


# ----------------------------------------------------------------------- models -------
def _golden(kind):
    out = {}
    for name in (f"g_{kind}.npz", f"g_{kind}_step1.npz", f"g_{kind}_step2.npz"):
        z = load_golden(name)
        out.update({k: z[k] for k in z.files})
    return out


def _model_from_golden(kind, g, dev):
    import rl_ctr_prediction_amd as P
    V, K = g["init/feature_embedding.weight"].shape
    F = g["x0"].shape[1]
    m = (P.DCN if kind == "dcn" else P.FNN)(V, F, K).to(dev)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    keys = [k[5:] for k in g if k.startswith("init/")]
    m.load_state_dict({k: torch.tensor(g[f"init/{k}"]) for k in keys}, strict=True)
    return m, keys


@pytest.mark.parametrize("kind", ["dcn", "fnn"])
def test_autograd_grads_and_adam_step_vs_reference(cuda, kind):
    g = _golden(kind)
    m, keys = _model_from_golden(kind, g, cuda)
    m.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    x, y = torch.tensor(g["x0"], device=cuda), torch.tensor(g["y0"], device=cuda)
    p = m(x)
    np.testing.assert_allclose(p.detach().cpu().numpy(), g["p0"], rtol=1e-5, atol=1e-7)
    with torch.no_grad():  # the no-grad path: z-only cross forward + the split final layer
        m.eval()
        np.testing.assert_allclose(m(x).cpu().numpy(), g["p0"], rtol=1e-5, atol=1e-7)
        m.train()
    loss = torch.nn.BCELoss()(p, y)
    assert loss.item() == pytest.approx(float(g["loss0"]), rel=1e-5)
    m.zero_grad()
    loss.backward()
    named = dict(m.named_parameters())
    assert sorted(named) == sorted(keys)
    for k in keys:
        assert named[k].grad is not None, k
        assert_grad_close(named[k].grad.cpu().numpy(), g[f"grad0/{k}"], err_msg=f"{kind} grad {k}")
    opt.step()
    x1 = torch.tensor(g["x1"], device=cuda)
    p1 = m(x1)
    np.testing.assert_allclose(p1.detach().cpu().numpy(), g["p1"], rtol=1e-5, atol=1e-7)
    with torch.no_grad():
        m.eval()
        np.testing.assert_allclose(m(x1).cpu().numpy(), g["p1"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("kind", ["dcn", "fnn"])
def test_dropout_forward_is_seeded(cuda, kind):
    import rl_ctr_prediction_amd as P
    torch.manual_seed(4)
    V, F, K, B = 300, 6, 8, 96
    m = (P.DCN if kind == "dcn" else P.FNN)(V, F, K).to(cuda)
    m.train()
    x = torch.randint(0, V, (B, F), device=cuda)
    outs = []
    for grad in (True, True, False, False):
        torch.manual_seed(11)
        with torch.set_grad_enabled(grad):
            p = m(x)
        assert p.shape == (B, 1)
        assert bool(((p > 0) & (p < 1)).all())
        outs.append(_bits(p))
    assert outs[0] == outs[1] and outs[2] == outs[3]
    torch.manual_seed(12)
    assert _bits(m(x)) != outs[0], "another seed must drop other elements"


def test_five_member_ensemble(cuda):
    """The reference's best ensemble (IPNN, DeepFM, FNN, DCN, FFM) through generate_preds."""
    import rl_ctr_prediction_amd as P
    from rl_ctr_prediction_amd import hip_ops
    from rl_ctr_prediction_amd.ensemble import generate_preds
    torch.manual_seed(2)
    V, F, K, B = 200, 4, 8, 32
    models = [P.InnerPNN(V, F, K), P.DeepFM(V, F, K), P.FNN(V, F, K), P.DCN(V, F, K),
              P.FFM(V, F, K)]
    model_dict = {i: mm.to(cuda).eval() for i, mm in enumerate(models)}
    M = len(models)
    x = torch.randint(0, V, (B, F), device=cuda)
    actions = torch.randint(1, M + 1, (B, 1), device=cuda)
    pw = torch.softmax(torch.randn(B, M, device=cuda), dim=1)
    ca = torch.rand(B, M, device=cuda) * 2 - 1
    labels = torch.randint(0, 2, (B, 1), device=cuda)
    y, r, rc = generate_preds(model_dict, x, actions, pw, ca, labels, cuda)
    assert y.shape == (B, 1) and r.shape == (B, 1) and rc.shape == (B, M)
    for t in (y, r, rc):
        assert bool(torch.isfinite(t.float()).all())
    with torch.no_grad():
        preds = torch.cat([model_dict[i](x).reshape(-1, 1).float() for i in range(M)], 1).contiguous()
    y2, r2, rc2 = hip_ops.ensemble_preds(preds, actions, pw, ca, labels)
    assert _bits(y) == _bits(y2) and _bits(r) == _bits(r2) and _bits(rc) == _bits(rc2)


@pytest.mark.parametrize("kind", ["DCN", "FNN"])
def test_driver_trains_saves_and_reloads(cuda, tmp_path, kind):
    from rl_ctr_prediction_amd import creat_data as Data
    from rl_ctr_prediction_amd import pretrain_main as PM
    (tmp_path / "data" / "toy").mkdir(parents=True)
    for f in (GOLDEN / "toy").iterdir():
        shutil.copy(f, tmp_path / "data" / "toy" / f.name)
    (tmp_path / "params").mkdir()
    data, params = str(tmp_path / "data") + "/", str(tmp_path / "params") + "/"
    PM.setup_seed(1)
    res = PM.main(data, "toy/", "", 10, kind, 2, 1e-3, 1e-5, "loss", 256, "cuda:0", params,
                  verbose=False)
    assert len(res["history"]) == 2
    for h in res["history"]:
        assert np.isfinite(h["train_loss"]) and np.isfinite(h["valid_loss"])
    assert 0.0 <= res["test_auc"] <= 1.0
    best = tmp_path / "params" / f"{kind}best.pth"
    assert best.exists()
    sd = torch.load(best, map_location=cuda, weights_only=True)
    g = _golden(kind.lower())
    assert set(sd) == {k[5:] for k in g if k.startswith("init/")}
    _, _, test_data, field_nums, feature_nums = PM.get_dataset(data, "toy/", "")
    fresh = PM.get_model(kind, feature_nums, field_nums, 10).to(cuda)
    fresh.load_state_dict(sd, strict=True)
    loader = PM.DeviceBatches(Data.libsvm_dataset(test_data[:, 1:], test_data[:, 0]), 256, cuda)
    preds, auc = PM.submission(fresh, loader, cuda)
    assert np.asarray(preds, dtype=np.float64).tobytes() == \
        np.asarray(res["test_preds"], dtype=np.float64).tobytes()
    assert 0.0 <= auc <= 1.0
