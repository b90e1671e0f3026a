"""The wave-per-example pair-input kernels built on stage_rows_wave (csrc/ctr_common.h) —
ctr_feature_embedding_forward(_planes) (csrc/fm_forward.hip), ctr_ipnn_forward(_planes) and
ctr_ipnn_backward (csrc/pnn.hip) — against tests/pair_input_refs.py at every edge of their
dispatch: the three staging paths, the aligned and the unaligned flat store, both LDS row
strides, the four backward kernels, both id types and dynamic LDS on both sides of 64 KB
(tests/test_pair_input_refs.py asserts on the CPU that pair_input_refs.EDGE_SHAPES takes every
label of every predicate).

Bars, all the project's own: the copied flat part bit-exact; the IPNN dots bitwise the fp32
emulation of the order the kernel promises ("torch.mul, then torch.sum", contraction off, k
ascending — both row strides); the three walks of the backward bitwise the emulation of
theirs (j ascending, j != f) and so one another; the matrix-core product, which sums inside
the matrix core, inside 1e-5 x the per-element L1 scale of the float64 gradient
(test_ipnn_forward_and_backward_vs_oracle's bar) and the same bits on a second launch.
Feature_Embedding's dot loop carries no contraction pragma, so the compiler may fuse its
multiply-adds and no order is promised: its dots are held to 1e-5 x their L1 scale around
float64, nothing tighter. On integer data (pair_input_refs.int_case) every order is exact, so
every kernel must return the int64 result as it is — a dropped, doubled or misplaced term
shows up as a whole number.

Outputs are slices of sentinel-filled buffers, wider and longer than the result: the spare
columns and rows and both guard bands must be intact after the call. The worst error : bar
ratio of each kernel is printed before it is asserted.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import pair_input_refs as R
from test_gpu_small_kernels import (SENT, _err, _guarded, _guards_intact, _hip,  # noqa: F401
                                    assert_bitwise)

pytestmark = pytest.mark.gpu

V, B0 = R.V_EDGE, R.B_EDGE
DTYPES = [torch.int32, torch.int64]
SHAPES = [pytest.param(F, K, id=f"F{F}-K{K}") for F, K in R.EDGE_SHAPES]
# one shape per staging path and backward kernel: loop / reg, vec / reg, loop / sreg,
# vec / mfma, chunked / lds
PATH_SHAPES = [(3, 5), (12, 8), (22, 10), (32, 32), (65, 4)]


def _dv(a, cuda, dtype=None):
    return torch.tensor(np.asarray(a), device=cuda, dtype=dtype)


@functools.lru_cache(maxsize=None)
def _case(F, K, B, exact):
    """The inputs of a shape with every reference, computed once and never written."""
    c = (R.int_case if exact else R.float_case)(F, K, B, V, seed=1000 * F + 10 * K + B)
    c["cat"], c["cat_scale"] = R.ipnn_cat_ref(c["E"], c["x"])
    c["fe"], c["fe_scale"] = R.fe_ref(c["E"], c["x"])
    c["g"], c["g_scale"] = R.ipnn_bwd_ref(c["E"], c["x"], c["dcat"])
    if not exact:
        c["dots32"] = R.ipnn_dots_f32(c["E"], c["x"])
        c["walk32"] = R.ipnn_walk_f32(c["E"], c["x"], c["dcat"])
    for v in c.values():
        v.setflags(write=False)
    return c


def _ratio(got, ref, scale):
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / (1e-5 * scale + 1e-30)))


def _flag(cuda):
    return torch.zeros(1, dtype=torch.int32, device=cuda)


def _set_mode(monkeypatch, env):
    if env:
        monkeypatch.setenv("CTR_IPNN_BWD", env)
    else:
        monkeypatch.delenv("CTR_IPNN_BWD", raising=False)


def _forward_guarded(cuda, x, E, B, W, **kw):
    """ipnn_forward into a [B + 2, W + 3] slice of a sentinel buffer; returns the [B, W]
    result after checking that nothing else was written."""
    buf, out = _guarded((B + 2, W + 3), cuda)
    ret = _hip().ipnn_forward(x, E, out=out, **kw)
    assert ret is out
    assert _guards_intact(buf, out), "guard bands"
    assert bool((out[B:] == SENT).all()), "rows past B written"
    assert bool((out[:B, W:] == SENT).all()), "columns past W written"
    return out[:B, :W]


def _backward_guarded(cuda, x, E, dcat, B, F, K):
    """ipnn_backward into the first B F rows of a guarded [B F + 2, K] buffer."""
    buf, out = _guarded((B * F + 2, K), cuda)
    ret = _hip().ipnn_backward(x, E, dcat, out=out)
    assert ret is out
    assert _guards_intact(buf, out), "guard bands"
    assert bool((out[B * F:] == SENT).all()), "rows past B F written"
    return out[:B * F]


def _check_forward(cuda, F, K, B, dtype, exact):
    """IPNN (tightly sized and guarded) and Feature_Embedding at one shape; returns the worst
    error : bar ratios (IPNN dots, Feature_Embedding dots)."""
    H = _hip()
    c = _case(F, K, B, exact)
    msg = f"F={F} K={K} B={B} {dtype} {'int' if exact else 'float'}"
    W, P, FK = R.width(F, K), R.n_pairs(F), F * K
    x, E = _dv(c["x"], cuda, dtype), _dv(c["E"], cuda)
    assert E.data_ptr() % 16 == 0
    flat = c["E"][c["x"]].reshape(B, FK)
    err = _flag(cuda)
    tight = H.ipnn_forward(x, E, err_flag=err)
    assert tuple(tight.shape) == (B, W), msg
    wide = _forward_guarded(cuda, x, E, B, W, err_flag=err)
    assert_bitwise(wide, tight, msg + ": guarded against tightly sized")
    got = tight.cpu().numpy()
    assert_bitwise(got[:, :FK], flat, msg + ": flat part")
    fe = H.feature_embedding(x, E, err_flag=err)
    assert tuple(fe.shape) == (B, W), msg
    fe = fe.cpu().numpy()
    assert_bitwise(fe[:, P:], flat, msg + ": Feature_Embedding rows")
    assert int(err.item()) == 0, msg
    if exact:
        np.testing.assert_array_equal(got, c["cat"], err_msg=msg + ": IPNN")
        np.testing.assert_array_equal(fe, c["fe"], err_msg=msg + ": Feature_Embedding")
        return 0.0, 0.0
    r_ip = _ratio(got[:, FK:], c["cat"][:, FK:], c["cat_scale"][:, FK:])
    r_fe = _ratio(fe[:, :P], c["fe"][:, :P], c["fe_scale"][:, :P])
    print(f"\n[pair_inputs] forward {msg} stage={R.stage_path(F, K)} ld={R.fwd_stride(K)} "
          f"lds={R.lds_bytes_fwd(F, K)}/{R.lds_bytes_fe(F, K)}: worst error / bar: "
          f"ipnn_forward {r_ip:.3g}, feature_embedding {r_fe:.3g}")
    assert r_ip <= 1.0 and r_fe <= 1.0, f"{msg}: {r_ip:.3g} / {r_fe:.3g} x the float64 bar"
    assert_bitwise(got[:, FK:], c["dots32"], msg + ": IPNN dots, documented order")
    return r_ip, r_fe


# ================================================================== 1. forward ==========
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,K", SHAPES)
def test_forward_at_every_edge(cuda, F, K, dtype):
    """Float data: flat part bit-exact, IPNN dots bitwise ipnn_dots_f32, Feature_Embedding
    dots inside 1e-5 x L1 of float64 (no order is promised there: its loop may contract).
    Integer data: both exact."""
    _check_forward(cuda, F, K, B0, dtype, exact=False)
    _check_forward(cuda, F, K, B0, dtype, exact=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("F,K", [(3, 5), (12, 8)])
def test_batch_sizes_around_a_block(cuda, F, K, B, dtype, monkeypatch):
    """B either side of the 4 waves of a block (and 9: three blocks, the last with one
    wave): forward and every backward kernel the shape admits, guarded."""
    _check_forward(cuda, F, K, B, dtype, exact=False)
    _check_forward(cuda, F, K, B, dtype, exact=True)
    for exact in (False, True):
        c = _case(F, K, B, exact)
        x, E, dcat = _dv(c["x"], cuda, dtype), _dv(c["E"], cuda), _dv(c["dcat"], cuda)
        for env, kern in R.bwd_modes(F, K):
            _set_mode(monkeypatch, env)
            got = _backward_guarded(cuda, x, E, dcat, B, F, K)
            assert kern != "mfma"
            assert_bitwise(got, c["g"].astype(np.float32) if exact else c["walk32"],
                           f"F={F} K={K} B={B} {env or 'default'}")


# =================================================================== 2. planes ==========
def _bf16_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def _check_planes(pl, want, B, W, msg):
    assert pl.t.shape == want.t.shape, msg
    np.testing.assert_array_equal(_bf16_bits(pl.t), _bf16_bits(want.t), err_msg=msg)
    assert bool((pl.t[0, :B, W] == 1).all()) and not bool(pl.t[1:, :, W].any()), msg + ": ones"
    assert not bool(pl.t[:, B:].any()) and not bool(pl.t[:, :, W + 1:].any()), msg + ": padding"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,K", SHAPES)
def test_planes_at_every_edge(cuda, F, K, dtype):
    """planes= (with and without the fp32 out) and feature_embedding(out_planes=) are bitwise
    split_planes of the fp32 result, in a Planes with the trainer's ones column; the ones
    column and the zero padding stay as they were."""
    H = _hip()
    c = _case(F, K, B0, False)
    B, W = B0, R.width(F, K)
    x, E = _dv(c["x"], cuda, dtype), _dv(c["E"], cuda)
    new = lambda: H.Planes(B, W, cuda, ones_col=True)  # noqa: E731
    cat = H.ipnn_forward(x, E)
    want = H.split_planes(cat, new())
    assert_bitwise(want.to_float(), cat, "the split is exact")
    for keep in (False, True):
        msg = f"F={F} K={K} {dtype} planes, out={keep}"
        pl = new()
        if keep:
            assert_bitwise(_forward_guarded(cuda, x, E, B, W, planes=pl), cat, msg)
        else:
            assert H.ipnn_forward(x, E, out=None, planes=pl) is None
        _check_planes(pl, want, B, W, msg)
    fe = H.feature_embedding(x, E)
    want = H.split_planes(fe, new())
    pl = new()
    assert_bitwise(H.feature_embedding(x, E, out_planes=pl), fe, "out beside the planes")
    _check_planes(pl, want, B, W, f"F={F} K={K} {dtype} feature_embedding planes")


# ================================================================= 3. backward ==========
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,K", SHAPES)
def test_backward_at_every_edge(cuda, F, K, dtype, monkeypatch):
    """The default and every CTR_IPNN_BWD value the shape admits, dcat 3 columns wider than
    W. lds / reg / sreg: bitwise ipnn_walk_f32 (so bitwise one another). The matrix-core
    product: inside 1e-5 x the per-element L1 scale of float64, the same bits on a second
    launch. Integer data: every kernel exact."""
    B = B0
    worst = {}
    for exact in (False, True):
        c = _case(F, K, B, exact)
        x, E, dcat = _dv(c["x"], cuda, dtype), _dv(c["E"], cuda), _dv(c["dcat"], cuda)
        assert dcat.stride(0) == R.width(F, K) + 3
        for env, kern in R.bwd_modes(F, K):
            msg = f"F={F} K={K} {dtype} CTR_IPNN_BWD={env or '(unset)'} -> {kern}"
            _set_mode(monkeypatch, env)
            got = _backward_guarded(cuda, x, E, dcat, B, F, K).cpu().numpy()
            if exact:
                np.testing.assert_array_equal(got, c["g"], err_msg=msg + ": integer data")
                continue
            r = _ratio(got, c["g"], c["g_scale"])
            worst[kern] = max(worst.get(kern, 0.0), r)
            print(f"\n[pair_inputs] backward {msg} lds={R.lds_bytes_bwd(F, K, kern)}: "
                  f"worst error / bar: {kern} {r:.3g}")
            assert r <= 1.0, f"{msg}: {r:.3g} x the float64 bar"
            if kern == "mfma":
                assert_bitwise(_backward_guarded(cuda, x, E, dcat, B, F, K), got,
                               msg + ": second launch")
            else:
                assert_bitwise(got, c["walk32"], msg + ": documented order")
    assert set(worst) == {k for _, k in R.bwd_modes(F, K)}


# ====================================================================== 4. ids ==========
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,K", PATH_SHAPES)
def test_bad_ids_flag_and_read_row_0(cuda, F, K, dtype, monkeypatch):
    """-1 in the first field, V in a middle one and V + 77 in the last (of three examples;
    example 0 repeats an id): the forwards raise the index flag, fault nothing and read row
    0 — every output is bitwise that of the batch with those ids replaced by 0, whose flat
    part is the rows of the table; the backward (it takes no flag) likewise."""
    H = _hip()
    B, W = B0, R.width(F, K)
    c = _case(F, K, B, False)
    good = np.maximum(c["x"], 1)  # row 0 is not what the good ids read
    good[0, 0] = good[0, F - 1]
    bad = good.copy()
    for (b, f), v in (((1, 0), -1), ((2, F // 2), V), ((4, F - 1), V + 77)):
        good[b, f], bad[b, f] = 0, v
    E, dcat = _dv(c["E"], cuda), _dv(c["dcat"], cuda)
    xg, xb = _dv(good, cuda, dtype), _dv(bad, cuda, dtype)
    for name, fn in (("ipnn_forward", lambda x, e: _forward_guarded(cuda, x, E, B, W, err_flag=e)),
                     ("feature_embedding", lambda x, e: H.feature_embedding(x, E, err_flag=e))):
        e_bad, e_good = _flag(cuda), _flag(cuda)
        rb, rg = fn(xb, e_bad), fn(xg, e_good)
        assert int(e_bad.item()) & 1 and int(e_good.item()) == 0, name
        with pytest.raises(IndexError):
            H.check_index_error(e_bad)
        assert_bitwise(rb, rg, f"F={F} K={K} {dtype} {name}")
        flat = rg[:, :F * K] if name == "ipnn_forward" else rg[:, R.n_pairs(F):]
        assert_bitwise(flat, c["E"][good].reshape(B, F * K), name + ": rows of the table")
    pl_b, pl_g = (H.Planes(B, W, cuda, ones_col=True) for _ in range(2))
    e_bad = _flag(cuda)
    H.ipnn_forward(xb, E, out=None, err_flag=e_bad, planes=pl_b)
    H.ipnn_forward(xg, E, out=None, planes=pl_g)
    assert int(e_bad.item()) & 1
    np.testing.assert_array_equal(_bf16_bits(pl_b.t), _bf16_bits(pl_g.t))
    want = R.ipnn_walk_f32(c["E"], good, c["dcat"])
    for env, kern in R.bwd_modes(F, K):
        _set_mode(monkeypatch, env)
        gb = _backward_guarded(cuda, xb, E, dcat, B, F, K)
        gg = _backward_guarded(cuda, xg, E, dcat, B, F, K)
        assert_bitwise(gb, gg, f"F={F} K={K} {dtype} backward {kern}")
        if kern != "mfma":
            assert_bitwise(gg, want, f"F={F} K={K} {dtype} backward {kern}: row-0 result")


# ================================================================ 5. alignment ==========
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,K", [(2, 4), (12, 8), (26, 16), (32, 64), (64, 32)])
def test_table_one_float_past_alignment(cuda, F, K, dtype, monkeypatch):
    """A table that starts one float past a 16-byte boundary (a contiguous view hip_ops
    accepts): stage_rows_wave leaves its float4 path, and every kernel gives the bits it
    gives with the aligned table."""
    H = _hip()
    B, W = B0, R.width(F, K)
    assert R.stage_path(F, K) == "vec" and R.stage_path(F, K, aligned=False) == "loop"
    c = _case(F, K, B, False)
    x, E, dcat = _dv(c["x"], cuda, dtype), _dv(c["E"], cuda), _dv(c["dcat"], cuda)
    ebuf, Em = _guarded((V, K), cuda, shift=1)
    Em.copy_(E)
    assert E.data_ptr() % 16 == 0 and Em.data_ptr() % 16 == 4 and Em.is_contiguous()
    msg = f"F={F} K={K} {dtype}"
    got = _forward_guarded(cuda, x, Em, B, W)
    assert_bitwise(got, H.ipnn_forward(x, E), msg + ": ipnn_forward")
    assert_bitwise(got[:, F * K:], c["dots32"], msg + ": dots, documented order")
    assert_bitwise(H.feature_embedding(x, Em), H.feature_embedding(x, E), msg + ": state")
    pl_m, pl_a = (H.Planes(B, W, cuda, ones_col=True) for _ in range(2))
    H.ipnn_forward(x, Em, out=None, planes=pl_m)
    H.ipnn_forward(x, E, out=None, planes=pl_a)
    np.testing.assert_array_equal(_bf16_bits(pl_m.t), _bf16_bits(pl_a.t), err_msg=msg)
    for env, kern in R.bwd_modes(F, K):
        _set_mode(monkeypatch, env)
        gm = _backward_guarded(cuda, x, Em, dcat, B, F, K)
        assert_bitwise(gm, _backward_guarded(cuda, x, E, dcat, B, F, K), f"{msg} {kern}")
    assert _guards_intact(ebuf, Em)


# ================================================================= 6. refusals ==========
def test_refusals_write_nothing(cuda):
    """F = 1, K = 0, a shape past the LDS limit and a bad `out` each raise before any launch:
    every guarded buffer is still all sentinel."""
    H, Err = _hip(), _err()
    B = 3
    bufs = []

    def guarded(shape, dtype=torch.float32):
        bufs.append(_guarded(shape, cuda, dtype))
        return bufs[-1][1]

    def inputs(F, K):
        c = R.int_case(F, K, B, V, seed=F + K)
        return _dv(c["x"], cuda), _dv(c["E"], cuda), _dv(c["dcat"], cuda)

    for F, K in ((1, 8), (5, 0)):
        x, E, dcat = inputs(F, K)
        W = R.width(F, K)
        with pytest.raises(Err):
            H.ipnn_forward(x, E, out=guarded((B, W + 4)))
        with pytest.raises(Err):
            H.ipnn_forward(x, E, out=guarded((B, W + 4)),
                           planes=H.Planes(B, W + 4, cuda, ones_col=True))
        with pytest.raises(Err):
            H.feature_embedding(x, E)
        with pytest.raises(Err):
            H.ipnn_backward(x, E, dcat, out=guarded((B * F + 1, K + 1)))
    for (F, K), what in ((R.REFUSED_FWD, "fwd"), (R.REFUSED_BWD, "bwd"), (R.REFUSED_FE, "fe")):
        x, E, dcat = inputs(F, K)
        with pytest.raises(Err, match="LDS"):
            if what == "fwd":
                H.ipnn_forward(x, E, out=guarded((B, R.width(F, K))))
            elif what == "bwd":
                H.ipnn_backward(x, E, dcat, out=guarded((B * F, K)))
            else:
                H.feature_embedding(x, E)
    # a bad `out`, at a shape that would otherwise run
    F, K = 12, 8
    x, E, dcat = inputs(F, K)
    W = R.width(F, K)
    with pytest.raises(ValueError):
        H.ipnn_forward(x, E, out=guarded((B, W), torch.float64))
    with pytest.raises(ValueError):
        H.ipnn_forward(x, E, out=guarded((B, W - 1)))
    with pytest.raises(ValueError):
        H.ipnn_forward(x, E, out=guarded((B - 1, W)))
    with pytest.raises(ValueError):
        H.ipnn_forward(x, E, out=guarded((B, 2 * W))[:, ::2])
    with pytest.raises(TypeError):
        H.ipnn_backward(x, E, dcat, out=guarded((B * F, K), torch.float64))
    with pytest.raises(ValueError):
        H.ipnn_backward(x, E, dcat, out=guarded((B * F, K))[:-1])
    with pytest.raises(ValueError):
        H.ipnn_backward(x, E, dcat, out=guarded((B * F, 2 * K))[:, :K])
    with pytest.raises(TypeError):
        H.ipnn_backward(x, E, dcat, out=torch.empty(B * F, K))
    with pytest.raises(ValueError):
        H.ipnn_backward(x, E, dcat[:, :W - 1].contiguous(), out=guarded((B * F, K)))
    torch.cuda.synchronize()
    for buf, _ in bufs:
        assert bool((buf == SENT).all())
    # and the same arguments with a good `out` run
    np.testing.assert_array_equal(
        H.ipnn_backward(x, E, dcat, out=guarded((B * F, K))).cpu().numpy(),
        R.ipnn_bwd_ref(E.cpu().numpy(), x.cpu().numpy(), dcat.cpu().numpy())[0])
