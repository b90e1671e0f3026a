"""CPU checks of tests/pair_input_refs.py, so that tests/test_gpu_pair_inputs.py compares the
pair-input kernels with references that something else has checked: the float64 references
against the oracle's torch ops and autograd, the fp32 emulations of the documented order
against float64 (inside the 1e-5 x L1 bar, with room to spare), the integer inputs' exactness
in fp32, the dispatch mirror written out by hand, and that EDGE_SHAPES takes every label of
every predicate — the GPU test can then never lose an edge silently."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import pair_input_refs as R
from oracle import ctr_oracle as O

REF_SHAPES = [(2, 1), (5, 3), (12, 8), (33, 64)]


@pytest.mark.parametrize("F,K", REF_SHAPES)
def test_float64_refs_vs_oracle_and_autograd(F, K):
    c = R.float_case(F, K, 7, 50, seed=F * K)
    E, x = torch.tensor(c["E"]).double(), torch.tensor(c["x"])
    W = R.width(F, K)
    cat, scale = R.ipnn_cat_ref(c["E"], c["x"])
    np.testing.assert_allclose(cat, O.ipnn_cat(E, x).numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(scale, O.ipnn_cat(E.abs(), x).numpy(), rtol=1e-13, atol=1e-13)
    fe, fscale = R.fe_ref(c["E"], c["x"])
    np.testing.assert_allclose(fe, O.feature_embedding(E, x).numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(fscale, O.feature_embedding(E.abs(), x).numpy(), rtol=1e-13,
                               atol=1e-13)
    # the backward: autograd through the oracle's forward, the wider dcat's first W columns
    d = torch.tensor(c["dcat"]).double()
    assert d.shape[1] == W + 3
    e = torch.nn.functional.embedding(x, E).requires_grad_(True)
    row, col = O.ipnn_pairs(F)
    torch.cat([e.reshape(7, -1), (e[:, row] * e[:, col]).sum(2)], 1).backward(d[:, :W])
    g, gs = R.ipnn_bwd_ref(c["E"], c["x"], c["dcat"])
    np.testing.assert_allclose(g, e.grad.reshape(7 * F, K).numpy(), rtol=1e-13, atol=1e-13)
    # its scale, the slow way (the loop of test_ipnn_forward_and_backward_vs_oracle)
    ea, pa = e.detach().abs(), d.abs()[:, F * K:W]
    bound = d.abs()[:, :F * K].reshape(7, F, K).clone()
    for p, (i, j) in enumerate(zip(row.tolist(), col.tolist())):
        bound[:, i] += pa[:, p:p + 1] * ea[:, j]
        bound[:, j] += pa[:, p:p + 1] * ea[:, i]
    np.testing.assert_allclose(gs, bound.reshape(7 * F, K).numpy(), rtol=1e-13, atol=1e-13)


def test_fp32_emulations_sit_inside_the_bar():
    """The documented order in fp32 against float64: far inside 1e-5 x the L1 scale (a
    K-term fp32 sum errs by about 2^-24 sqrt(K) of it), and equal to the plain sequential
    loops written out element by element."""
    worst_d = worst_w = 0.0
    for F, K in REF_SHAPES:
        c = R.float_case(F, K, 7, 50, seed=F + K)
        cat, scale = R.ipnn_cat_ref(c["E"], c["x"])
        dots = R.ipnn_dots_f32(c["E"], c["x"])
        worst_d = max(worst_d, float(np.max(np.abs(dots - cat[:, F * K:])
                                            / (1e-5 * scale[:, F * K:]))))
        g, gs = R.ipnn_bwd_ref(c["E"], c["x"], c["dcat"])
        walk = R.ipnn_walk_f32(c["E"], c["x"], c["dcat"])
        worst_w = max(worst_w, float(np.max(np.abs(walk - g) / (1e-5 * gs))))
        # element by element, example 0 and the last one
        e = c["E"][c["x"]]
        i, j = np.triu_indices(F, k=1)
        for b in (0, 6):
            for p in range(len(i)):
                acc = np.float32(0)
                for k in range(K):
                    acc = np.float32(acc + np.float32(e[b, i[p], k] * e[b, j[p], k]))
                assert acc == dots[b, p], (F, K, b, p)
            D = R.pair_matrix(c["dcat"], F, K)[b]
            for f in (0, F // 2, F - 1):
                for k in (0, K - 1):
                    gv = c["dcat"][b, f * K + k]
                    for jj in range(F):
                        if jj != f:
                            gv = np.float32(gv + np.float32(D[f, jj] * e[b, jj, k]))
                    assert gv == walk[b * F + f, k], (F, K, b, f, k)
    print(f"\n[pair_inputs] fp32 emulation, worst error / (1e-5 x L1): dots {worst_d:.3g}, "
          f"walk {worst_w:.3g}")
    assert worst_d <= 0.1 and worst_w <= 0.1


def test_int_case_is_exact_in_fp32():
    """The L1 norm of every sum of every edge shape stays below 2^24 (so any order is exact),
    and the fp32 emulations return the integer results."""
    for F, K in R.EDGE_SHAPES + (R.REFUSED_FWD, R.REFUSED_BWD):
        c = R.int_case(F, K, R.B_EDGE, R.V_EDGE, seed=F * 131 + K)
        for a in (c["E"], c["dcat"]):
            assert a.dtype == np.float32 and np.array_equal(a, np.rint(a))
            assert np.abs(a).max() <= 8
        cat, scale = R.ipnn_cat_ref(c["E"], c["x"])
        g, gs = R.ipnn_bwd_ref(c["E"], c["x"], c["dcat"])
        assert max(scale.max(), gs.max()) < 2 ** 24, (F, K)
        assert np.array_equal(cat, np.rint(cat)) and np.array_equal(g, np.rint(g))
        if F * K <= 2048:
            assert np.array_equal(R.ipnn_dots_f32(c["E"], c["x"]), cat[:, F * K:]), (F, K)
            assert np.array_equal(R.ipnn_walk_f32(c["E"], c["x"], c["dcat"]), g), (F, K)


def test_cases_hold_what_they_promise():
    for F, K in R.EDGE_SHAPES:
        c = R.float_case(F, K, R.B_EDGE, R.V_EDGE, seed=1)
        x = c["x"]
        assert x.min() >= 0 and x.max() < R.V_EDGE
        assert x[0, 0] == x[0, F - 1]  # a repeated id inside an example
        assert x[R.B_EDGE - 1, F // 2] == x[0, F // 2]  # a row two examples use
        assert c["dcat"].shape == (R.B_EDGE, R.width(F, K) + 3)


def test_dispatch_mirror_by_hand():
    """The predicates at shapes read off the launchers by hand (csrc/ctr_common.h
    stage_rows_wave, csrc/pnn.hip launch_ipnn_backward_reg and the LDS sizes)."""
    assert [R.stage_path(*s) for s in ((32, 64), (64, 32), (33, 64), (64, 5), (65, 4), (2, 1))] \
        == ["vec", "vec", "loop", "loop", "chunked", "loop"]
    assert R.stage_path(12, 8, aligned=False) == "loop"
    assert [R.last_chunk(F) for F in (2, 64, 65, 128, 129)] == [2, 64, 1, 64, 1]
    assert [R.fwd_stride(K) for K in (1, 4, 5, 63, 64)] == [2, 8, 6, 64, 68]
    want = {(2, 32): "mfma", (32, 128): "mfma", (31, 32): "mfma", (5, 96): "mfma",
            (26, 16): "sreg", (22, 63): "sreg", (26, 1): "sreg",
            (32, 33): "reg", (32, 63): "reg", (2, 1): "reg", (12, 8): "reg",
            (33, 8): "lds", (33, 64): "lds", (5, 65): "lds", (7, 68): "lds", (39, 128): "lds",
            (26, 65): "lds", (64, 32): "lds", (129, 4): "lds"}
    for s, k in want.items():
        assert R.bwd_kernel(*s) == k, s
    assert R.bwd_modes(26, 64) == [("", "mfma"), ("m", "mfma"), ("sreg", "sreg"),
                                   ("reg", "reg"), ("lds", "lds")]
    assert R.bwd_modes(22, 128) == [("", "mfma"), ("m", "mfma"), ("lds", "lds")]
    assert R.bwd_modes(33, 8) == [("", "lds"), ("lds", "lds")]
    assert R.bwd_modes(12, 8) == [("", "reg"), ("reg", "reg"), ("lds", "lds")]
    assert (R.lds_bytes_fwd(31, 128), R.lds_bytes_fwd(32, 128)) == (65472, 67584)
    assert (R.lds_bytes_bwd(64, 32), R.lds_bytes_bwd(39, 128)) == (66048, 92352)
    assert R.lds_bytes_bwd(129, 4) == 142416 and R.lds_bytes_fwd(22, 128) == 46464
    assert R.lds_bytes_fe(39, 128) == 80496 and R.lds_bytes_fwd(39, 128) == 82368
    assert R.lds_bytes_bwd(32, 64, "reg") == 7936 and R.lds_bytes_bwd(32, 64, "mfma") == 0
    assert R.lds_bytes_bwd(26, 64, "sreg") == 0
    assert [R.lds_class(n) for n in (65536, 65537, 163840, 163841)] == \
        ["plain", "asked", "asked", "refused"]
    assert R.lds_class(R.lds_bytes_fwd(*R.REFUSED_FWD)) == "refused"
    assert R.lds_class(R.lds_bytes_bwd(*R.REFUSED_BWD)) == "refused"
    assert R.lds_class(R.lds_bytes_fe(*R.REFUSED_FE)) == "refused"
    assert R.bwd_kernel(*R.REFUSED_BWD) == "lds"


def test_edge_shapes_take_every_label():
    """Every label of every predicate is taken by an EDGE_SHAPES entry (the GPU test runs
    them all at B_EDGE examples, tightly sized and with 3 spare columns)."""
    S, B = R.EDGE_SHAPES, R.B_EDGE
    assert len(S) == len(set(S)) == 28 and all(len(v) for v in R.EDGES.values())
    assert {R.stage_path(*s) for s in S} == {"vec", "loop", "chunked"}
    # the fast path's limit from both sides, F = 64 on both paths, a short last chunk after
    # one and after two whole ones
    vec = [s for s in S if R.stage_path(*s) == "vec"]
    assert max(F * K for F, K in vec) == 2048 and max(F for F, K in vec) == 64
    assert any(F * K > 2048 and F <= 64 and K % 4 == 0 for F, K in S)
    assert any(F == 64 and R.stage_path(F, K) == "loop" for F, K in S)
    assert {(F - 1) // 64 for F, K in S if R.stage_path(F, K) == "chunked"} == {1, 2}
    assert {R.last_chunk(F) for F, K in S if R.stage_path(F, K) == "chunked"} == {1}
    # the flat store of the fast path, aligned and not, for IPNN (b x ldc) and
    # Feature_Embedding (b x W + P)
    for ldx in (0, 3):
        ip = {R.flat_aligned(b * (R.width(*s) + ldx)) for s in vec for b in range(B)}
        assert ip == {True, False}, ldx
    fe = {R.flat_aligned(b * R.width(*s) + R.n_pairs(s[0])) for s in vec for b in range(B)}
    assert fe == {True, False}
    # both row strides on each staging path that can have them
    assert {(R.stage_path(*s), s[1] % 4 == 0) for s in S} == \
        {("vec", True), ("loop", True), ("loop", False), ("chunked", True)}
    # pairs: fewer than a wave, one short of / just past a wave, several trips
    P = {R.n_pairs(F) for F, K in S}
    assert {1, 3, 55, 66} <= P and max(P) > 64 * 64
    # the four backward kernels, each forced and by default, at their edges
    kern = {k for s in S for _, k in R.bwd_modes(*s)}
    assert kern == {"mfma", "sreg", "reg", "lds"}
    assert {R.bwd_kernel(*s) for s in S} == kern
    mf = [s for s in S if R.bwd_kernel(*s) == "mfma"]
    assert {K // 32 for F, K in mf} == {1, 2, 3, 4} and {2, 5, 31, 32} <= {F for F, K in mf}
    assert {(F, K) for F, K in S if R.bwd_kernel(F, K) == "sreg"} == \
        {(22, 10), (22, 63), (26, 1), (26, 16)}
    rg = [s for s in S if R.bwd_kernel(*s) == "reg"]
    assert (32, 33) in rg and (32, 63) in rg and (2, 1) in rg
    ld = [s for s in S if R.bwd_kernel(*s) == "lds"]
    assert any(F > 32 and K <= 64 for F, K in ld) and any(F <= 32 and K > 64 for F, K in ld)
    # dynamic LDS: under and past 64 KB for each kernel that has a tile, the forward at the
    # last size under it; nothing in EDGE_SHAPES is refused
    for fn in (R.lds_bytes_fe, R.lds_bytes_fwd, R.lds_bytes_bwd):
        assert {R.lds_class(fn(*s)) for s in S} == {"plain", "asked"}, fn.__name__
    assert max(R.lds_bytes_fwd(*s) for s in S if R.lds_class(R.lds_bytes_fwd(*s)) == "plain") \
        == 65472
    asked = {s for s in S if "asked" in (R.lds_class(R.lds_bytes_fwd(*s)),
                                         R.lds_class(R.lds_bytes_bwd(*s)),
                                         R.lds_class(R.lds_bytes_fe(*s)))}
    assert asked >= {(32, 128), (64, 32), (39, 128), (129, 4)}
