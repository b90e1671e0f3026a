"""CPU checks of tests/fm_path_refs.py, so that tests/test_gpu_fm_path.py compares the FM
forward and the segmented row sums with references and layouts that something else has
checked: the dispatch table, that every lettered layout case is present for every (C, G, T)
the K list produces (the GPU test can then never miss an edge silently), that the keys give
the intended plan, the fp32 emulation against float64 and against plain sequential sums, the
FM forward references against the oracle, and that the integer inputs stay exact in fp32."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import fm_path_refs as R
from conftest import grad_bound
from oracle import ctr_oracle as O

CLASSES = sorted(R.seg_classes())


def test_seg_class_table():
    """(vec, KV, LPR, C, G, T) for every K of the GPU tests, written out by hand from
    launch_seg (vec, KV, LPR), seg_chunk (C) and seg_combine_apply_kernel (G, T)."""
    want = {
        (1, True): (False, 1, 1, 4, 64, 16),
        (3, True): (False, 3, 4, 4, 16, 16),
        (4, True): (True, 1, 1, 4, 64, 16),
        (8, True): (True, 2, 2, 4, 32, 16),
        (10, True): (False, 10, 16, 16, 4, 8),
        (12, True): (True, 3, 4, 4, 16, 16),
        (16, True): (True, 4, 4, 4, 16, 16),
        (17, True): (False, 17, 32, 16, 2, 8),
        (32, True): (True, 8, 8, 4, 8, 8),
        (33, True): (False, 33, 64, 16, 1, 8),
        (64, True): (True, 16, 16, 16, 4, 8),
        (128, True): (True, 32, 32, 16, 2, 8),
        (256, True): (True, 64, 64, 16, 1, 8),
        (16, False): (False, 16, 16, 16, 4, 8),
        (64, False): (False, 64, 64, 16, 1, 8),
        (65, True): None, (260, True): None, (128, False): None,
    }
    assert {k for k, v in want.items() if v is not None} == \
        {(K, True) for K in R.SEG_K} | {(K, False) for K in R.SEG_K_MISALIGNED}
    assert {k for k, v in want.items() if v is None} == set(R.SEG_UNSUPPORTED)
    for (K, al), w in want.items():
        assert R.seg_class(K, al) == w, (K, al)
    assert set(CLASSES) == {(4, 64, 16), (4, 32, 16), (4, 16, 16), (4, 8, 8), (16, 4, 8),
                            (16, 2, 8), (16, 1, 8)}


@pytest.mark.parametrize("C,G,T", CLASSES)
def test_edge_runs_hold_every_case(C, G, T):
    runs = R.edge_runs(C, G, T)
    off0, off1, P = R.row_pieces(runs, C)
    # row_pieces itself, the slow way: the chunks each position of a run falls in
    pos = 0
    for u, n in enumerate(runs):
        chunks = {p // C for p in range(pos, pos + n)}
        assert (off0[u], off1[u], P[u]) == (pos, pos + n, len(chunks)), u
        pos += n
    got = R.layout_cases(runs, C, G, T)
    for case in "abcdeghi":
        assert got[case], f"case {case} missing for C={C} G={G} T={T}"
    for p in R.edge_P(G, T):
        assert (p, True) in got["f"] and (p, False) in got["f"], (p, C, G, T)
    assert {2, 3, T, T + 1, 2 * T + 3} <= set(R.edge_P(G, T))
    if G > 2:
        assert {G - 1, G, G + 1} <= set(R.edge_P(G, T))
    # all three routes of the fused apply: 1 piece, 2..T pieces, more than T
    assert (P == 1).any() and ((P >= 2) & (P <= T)).any() and (P > T).any()
    assert sum(runs) <= 4096 and int(P.max()) * C <= 560 + C


@pytest.mark.parametrize("C,G,T", CLASSES)
def test_edge_cases_are_not_vacuous(C, G, T):
    """layout_cases says no where a case is absent: plain layouts have none of c, d, g."""
    flat = R.layout_cases([C] * (2 * G), C, G, T)
    assert flat["a"] and not (flat["b"] or flat["c"] or flat["d"] or flat["e"] or flat["i"])
    assert flat["g"] == (G == 1) and flat["h"] == (G == 1)
    ones = R.layout_cases([1] * (C + 1), C, G, T)
    assert not (ones["a"] or ones["b"] or ones["c"] or ones["d"] or ones["i"]) and ones["e"]
    assert ones["f"] == set()


@pytest.mark.parametrize("C,G,T", CLASSES)
def test_tiny_and_long_layouts(C, G, T):
    assert R.tiny_layouts(C) == [[1], [C - 1], [C + 1]]
    runs = R.long_runs(C, G, T)
    off0, off1, P = R.row_pieces(runs, C)
    assert len(runs) > 8192 and off1[-1] > 8192
    late = P[8192:]
    assert ((late >= 2) & (late <= T)).any() and (late > T).any()
    assert off1[-1] <= 8192 + 8192 // 97 + 40 * C  # K = 256: 8 MB of values


@pytest.mark.parametrize("C,G,T", CLASSES)
def test_keys_give_the_layout(C, G, T):
    for runs in [R.edge_runs(C, G, T)] + R.tiny_layouts(C):
        keys, V = R.keys_from_runs(runs, seed=C + G)
        order, rows, off = R.plan_of(keys)
        np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(runs)]))
        assert rows.size == len(runs) and (rows != np.arange(rows.size)).all()
        assert (np.diff(rows) >= 1).all() and (np.diff(rows) > 1).any() or rows.size == 1
        assert 0 <= keys.min() and keys.max() < V
        if rows.size > 1:  # one row's slots are in slot order whatever the permutation
            assert (order != np.arange(keys.size)).any()
        # the stable sort: slots ascend inside every run
        for u in range(rows.size):
            seg = order[off[u]:off[u + 1]]
            assert (keys[seg] == rows[u]).all() and (np.diff(seg) > 0).all()


def _chunked_then_sequential(keys, vals, C):
    """Every row's chunk sums (sequential, from zero) added sequentially in chunk order."""
    order, rows, off = R.plan_of(keys)
    v = np.asarray(vals, np.float32)[order]
    out = np.zeros((rows.size, v.shape[1]), np.float32)
    for u in range(rows.size):
        for ch in range(off[u] // C, (off[u + 1] - 1) // C + 1):
            piece = np.zeros(v.shape[1], np.float32)
            for pos in range(max(off[u], ch * C), min(off[u + 1], (ch + 1) * C)):
                piece = piece + v[pos]
            out[u] = out[u] + piece
    return out


@pytest.mark.parametrize("C,G,T", CLASSES)
def test_f32_tree_vals_mode(C, G, T):
    """Random data: inside the float64 bar; a row inside one chunk is the plain sequential
    fp32 sum of its slots; with one accumulator (G = 1) a spanning row is the plain sequential
    fp32 sum of its chunk sums; integers: every order gives the same, exact, sums."""
    runs = R.edge_runs(C, G, T)
    keys, V = R.keys_from_runs(runs, seed=7)
    K, F = 5, 3
    x = R.float_seg_inputs(keys.size, K, F, V, seed=11)
    ref = R.seg_sums_f64(keys, vals=x["vals"], vals_lin=x["vals_lin"])
    got, gl = R.seg_sums_f32_tree(keys, C, G, vals=x["vals"], vals_lin=x["vals_lin"])
    assert got.dtype == np.float32 and gl.dtype == np.float32
    assert (np.abs(got - ref["sums"]) <= grad_bound(ref["sums"], cond=ref["cond"])).all()
    assert (np.abs(gl - ref["lin"]) <= grad_bound(ref["lin"], cond=ref["cond_lin"])).all()
    np.testing.assert_array_equal(ref["counts"], runs)
    _, _, P = R.row_pieces(runs, C)
    seq = R.seq_sums_f32(keys, x["vals"])
    np.testing.assert_array_equal(got[P == 1], seq[P == 1])
    if G == 1:
        np.testing.assert_array_equal(got, _chunked_then_sequential(keys, x["vals"], C))
    else:
        assert (got[P > 1] != seq[P > 1]).any()  # the tree is a different order
    xi = R.int_seg_inputs(keys.size, K, F, V, seed=13)
    ri = R.seg_sums_f64(keys, vals=xi["vals"])
    gi, none = R.seg_sums_f32_tree(keys, C, G, vals=xi["vals"])
    assert none is None and ri["lin"] is None
    np.testing.assert_array_equal(gi, ri["sums"])
    np.testing.assert_array_equal(R.seq_sums_f32(keys, xi["vals"]), ri["sums"])


@pytest.mark.parametrize("C,G,T", CLASSES)
@pytest.mark.parametrize("with_dx", [False, True])
def test_f32_tree_fm_mode(C, G, T, with_dx):
    runs = R.edge_runs(C, G, T)
    keys, V = R.keys_from_runs(runs, seed=8)
    K, F = 4, 3
    for make, exact in ((R.float_seg_inputs, False), (R.int_seg_inputs, True)):
        x = make(keys.size, K, F, V, seed=17)
        kw = dict(F=F, gz=x["gz"], sum_e=x["sum_e"], emb=x["emb"], dx=x["dx"] if with_dx else None)
        ref = R.seg_sums_f64(keys, **kw)
        got, gl = R.seg_sums_f32_tree(keys, C, G, **kw)
        if exact:
            np.testing.assert_array_equal(got, ref["sums"])
            np.testing.assert_array_equal(gl, ref["lin"])
        else:
            assert (np.abs(got - ref["sums"]) <= grad_bound(ref["sums"], cond=ref["cond"])).all()
            assert (np.abs(gl - ref["lin"]) <= grad_bound(ref["lin"], cond=ref["cond_lin"])).all()
    # the float64 sums, the slow way, for one row
    u = int(np.argmax(runs))
    slots = np.flatnonzero(keys == ref["rows"][u])
    want = sum(float(x["gz"][s // F]) * (x["sum_e"][s // F].astype(np.float64) -
                                         x["emb"][ref["rows"][u]]) +
               (x["dx"][s] if with_dx else 0.0) for s in slots)
    np.testing.assert_allclose(ref["sums"][u], want, rtol=1e-12, atol=1e-12)


def test_integer_inputs_stay_exact():
    """The L1 norm of every sum is below 2^23, so fp32 holds every partial sum of any order
    exactly: the segmented sums over every layout used on the GPU (the worst row is 2T + 3
    pieces of 16 = 560 slots of at most |g s| + |g e| + |d| = 16 + 8 + 4), and the FM forward
    at its largest shape (K = 260, F = 65: at most 260 x (130^2 + 65 x 4) = 4 461 600)."""
    lim = 2 ** 23
    K, F = 4, 3
    for (C, G, T) in CLASSES:
        for runs in (R.edge_runs(C, G, T), R.long_runs(C, G, T)):
            keys, V = R.keys_from_runs(runs, seed=1)
            x = R.int_seg_inputs(keys.size, K, F, V, seed=2)
            for kw in (dict(vals=x["vals"], vals_lin=x["vals_lin"]),
                       dict(F=F, gz=x["gz"], sum_e=x["sum_e"], emb=x["emb"], dx=x["dx"])):
                r = R.seg_sums_f64(keys, **kw)
                assert r["cond"].max() < lim and r["cond_lin"].max() < lim
            assert max(runs) * 28 < lim and max(runs) * 2 * 4 < lim  # any draw of the ranges
    assert 260 * (130 ** 2 + 65 * 4) + 65 * 4 + 4 < lim
    for (K, F, B) in ((260, 65, 5), (256, 64, 5), (130, 65, 67)):
        x = R.int_fm_inputs(B, F, K, 37, seed=K + F)
        assert R.fm_forward_int(x["x"], x["E"], x["w"], x["b"])["l1"].max() < lim
    # the ranges themselves
    x = R.int_seg_inputs(4000, 4, 3, 50, seed=3)
    for k, hi in (("vals", 4), ("vals_lin", 4), ("dx", 4), ("emb", 4), ("sum_e", 8), ("gz", 2)):
        assert x[k].dtype == np.float32 and x[k].min() == -hi and x[k].max() == hi
        assert (x[k] == np.round(x[k])).all()
    x = R.int_fm_inputs(50, 20, 16, 37, seed=4)
    assert x["E"].min() == -2 and x["E"].max() == 2 and np.abs(x["w"]).max() == 4


@pytest.mark.parametrize("K,F,B", [(4, 1, 1), (10, 8, 5), (16, 33, 4), (65, 65, 3)])
def test_fm_forward_refs(K, F, B):
    """fm_forward_f64 against the oracle's FM (torch, in float64) and torch's sigmoid + BCE and
    their autograd; fm_forward_int equal to it on integer tables."""
    V = 37
    x = R.float_fm_inputs(B, F, K, V, seed=K + F)
    params = {"feature_embedding.weight": torch.tensor(x["E"]).double(),
              "linear.weight": torch.tensor(x["w"]).double(),
              "bias": torch.tensor(x["b"]).double()}
    r = R.fm_forward_f64(x["x"], x["E"], x["w"], x["b"], y=x["y"])
    z = O.fm_logit(params, torch.tensor(x["x"])).reshape(-1).double().requires_grad_(True)
    np.testing.assert_allclose(r["z"], z.detach().numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["sum_e"], x["E"].astype(np.float64)[x["x"]].sum(1), rtol=1e-13)
    np.testing.assert_array_equal(r["emb"], x["E"][x["x"]].reshape(B, F * K))
    assert (r["mag"] >= np.abs(r["z"]) - 1e-12).all()
    p = torch.sigmoid(z)
    loss = torch.nn.functional.binary_cross_entropy(p, torch.tensor(x["y"]).double(),
                                                    reduction="none")
    loss.mean().backward()
    np.testing.assert_allclose(r["p"], p.detach().numpy(), rtol=1e-13)
    np.testing.assert_allclose(r["loss_elem"], loss.detach().numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(r["gz"], z.grad.numpy(), rtol=1e-9, atol=1e-18)
    xi = R.int_fm_inputs(B, F, K, V, seed=K)
    ri = R.fm_forward_int(xi["x"], xi["E"], xi["w"], xi["b"])
    rf = R.fm_forward_f64(xi["x"], xi["E"], xi["w"], xi["b"])
    np.testing.assert_array_equal(ri["z"], rf["z"])
    np.testing.assert_array_equal(ri["sum_e"], rf["sum_e"])
    np.testing.assert_array_equal(ri["l1"], 2 * rf["mag"] - np.abs(xi["w"][xi["x"], 0]).sum(1)
                                  - abs(float(xi["b"][0])))
