"""The contract of the GEMM entry points (include/ctr_hip.h: ctr_gemm_f32_ex, ctr_gemm_f32,
ctr_gemm_planes, ctr_gemm_planes_lastcol) outside the one regime the other GEMM tests run in
(fresh, tight, aligned torch tensors compared within a tolerance): leading dimensions larger
than the extents, bases off a 16-byte boundary (the register-staged and scalar-store paths at
extents that ARE multiples of 4), K = 0 and k-tiles that are tails from the start, the
measured AUTO table, and the dropout mask / GRAD_MASK element by element against
tests/gemm_refs.py.

The calls go to the C ABI directly (hip_ops.gemm only takes contiguous tensors). Operands
live in poisoned slabs (gemm_refs.carve): NaN around every input, 777.0 around every output,
with a margin wide enough that a whole k-tile read past an operand stays inside the test's
own allocation; any USE of out-of-extent data shows as NaN in C, any stray store as a
changed sentinel.

Data: integers in [-3, 3] are exact in plane 0 of the bf16 split and every partial sum stays
below 2^24 (K <= 8192), so the exact-fp32 kernel, the split-bf16 kernel and the planes kernel
must all EQUAL the fp64 product, on every element; `==` on every element, so a NaN never
passes. Random data is held to the bar of test_gemm_every_tiling, 2e-6 * (|A| @ |B|).

The host-validation tests at the end need no GPU and carry no gpu mark.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import gemm_refs as R

gpu = pytest.mark.gpu

ALGO = {"exact": 1, "split": 2}  # enum ctr_gemm_algo
TRANS = [(0, 0), (0, 1), (1, 0), (1, 1)]
CTR_ERR_WORKSPACE = 3
# every compiled tiling of csrc/gemm.hip (kTiles) and csrc/gemm_sb16.hip (kSb16), as
# test_gemm_every_tiling
TILINGS = [("exact", t) for t in range(10)] + [("split", t) for t in range(8)]

_WS_QUERY = {"ctr_gemm_f32_ex": "ctr_gemm_f32_ex_workspace_bytes",
             "ctr_gemm_f32": "ctr_gemm_f32_workspace_bytes",
             "ctr_gemm_planes": "ctr_gemm_planes_workspace_bytes",
             "ctr_gemm_planes_lastcol": "ctr_gemm_planes_workspace_bytes"}


def _lib():
    from rl_ctr_prediction_amd._lib import lib
    return lib


def _H():
    from rl_ctr_prediction_amd import hip_ops
    return hip_ops


def _p(x):
    if x is None:
        return None
    if isinstance(x, R.Slab):
        return x.ptr()
    return x.data_ptr()


def _call(name, dev, head, tail, short=0):
    """lib.<name>(*head, *tail, ws, ws_bytes, stream) -> status. `head` = the leading
    ([algo,] orientation, M, N, K) arguments, which are also those of the matching
    *_workspace_bytes query; the workspace is exactly the queried size minus `short`."""
    lib = _lib()
    nbytes = getattr(lib, _WS_QUERY[name])(*head)
    assert nbytes >= 0, (name, head, nbytes)
    give = max(nbytes - short, 0)
    ws = torch.empty(max(give, 1), dtype=torch.uint8, device=dev) if nbytes else None
    return lib.raw(name)(*head, *tail, _p(ws), give, _H()._stream())


def _err():
    return _lib().load().ctr_last_error().decode(errors="replace")


def _gemm(dev, algo, ta, tb, M, N, K, A, lda, B, ldb, C, ldc, *, epi=R.EPI_NONE, bias=None,
          aux=None, ldaux=0, scale=1.0, p=0.0, seed=0, offset=0, step=None, short=0):
    """ctr_gemm_f32_ex, or ctr_gemm_f32 (CTR_GEMM_AUTO) for algo = None."""
    tail = (_p(A), lda, _p(B), ldb, _p(C), ldc, epi, _p(bias), _p(aux), ldaux, scale, p, seed,
            offset, _p(step))
    if algo is None:
        return _call("ctr_gemm_f32", dev, (ta, tb, M, N, K), tail, short)
    return _call("ctr_gemm_f32_ex", dev, (algo, ta, tb, M, N, K), tail, short)


def _planes_gemm(dev, a_rc, b_rc, M, N, K, pa, pb, C, ldc, *, Cp=None, epi=R.EPI_NONE,
                 bias=None, aux=None, ldaux=0, scale=1.0, p=0.0, seed=0, offset=0, step=None,
                 last_col=None, lastcol_entry=False):
    tail = [pa.desc, pb.desc, _p(C), ldc, Cp.desc if Cp is not None else None, epi, _p(bias),
            _p(aux), ldaux, scale, p, seed, offset, _p(step)]
    if lastcol_entry:
        return _call("ctr_gemm_planes_lastcol", dev, (a_rc, b_rc, M, N, K),
                     tail + [_p(last_col)])
    return _call("ctr_gemm_planes", dev, (a_rc, b_rc, M, N, K), tail)


def _ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def _int_problem(M, N, K, lo=-3):
    """A [M, K], B [K, N] (integers in [lo, 3]) and their fp64 product, computed once."""
    A, B = _ints((M, K), 1000 * M + 10 * N + K, lo), _ints((K, N), 7 * M + N + 100 * K + 1, lo)
    ref = A.double() @ B.double()
    assert float(ref.abs().max()) < 2 ** 24
    return A, B, ref


@functools.lru_cache(maxsize=None)
def _rand_problem(M, N, K):
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    A, B = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g)
    return A, B, A.double() @ B.double(), A.double().abs() @ B.double().abs()


def _stored(X, trans):
    """The stored form of a logical operand: X itself, or its transpose."""
    return (X.t() if trans else X).contiguous()


def _operand(X, trans, pad, off, dev):
    S = _stored(X, trans)
    return R.carve(S.shape[0], S.shape[1], S.shape[1] + pad, off, dev, values=S)


def _out(M, N, pad, off, dev):
    return R.carve(M, N, N + pad, off, dev, fill=R.SENTINEL)


def _check_out(Cs, want64, what):
    got = Cs.view.cpu()
    assert not got.isnan().any(), ("NaN in C", what)
    bad = got.double() != want64
    assert not bad.any(), (what, int(bad.sum()), "elements differ; first",
                           torch.nonzero(bad)[0].tolist())
    assert Cs.pad_intact(), ("stores outside C's valid region", what)
    return got


# ------------------------------------------------------------- a. layout matrix -------
# (A base offset, lda - extent, B base offset, ldb - extent, C base offset, ldc - N), floats
LAYOUTS = {
    "tight": (0, 0, 0, 0, 0, 0),
    "a_off1": (1, 0, 0, 0, 0, 0), "b_off1": (0, 0, 1, 0, 0, 0),
    "lda+1": (0, 1, 0, 0, 0, 0), "lda+4": (0, 4, 0, 0, 0, 0),
    "ldb+1": (0, 0, 0, 1, 0, 0), "ldb+4": (0, 0, 0, 4, 0, 0),
    "c_off1": (0, 0, 0, 0, 1, 0), "ldc+1": (0, 0, 0, 0, 0, 1), "ldc+4": (0, 0, 0, 0, 0, 4),
    "all": (1, 1, 1, 4, 1, 1), "all_swapped": (1, 4, 1, 1, 1, 4),
}


@gpu
@pytest.mark.parametrize("M,N,K", [(100, 72, 96), (97, 70, 33)])
@pytest.mark.parametrize("ta,tb", TRANS)
@pytest.mark.parametrize("algo", ["exact", "split"])
def test_layout_matrix(cuda, algo, ta, tb, M, N, K, monkeypatch):
    """Alignment and leading dimensions select a staging / store path, never a result. At
    (100, 72, 96) every extent is a multiple of 4, so the tight aligned call stages by LDS-DMA
    and stores float4, and each other variant moves one operand (or C) to the register-staged
    / scalar path at the SAME shape. Integer data: equal to fp64 and to the tight variant on
    every element. Random data: inside 2e-6 * (|A| @ |B|), and bitwise the tight variant's —
    both staging paths build the same LDS image and run the same MFMA sequence over it, and
    the store path does not touch the value."""
    monkeypatch.delenv("CTR_GEMM_CFG", raising=False)
    Ai, Bi, refi = _int_problem(M, N, K)
    Ar, Br, refr, boundr = _rand_problem(M, N, K)
    tight = {}
    for name, (oa, pa, ob, pb, oc, pc) in LAYOUTS.items():
        for kind, (A, B) in (("int", (Ai, Bi)), ("rand", (Ar, Br))):
            As, Bs = _operand(A, ta, pa, oa, cuda), _operand(B, tb, pb, ob, cuda)
            Cs = _out(M, N, pc, oc, cuda)
            rc = _gemm(cuda, ALGO[algo], ta, tb, M, N, K, As, As.ld, Bs, Bs.ld, Cs, Cs.ld)
            assert rc == 0, (name, _err())
            what = (algo, ta, tb, M, N, K, name, kind)
            if kind == "int":
                got = _check_out(Cs, refi, what)
            else:
                got = Cs.view.cpu()
                bad = ~((got.double() - refr).abs() <= 2e-6 * boundr + 1e-30)
                assert not bad.any(), (what, int(bad.sum()))
                assert Cs.pad_intact(), what
            assert As.pad_intact() and Bs.pad_intact()  # inputs are read-only
            if name == "tight":
                tight[kind] = got
            else:
                assert torch.equal(got.view(torch.int32), tight[kind].view(torch.int32)), what


# ------------------------------------------------------------------ b. K edges --------
K_EDGES = [0, 1, 3, 4, 8, 28, 31, 32, 33, 36, 60, 64, 65, 68, 100]


@gpu
@pytest.mark.parametrize("algo,tile", TILINGS)
def test_k_edges_every_tiling(cuda, algo, tile, monkeypatch):
    """M, N = 36, 40 on each compiled tiling, single pass: K below one k-tile (32, or 64 on the
    BK = 64 tilings) on the LDS-DMA path (K % 4 == 0) and on the register path, K one past a
    tile, K = 0. Every transpose, tight aligned operands inside poisoned slabs. K = 0 passes
    A = B = NULL and must give the epilogue of 0: zeros, or the broadcast bias."""
    monkeypatch.setenv("CTR_GEMM_CFG", f"{tile},1")
    M, N = 36, 40
    A_full, B_full, _ = _int_problem(M, N, max(K_EDGES))
    bias = _ints((N,), 99)
    bias_d = bias.to(cuda)
    for K in K_EDGES:
        A, B = A_full[:, :K], B_full[:K, :]
        ref = A.double() @ B.double()
        for ta, tb in TRANS:
            what = (algo, tile, K, ta, tb)
            Cs = _out(M, N, 0, 0, cuda)
            if K == 0:
                lda, ldb = (M if ta else 4), (4 if tb else N)
                rc = _gemm(cuda, ALGO[algo], ta, tb, M, N, 0, None, lda, None, ldb, Cs, N)
                assert rc == 0, (what, _err())
                _check_out(Cs, torch.zeros(M, N, dtype=torch.float64), what)
                Cs = _out(M, N, 0, 0, cuda)
                rc = _gemm(cuda, ALGO[algo], ta, tb, M, N, 0, None, lda, None, ldb, Cs, N,
                           epi=R.EPI_BIAS, bias=bias_d)
                assert rc == 0, (what, _err())
                _check_out(Cs, bias.double().expand(M, N), what + ("bias",))
                continue
            As, Bs = _operand(A, ta, 0, 0, cuda), _operand(B, tb, 0, 0, cuda)
            rc = _gemm(cuda, ALGO[algo], ta, tb, M, N, K, As, As.ld, Bs, Bs.ld, Cs, N)
            assert rc == 0, (what, _err())
            _check_out(Cs, ref, what)


@gpu
@pytest.mark.parametrize("algo,tile", TILINGS)
def test_k_edges_forced_split_k(cuda, algo, tile, monkeypatch):
    """CTR_GEMM_CFG = "tile,2": K = 65, 68, 100, 132 give slabs 64+1, 64+4, 64+36, 96+36 — a
    last slab whose FIRST k-tile is already a tail (BK = 32 and BK = 64 tilings), on the
    LDS-DMA path where the orientation allows it. ldc = N + 3 and BIAS_RELU put the reduce
    kernel's ldc and epilogue on the path."""
    monkeypatch.setenv("CTR_GEMM_CFG", f"{tile},2")
    M, N = 36, 40
    A_full, B_full, _ = _int_problem(M, N, 132)
    bias = _ints((N,), 98)
    bias_d = bias.to(cuda)
    lib = _lib()
    for K in (65, 68, 100, 132):
        A, B = A_full[:, :K], B_full[:K, :]
        want = torch.from_numpy(R.epilogue_ref((A.double() @ B.double()).numpy(),
                                               R.EPI_BIAS_RELU, bias=bias.numpy())).double()
        assert (want == 0).any() and (want > 0).any()
        for ta, tb in TRANS:
            what = (algo, tile, K, ta, tb)
            assert lib.ctr_gemm_f32_ex_workspace_bytes(ALGO[algo], ta, tb, M, N, K) == \
                2 * M * N * 4, what  # two slabs
            As, Bs = _operand(A, ta, 0, 0, cuda), _operand(B, tb, 0, 0, cuda)
            Cs = _out(M, N, 3, 0, cuda)
            rc = _gemm(cuda, ALGO[algo], ta, tb, M, N, K, As, As.ld, Bs, Bs.ld, Cs, Cs.ld,
                       epi=R.EPI_BIAS_RELU, bias=bias_d)
            assert rc == 0, (what, _err())
            _check_out(Cs, want, what)


# ------------------------------------------------- c. AUTO on the measured table ------
# kKnown of csrc/gemm.hip: (M, N, K, trans_a, trans_b, splits)
KNOWN = [(8192, 300, 1664, 0, 1, 2), (8192, 200, 300, 0, 1, 1), (8192, 300, 200, 0, 0, 1),
         (8192, 1664, 300, 0, 0, 1), (200, 300, 8192, 1, 0, 16), (300, 1664, 8192, 1, 0, 8),
         (4096, 1024, 741, 0, 1, 1), (1024, 741, 4096, 1, 0, 4), (4096, 512, 1024, 0, 1, 1),
         (4096, 1024, 512, 0, 0, 1), (512, 1024, 4096, 1, 0, 8)]


@gpu
@pytest.mark.parametrize("M,N,K,ta,tb,splits", KNOWN)
def test_auto_on_the_measured_table(cuda, M, N, K, ta, tb, splits, monkeypatch):
    """ctr_gemm_f32 (CTR_GEMM_AUTO) on each hand-measured (algo, tile, splits) row, in its
    listed orientation: integer data, equal to the fp64 product computed on the CPU. Rows
    with split-K first get a workspace one byte short: CTR_ERR_WORKSPACE, C untouched."""
    monkeypatch.delenv("CTR_GEMM_CFG", raising=False)
    lib = _lib()
    g = torch.Generator().manual_seed(K + N)
    A = torch.randint(-3, 4, (M, K), generator=g).float()
    B = torch.randint(-3, 4, (K, N), generator=g).float()
    ref = A.double() @ B.double()
    a, b = _stored(A, ta).to(cuda), _stored(B, tb).to(cuda)
    C = torch.full((M, N), R.SENTINEL, device=cuda)
    nbytes = lib.ctr_gemm_f32_workspace_bytes(ta, tb, M, N, K)
    if lib.raw("ctr_gemm_resolved_algo")(0) == ALGO["split"]:  # the table is in force
        assert nbytes == (splits * M * N * 4 if splits > 1 else 0), (nbytes, splits)
    if nbytes > 0:
        rc = _gemm(cuda, None, ta, tb, M, N, K, a, a.stride(0), b, b.stride(0), C, N, short=1)
        assert rc == CTR_ERR_WORKSPACE, (rc, _err())
        assert "workspace" in _err()
        assert bool((C == R.SENTINEL).all()), "C written by a refused call"
    rc = _gemm(cuda, None, ta, tb, M, N, K, a, a.stride(0), b, b.stride(0), C, N)
    assert rc == 0, _err()
    got = C.cpu().double()
    bad = got != ref
    assert not bad.any(), (int(bad.sum()), M, N, K, ta, tb)


# ------------------------------------------------ d. dropout against the reference ----
DROP_SEEDS = [0, 123, 2 ** 64 - 1]
DROP_OFFSETS = [0, 777, 2 ** 32 - 5, 2 ** 63]
DROP_STEPS = [None, 3, 2 ** 31 - 1]
DROP_M, DROP_N = 37, 50
# 0.15: float32(1 / (1 - p)) formed in double differs by one ulp from the fp32 quotient
# 1.0f / (1.0f - p), so a kernel scaling by the latter misses the kept values
DROP_P = [0.0, 0.15, 0.2, 0.5]


@functools.lru_cache(maxsize=None)
def _drop_problem(K):
    """A [M, K], W [N, K] non-negative integers, bias 1: every pre-activation is >= 1, so
    the zeros of the output are exactly the dropped elements."""
    A, Bm, ref = _int_problem(DROP_M, DROP_N, K, lo=0)
    return A, Bm.t().contiguous(), ref, torch.ones(DROP_N)


@functools.lru_cache(maxsize=None)
def _drop_want(K, p, seed, offset, step):
    _, _, ref, bias = _drop_problem(K)
    keep = R.dropout_keep(DROP_M, DROP_N, p, seed, offset, step)
    want = R.epilogue_ref(ref.numpy(), R.EPI_BIAS_RELU_DROP, bias=bias.numpy(), keep=keep,
                          drop_scale=R.drop_scale(p))
    assert np.array_equal(want == 0, ~keep)
    return torch.from_numpy(want).double(), torch.from_numpy(~keep)


def _drop_cases(cuda):
    steps = {s: (None if s is None else torch.tensor([s], dtype=torch.int32, device=cuda))
             for s in DROP_STEPS}
    for seed in DROP_SEEDS:
        for offset in DROP_OFFSETS:
            for s, sd in steps.items():
                yield seed, offset, s, sd


@gpu
@pytest.mark.parametrize("p", DROP_P)
@pytest.mark.parametrize("K,cfg", [(16, None), (96, "0,2")])
@pytest.mark.parametrize("algo", ["exact", "split"])
def test_dropout_mask_is_the_documented_hash(cuda, algo, K, cfg, p, monkeypatch):
    """keep(m, n) iff hash_u32(seed, offset + (step << 32) + m*N + n) >= float32(p) * 2^32,
    kept values float32(v) * float32(1 / (1 - p)): the set of zeros and every kept value,
    for 64-bit seeds and offsets, a device step of 3 and of 2^31 - 1, at ldc = N + 3 (the
    counter runs over N, not ldc). (37, 50, 96) under CTR_GEMM_CFG = "0,2" takes the split-K
    path, where the reduce kernel applies the epilogue and must add the step itself."""
    if cfg is None:
        monkeypatch.delenv("CTR_GEMM_CFG", raising=False)
    else:
        monkeypatch.setenv("CTR_GEMM_CFG", cfg)
    M, N = DROP_M, DROP_N
    A, W, _, bias = _drop_problem(K)
    nbytes = _lib().ctr_gemm_f32_ex_workspace_bytes(ALGO[algo], 0, 1, M, N, K)
    assert nbytes == (2 * M * N * 4 if cfg else 0)
    a, w, bias_d = A.to(cuda), W.to(cuda), bias.to(cuda)
    for seed, offset, s, sd in _drop_cases(cuda):
        what = (algo, K, p, seed, offset, s)
        want, dropped = _drop_want(K, p, seed, offset, s)
        Cs = _out(M, N, 3, 0, cuda)
        rc = _gemm(cuda, ALGO[algo], 0, 1, M, N, K, a, K, w, K, Cs, Cs.ld,
                   epi=R.EPI_BIAS_RELU_DROP, bias=bias_d, p=p, seed=seed, offset=offset, step=sd)
        assert rc == 0, (what, _err())
        got = Cs.view.cpu()
        assert torch.equal(got == 0, dropped), (what, "the set of zeros is not ~keep")
        _check_out(Cs, want, what)


@gpu
@pytest.mark.parametrize("p", DROP_P)
@pytest.mark.parametrize("K,cfg", [(16, None), (96, "4,2")])
@pytest.mark.parametrize("mode", ["out", "out_planes"])
def test_dropout_mask_planes(cuda, mode, K, cfg, p, monkeypatch):
    """The same reference for ctr_gemm_planes, writing fp32 C only (ldc = N + 3) and the
    output planes only; (37, 50, 96) under CTR_GEMM_PLANES_CFG = "4,2" goes through
    planes_reduce_kernel."""
    H = _H()
    if cfg is None:
        monkeypatch.delenv("CTR_GEMM_PLANES_CFG", raising=False)
    else:
        monkeypatch.setenv("CTR_GEMM_PLANES_CFG", cfg)
        assert H.gemm_planes_config(False, False, DROP_M, DROP_N, K)["splits"] == 2
    M, N = DROP_M, DROP_N
    A, W, _, bias = _drop_problem(K)
    pa, pw, bias_d = H.split_planes(A.to(cuda)), H.split_planes(W.to(cuda)), bias.to(cuda)
    for seed, offset, s, sd in _drop_cases(cuda):
        what = (mode, K, p, seed, offset, s)
        want, dropped = _drop_want(K, p, seed, offset, s)
        kw = dict(epi=R.EPI_BIAS_RELU_DROP, bias=bias_d, p=p, seed=seed, offset=offset, step=sd)
        if mode == "out":
            Cs = _out(M, N, 3, 0, cuda)
            rc = _planes_gemm(cuda, 0, 0, M, N, K, pa, pw, Cs, Cs.ld, **kw)
            assert rc == 0, (what, _err())
            assert torch.equal(Cs.view.cpu() == 0, dropped), what
            _check_out(Cs, want, what)
        else:
            Cp = H.Planes(M, N, cuda)
            rc = _planes_gemm(cuda, 0, 0, M, N, K, pa, pw, None, 0, Cp=Cp, **kw)
            assert rc == 0, (what, _err())
            got = Cp.to_float().cpu()
            assert torch.equal(got == 0, dropped), what
            assert torch.equal(got.double(), want), what
            t = Cp.t.float()
            assert bool((t[:, M:, :] == 0).all()) and bool((t[:, :, N:] == 0).all()), what


# ------------------------------------------------------------------ e. GRAD_MASK ------
@gpu
@pytest.mark.parametrize("kernel", ["exact", "split", "planes"])
def test_grad_mask_strided_aux(cuda, kernel, monkeypatch):
    """C = aux > 0 ? (A.B) * scale : 0 with aux at ldaux = N + 5, one float off a 16-byte
    boundary, drawn from {-1, -0.0, 0.0, 1, +inf}; aux's pad columns hold 1.0, so indexing
    aux by anything but m*ldaux + n lets masked elements through."""
    monkeypatch.delenv("CTR_GEMM_CFG", raising=False)
    monkeypatch.delenv("CTR_GEMM_PLANES_CFG", raising=False)
    M, N, K = 37, 50, 40
    A, B, ref = _int_problem(M, N, K)
    g = torch.Generator().manual_seed(4)
    vals = torch.tensor([-1.0, -0.0, 0.0, 1.0, float("inf")])
    aux = vals[torch.randint(0, 5, (M, N), generator=g)]
    auxs = R.carve(M, N, N + 5, 1, cuda, fill=1.0, values=aux)
    want = torch.from_numpy(R.epilogue_ref(ref.numpy(), R.EPI_GRAD_MASK, aux=aux.numpy(),
                                           scale=1.25)).double()
    assert (want != 0).any() and (want[aux <= 0] == 0).all()
    Cs = _out(M, N, 0, 0, cuda)
    if kernel == "planes":
        H = _H()
        pa, pb = H.split_planes(A.to(cuda)), H.split_planes(B.t().contiguous().to(cuda))
        rc = _planes_gemm(cuda, 0, 0, M, N, K, pa, pb, Cs, N, epi=R.EPI_GRAD_MASK, aux=auxs,
                          ldaux=auxs.ld, scale=1.25)
    else:
        a, b = A.to(cuda), B.to(cuda)
        rc = _gemm(cuda, ALGO[kernel], 0, 0, M, N, K, a, K, b, N, Cs, N, epi=R.EPI_GRAD_MASK,
                   aux=auxs, ldaux=auxs.ld, scale=1.25)
    assert rc == 0, _err()
    _check_out(Cs, want, kernel)
    assert torch.equal(auxs.view.cpu().view(torch.int32), aux.view(torch.int32))


# ------------------------------------------------------------ f. planes outputs -------
def _planes_operands(H, A, B, a_rc, b_rc, dev, ones_col=False):
    """Planes of A [M, K] (stored [K, M] when a_rc) and of B [K, N] (stored [N, K] unless
    b_rc; with ones_col the b_rc planes carry a ones column after column N - 1)."""
    pa = H.split_planes(_stored(A, a_rc).to(dev))
    Bs = _stored(B, not b_rc).to(dev)
    pb = H.Planes(Bs.shape[0], Bs.shape[1], dev, ones_col=ones_col)
    H.split_planes(Bs, out=pb)
    return pa, pb


@gpu
@pytest.mark.parametrize("M,N,K", [(37, 45, 100), (130, 72, 64)])
def test_planes_output_layouts(cuda, M, N, K, monkeypatch):
    """ctr_gemm_planes with C at ldc in {N, N + 1, N + 4} and base offset {0, 1}, every
    orientation: equal to fp64, bitwise the tight aligned call's, pads and margins intact."""
    monkeypatch.delenv("CTR_GEMM_PLANES_CFG", raising=False)
    H = _H()
    A, B, ref = _int_problem(M, N, K)
    for a_rc, b_rc in TRANS:
        pa, pb = _planes_operands(H, A, B, a_rc, b_rc, cuda)
        tight = None
        for pad in (0, 1, 4):
            for off in (0, 1):
                what = (M, N, K, a_rc, b_rc, pad, off)
                Cs = _out(M, N, pad, off, cuda)
                rc = _planes_gemm(cuda, a_rc, b_rc, M, N, K, pa, pb, Cs, Cs.ld)
                assert rc == 0, (what, _err())
                got = _check_out(Cs, ref, what)
                if tight is None:
                    tight = got
                assert torch.equal(got.view(torch.int32), tight.view(torch.int32)), what


@gpu
@pytest.mark.parametrize("M,N,K", [(37, 45, 100), (130, 72, 64)])
def test_planes_lastcol_layouts(cuda, M, N, K, monkeypatch):
    """ctr_gemm_planes_lastcol: B's planes carry a ones column, the call asks for N + 1
    columns, C holds the first N at ldc in {N, N + 1, N + 4} (relative to the N columns
    stored) and base offset {0, 1}, and last_col the (N + 1)-th: the sums over k of A,
    exactly. Nothing is stored past last_col[M - 1] or outside C's valid region."""
    monkeypatch.delenv("CTR_GEMM_PLANES_CFG", raising=False)
    H = _H()
    A, B, ref = _int_problem(M, N, K)
    sums = A.double().sum(1)
    for a_rc in (0, 1):
        pa, pb = _planes_operands(H, A, B, a_rc, 1, cuda, ones_col=True)
        tight = None
        for pad in (0, 1, 4):
            for off in (0, 1):
                what = (M, N, K, a_rc, pad, off)
                Cs = _out(M, N, pad, off, cuda)
                lc = R.carve(1, M, M, 0, cuda, fill=R.SENTINEL)
                rc = _planes_gemm(cuda, a_rc, 1, M, N + 1, K, pa, pb, Cs, Cs.ld, last_col=lc,
                                  lastcol_entry=True)
                assert rc == 0, (what, _err())
                got = _check_out(Cs, ref, what)
                assert torch.equal(lc.view.cpu().double().reshape(-1), sums), what
                assert lc.pad_intact(), what
                if tight is None:
                    tight = got
                assert torch.equal(got.view(torch.int32), tight.view(torch.int32)), what


@gpu
def test_planes_k_zero_gives_the_epilogue_of_zero(cuda, monkeypatch):
    """K = 0 with Planes(rows, 0) operands (all padding, all zero): EPI_BIAS gives the
    broadcast bias, EPI_NONE zeros."""
    monkeypatch.delenv("CTR_GEMM_PLANES_CFG", raising=False)
    H = _H()
    M, N = 37, 45
    pa, pb = H.Planes(M, 0, cuda), H.Planes(N, 0, cuda)
    bias = _ints((N,), 97)
    Cs = _out(M, N, 1, 1, cuda)
    rc = _planes_gemm(cuda, 0, 0, M, N, 0, pa, pb, Cs, Cs.ld, epi=R.EPI_BIAS, bias=bias.to(cuda))
    assert rc == 0, _err()
    _check_out(Cs, bias.double().expand(M, N), "bias")
    Cs = _out(M, N, 1, 1, cuda)
    rc = _planes_gemm(cuda, 0, 0, M, N, 0, pa, pb, Cs, Cs.ld)
    assert rc == 0, _err()
    _check_out(Cs, torch.zeros(M, N, dtype=torch.float64), "none")


# ------------------------------------------------- g. host validation (no GPU) --------
@pytest.fixture(scope="module")
def built_lib():
    from rl_ctr_prediction_amd.build_lib import LIB, build
    try:
        build()
    except RuntimeError as e:  # no hipcc in this environment
        pytest.skip(str(e))
    return LIB


def _f32_args(ta=0, tb=0, M=8, N=12, K=20, lda=None, ldb=None, ldc=None, epi=R.EPI_NONE,
              ldaux=0, p=0.0, algo=1, aux=None, bias=None):
    """ctr_gemm_f32_ex arguments that pass every check unless overridden; the pointers are
    never dereferenced (a refused call launches nothing)."""
    lda = (M if ta else K) if lda is None else lda
    ldb = (K if tb else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    return (algo, ta, tb, M, N, K, 64, lda, 64, ldb, 64, ldc, epi, bias, aux, ldaux, 1.0, p, 0, 0,
            None, None, 0, None)


@pytest.mark.parametrize("ta,tb", TRANS)
def test_leading_dimensions_below_the_minimum_are_refused(built_lib, ta, tb):
    """lda >= (trans_a ? M : K), ldb >= (trans_b ? K : N), ldc >= N, checked on the host
    before any launch, for each orientation."""
    from rl_ctr_prediction_amd._lib import CtrHipError, lib
    M, N, K = 8, 12, 20
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: lda too small"):
        lib.ctr_gemm_f32_ex(*_f32_args(ta, tb, lda=(M if ta else K) - 1))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: ldb too small"):
        lib.ctr_gemm_f32_ex(*_f32_args(ta, tb, ldb=(K if tb else N) - 1))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: bad C"):
        lib.ctr_gemm_f32_ex(*_f32_args(ta, tb, ldc=N - 1))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: lda too small"):
        lib.ctr_gemm_f32(*_f32_args(ta, tb, lda=(M if ta else K) - 1)[1:])


def test_gemm_argument_checks_without_gpu(built_lib):
    from rl_ctr_prediction_amd._lib import CtrHipError, lib
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: aux missing"):
        lib.ctr_gemm_f32_ex(*_f32_args(epi=R.EPI_GRAD_MASK, aux=64, ldaux=11))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: aux missing"):
        lib.ctr_gemm_f32_ex(*_f32_args(epi=R.EPI_GRAD_MASK, aux=None, ldaux=12))
    with pytest.raises(CtrHipError, match=r"ctr_gemm_f32: dropout p must be in \[0,1\)"):
        lib.ctr_gemm_f32_ex(*_f32_args(epi=R.EPI_BIAS_RELU_DROP, bias=64, p=1.0))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: dropout p"):
        lib.ctr_gemm_f32_ex(*_f32_args(p=-0.5))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: bad algo 3"):
        lib.ctr_gemm_f32_ex(*_f32_args(algo=3))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: bad algo -1"):
        lib.ctr_gemm_f32_ex(*_f32_args(algo=-1))
    for neg in (dict(M=-1), dict(N=-1), dict(K=-1)):
        with pytest.raises(CtrHipError, match="ctr_gemm_f32: negative size"):
            lib.ctr_gemm_f32_ex(*_f32_args(**neg, lda=64, ldb=64, ldc=64))
    with pytest.raises(CtrHipError, match="ctr_gemm_f32: null operand"):
        a = list(_f32_args())
        a[6] = None
        lib.ctr_gemm_f32_ex(*a)
    dll = lib.load()
    assert dll.ctr_gemm_f32_ex_workspace_bytes(3, 0, 0, 8, 8, 8) == -1
    assert dll.ctr_gemm_f32_ex_workspace_bytes(1, 0, 0, -1, 8, 8) == -1
    assert dll.ctr_gemm_f32_ex_workspace_bytes(1, 0, 0, 8, 8, 0) == 0


def test_planes_argument_checks_without_gpu(built_lib):
    """ctr_gemm_planes / _lastcol: ldc against the columns actually stored, and GRAD_MASK's
    aux needs ldaux >= N as in ctr_gemm_f32_ex."""
    from rl_ctr_prediction_amd._lib import CtrHipError, PlanesDesc, lib
    M, N, K = 8, 12, 20
    pl = PlanesDesc(64, 32, 32 * 32, 32, 32)  # [3][32][32], never dereferenced

    def args(ldc=N, epi=R.EPI_NONE, aux=None, ldaux=0, p=0.0, M=M, N=N, K=K):
        return [0, 0, M, N, K, pl, pl, 64, ldc, None, epi, None, aux, ldaux, 1.0, p, 0, 0, None]

    tail = [None, 0, None]  # ws, ws_bytes, stream
    with pytest.raises(CtrHipError, match="ctr_gemm_planes: ldc < N"):
        lib.ctr_gemm_planes(*args(ldc=N - 1), *tail)
    with pytest.raises(CtrHipError, match="ctr_gemm_planes: ldc < N"):
        lib.ctr_gemm_planes_lastcol(*args(ldc=N - 2), 64, *tail)
    for fn, extra in ((lib.ctr_gemm_planes, []), (lib.ctr_gemm_planes_lastcol, [64])):
        with pytest.raises(CtrHipError, match="ctr_gemm_planes: GRAD_MASK needs aux with ldaux >= N"):
            fn(*args(epi=R.EPI_GRAD_MASK, aux=64, ldaux=N - 1), *extra, *tail)
        with pytest.raises(CtrHipError, match="ctr_gemm_planes: GRAD_MASK needs aux"):
            fn(*args(epi=R.EPI_GRAD_MASK, aux=None, ldaux=N), *extra, *tail)
        with pytest.raises(CtrHipError, match="ctr_gemm_planes: drop_p out of range"):
            fn(*args(epi=R.EPI_BIAS_RELU_DROP, p=1.0), *extra, *tail)
        with pytest.raises(CtrHipError, match="ctr_gemm_planes: negative size"):
            fn(*args(K=-1), *extra, *tail)
