"""Plain numpy references for the wave-per-example pair-input kernels built on
stage_rows_wave (csrc/ctr_common.h): Feature_Embedding's state (csrc/fm_forward.hip) and the
IPNN MLP input with its slot gradients (csrc/pnn.hip), and the shapes that put them on every
edge of their dispatch. Nothing here touches the library: tests/test_pair_input_refs.py
checks it on the CPU, tests/test_gpu_pair_inputs.py runs the kernels against it.

* fe_ref / ipnn_cat_ref / ipnn_bwd_ref: float64, each with the per-element L1 scale of its
  summands (sum |e_i||e_j| for a dot, |dflat| + sum_j |d_fj||e_j| for a slot gradient; the
  copied flat part's scale is |e|) — the bar of test_ipnn_forward_and_backward_vs_oracle is
  1e-5 x that scale;
* ipnn_dots_f32 / ipnn_walk_f32: the fp32 emulation of the order the kernel comments promise
  ("torch.mul, then torch.sum", contraction off, k ascending; the walks' j ascending, j != f);
* int_case: small-integer tables and dcat, for which every summation order is exact in fp32;
* the dispatch predicates of the launchers, restated from their rules, and EDGE_SHAPES, which
  takes every label of every predicate (asserted on the CPU).
"""
from __future__ import annotations

import numpy as np

WAVE = 64
F32 = np.float32
LDS_LIMIT = 160 * 1024  # bytes of dynamic LDS a block may ask for (ipnn_check)
LDS_ASK = 64 * 1024  # past this the launcher asks for it (allow_lds, csrc/ctr_common.h)
REG_LDS = 4 * (32 * 31 // 2) * 4  # the register walk's pair values: 4 waves x 496 floats
V_EDGE = 97  # rows of the tables the edge tests use
B_EDGE = 5  # two blocks of 4 waves, the second with one wave

# (F, K) by the edge it is there for (the union is EDGE_SHAPES)
EDGES = {
    "smallest shapes, the unaligned flat store": ((2, 1), (2, 4), (3, 5)),
    "P = 55 / 66 around one wave of pairs": ((11, 8), (12, 8)),
    "scalar-operand walk, K in {1, 10, 16, 63}": ((22, 10), (22, 63), (26, 1), (26, 16)),
    "register walk at F = 32, K either side of 32 and at 63": ((32, 33), (32, 63)),
    "matrix-core product: F = 2, odd F, F = 31 / 32, K = 32 x {1, 2, 3, 4}":
        ((2, 32), (31, 32), (32, 32), (32, 64), (5, 96), (22, 128)),
    "LDS tile: F > 32, or K > 64 with K % 32 != 0": ((33, 8), (33, 64), (5, 65), (7, 68)),
    "staging fast path at exactly F K = 2048": ((32, 64), (64, 32)),
    "staging fast path just past F K = 2048": ((33, 64),),
    "staging at F = 64 without the fast path": ((64, 5),),
    "chunked staging, f0 > 0 with a 1-field last chunk": ((65, 4), (129, 4)),
    "forward at the last size under 64 KB": ((31, 128),),
    "dynamic LDS past 64 KB": ((32, 128), (64, 32), (39, 128)),
}
EDGE_SHAPES = tuple(dict.fromkeys(s for v in EDGES.values() for s in v))
# shapes past LDS_LIMIT, refused before any launch: (F, K) of the forward, of the tile
# backward and of Feature_Embedding
REFUSED_FWD, REFUSED_BWD, REFUSED_FE = (64, 160), (150, 4), (64, 160)


# ------------------------------------------------------------------ dispatch ---------
def n_pairs(F: int) -> int:
    return F * (F - 1) // 2


def width(F: int, K: int) -> int:
    return F * K + n_pairs(F)


def stage_path(F: int, K: int, aligned: bool = True) -> str:
    """stage_rows_wave: `vec` (float4 pieces, every load in flight: F <= 64, K % 4 == 0,
    F K <= 2048 and a 16-byte-aligned table), else the element loop — `loop` in one chunk of
    up to 64 fields, `chunked` past 64 (f0 > 0)."""
    if F <= 64 and K % 4 == 0 and F * K <= 2048 and aligned:
        return "vec"
    return "chunked" if F > 64 else "loop"


def last_chunk(F: int) -> int:
    """Fields of the element loop's last chunk."""
    return F - 64 * ((F - 1) // 64)


def flat_aligned(offset: int) -> bool:
    """The vec staging path's flat store of an example whose flat part starts `offset` floats
    past a 16-byte boundary (b x ldc for IPNN, b x W + P for Feature_Embedding): float4
    stores when aligned, four scalar stores otherwise."""
    return offset % 4 == 0


def fwd_stride(K: int) -> int:
    """LDS row stride of ipnn_forward_kernel: K + 4 (float4 reads in the dots) or K + 1."""
    return K + 4 if K % 4 == 0 else K + 1


def bwd_kernel(F: int, K: int, env: str = "") -> str:
    """The kernel ctr_ipnn_backward launches under CTR_IPNN_BWD=env (its first letter
    counts): `mfma` the matrix-core product, `sreg` the scalar-operand walk, `reg` the
    register walk, `lds` the LDS tile."""
    e = env[:1]
    if e in ("", "m") and F <= 32 and K % 32 == 0:
        return "mfma"
    if e == "l" or F > 32 or K > 64:
        return "lds"
    if e != "r" and F in (26, 22):
        return "sreg"
    return "reg"


def bwd_modes(F: int, K: int):
    """[(env, kernel)]: the default and every CTR_IPNN_BWD value that selects the kernel it
    names at this shape."""
    out = [("", bwd_kernel(F, K))]
    for env, kern in (("m", "mfma"), ("sreg", "sreg"), ("reg", "reg"), ("lds", "lds")):
        if bwd_kernel(F, K, env) == kern:
            out.append((env, kern))
    return out


def lds_bytes_fe(F: int, K: int) -> int:
    return 16 * F * (K + 1)


def lds_bytes_fwd(F: int, K: int) -> int:
    return 16 * F * fwd_stride(K)


def lds_bytes_bwd(F: int, K: int, kernel: str = "lds") -> int:
    """Dynamic LDS of a block of the backward kernel that is launched."""
    if kernel == "lds":
        return 16 * (F * (K + 1) + n_pairs(F))
    return REG_LDS if kernel == "reg" else 0


def lds_class(nbytes: int) -> str:
    return "refused" if nbytes > LDS_LIMIT else "asked" if nbytes > LDS_ASK else "plain"


# ------------------------------------------------------------------- inputs ----------
def float_case(F: int, K: int, B: int, V: int, seed: int, ldd_extra: int = 3) -> dict:
    """N(0, 1) tables and dcat (ldd_extra columns wider than W), random ids with a repeated
    id inside example 0 (and a row used by two examples where B > 1)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, V, (B, F))
    x[0, 0] = x[0, F - 1]
    if B > 1:
        x[B - 1, F // 2] = x[0, F // 2]
    return dict(x=x, E=rng.standard_normal((V, K)).astype(F32),
                dcat=rng.standard_normal((B, width(F, K) + ldd_extra)).astype(F32))


def int_case(F: int, K: int, B: int, V: int, seed: int, ldd_extra: int = 3) -> dict:
    """Integer-valued fp32 tables and dcat in [-8, 8]: a dot's L1 norm is at most 64 K and a
    slot gradient's 8 + 64 (F - 1), far below 2^24, so every summation order (the matrix
    core's too) is exact and the int64 result must come back as it is."""
    rng = np.random.default_rng(seed)
    c = float_case(F, K, B, V, seed, ldd_extra)
    c["E"] = rng.integers(-8, 9, (V, K)).astype(F32)
    c["dcat"] = rng.integers(-8, 9, c["dcat"].shape).astype(F32)
    return c


# --------------------------------------------------------------- float64 --------------
def _pairs(F):
    return np.triu_indices(F, k=1)  # row-major (0,1),(0,2)..(0,F-1),(1,2)..


def _dots(e):
    i, j = _pairs(e.shape[1])
    return np.einsum("bpk,bpk->bp", e[:, i], e[:, j])


def ipnn_cat_ref(E, x):
    """(cat, scale) float64 [B, F K + P]: flat(E[x]) ++ <e_i, e_j>, i < j."""
    e = np.asarray(E, np.float64)[x]
    B = e.shape[0]
    a = np.abs(e)
    return (np.concatenate([e.reshape(B, -1), _dots(e)], 1),
            np.concatenate([a.reshape(B, -1), _dots(a)], 1))


def fe_ref(E, x):
    """(state, scale) float64 [B, P + F K]: Feature_Embedding's pair dots, then the rows."""
    cat, scale = ipnn_cat_ref(E, x)
    FK = x.shape[1] * np.asarray(E).shape[1]
    swap = lambda a: np.concatenate([a[:, FK:], a[:, :FK]], 1)  # noqa: E731
    return swap(cat), swap(scale)


def pair_matrix(dcat, F: int, K: int):
    """D [B, F, F]: the symmetric matrix of dcat's pair columns, zero diagonal."""
    dcat = np.asarray(dcat)
    i, j = _pairs(F)
    D = np.zeros((dcat.shape[0], F, F), dcat.dtype)
    D[:, i, j] = D[:, j, i] = dcat[:, F * K:width(F, K)]
    return D


def ipnn_bwd_ref(E, x, dcat):
    """(dslot, scale) float64 [B F, K]: dflat + D e per example."""
    E = np.asarray(E, np.float64)
    B, F = x.shape
    K = E.shape[1]
    e, d = E[x], np.asarray(dcat, np.float64)
    D, dflat = pair_matrix(d, F, K), d[:, :F * K].reshape(B, F, K)
    g = dflat + np.einsum("bfj,bjk->bfk", D, e)
    s = np.abs(dflat) + np.einsum("bfj,bjk->bfk", np.abs(D), np.abs(e))
    return g.reshape(B * F, K), s.reshape(B * F, K)


# ------------------------------------------------------- fp32, documented order -------
def ipnn_dots_f32(E, x):
    """[B, P] fp32: acc = fl(acc + fl(e_i[k] e_j[k])) for k ascending from 0."""
    e = np.asarray(E, F32)[x]
    i, j = _pairs(e.shape[1])
    ei, ej = e[:, i], e[:, j]
    acc = np.zeros(ei.shape[:2], F32)
    for k in range(e.shape[2]):
        acc = acc + ei[:, :, k] * ej[:, :, k]
    assert acc.dtype == F32
    return acc


def ipnn_walk_f32(E, x, dcat):
    """[B F, K] fp32: g = dflat[f, k], then g = fl(g + fl(d(f, j) e_j[k])) for j ascending,
    j != f."""
    E = np.asarray(E, F32)
    B, F = x.shape
    K = E.shape[1]
    e, d = E[x], np.asarray(dcat, F32)
    D = pair_matrix(d, F, K)
    g = d[:, :F * K].reshape(B, F, K).copy()
    rows = np.arange(F)[None, :, None]
    for j in range(F):  # every f at once: the term of j, skipped where f == j
        g = np.where(rows == j, g, g + D[:, :, j, None] * e[:, None, j, :])
    assert g.dtype == F32
    return g.reshape(B * F, K)
