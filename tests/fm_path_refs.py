"""Plain numpy references for the fused FM forward (csrc/fm_forward.hip) and the segmented
row sums (csrc/sparse_grad.hip), and the slot layouts that put a row's run of sorted
positions on every path edge of the latter. Nothing here touches the library:
tests/test_fm_path_refs.py checks it on the CPU, tests/test_gpu_fm_path.py runs the kernels
against it.

* seg_class: the (K, alignment) -> (vec, KV, LPR, C, G, T) dispatch of launch_seg, seg_chunk
  and seg_combine_apply_kernel, restated from their rules;
* edge_runs / tiny_layouts / long_runs: run lengths, one per unique row in ascending row
  order, so that seg_offsets = cumsum by construction; layout_cases names the lettered cases
  (a .. i of the docstring of edge_runs) a list of run lengths contains;
* keys_from_runs: keys whose sparse plan is that layout (row ids with gaps, slots permuted);
* seg_sums_f64 / seg_sums_f32_tree: the per-row sums in float64 with the L1 norm of their
  summands, and the fp32 emulation of the kernels' documented summation order;
* fm_forward_f64 / fm_forward_int: the FM forward in float64, and exactly in integers.

Integer inputs (int_seg_inputs, int_fm_inputs) make every correct summation order exact in
fp32 as long as the L1 norm of each sum stays below 2^23; test_fm_path_refs.py asserts that
for the largest layouts and shapes the GPU tests use.
"""
from __future__ import annotations

import numpy as np

WAVE = 64
# every K of the segmented-sum tests; 65 and 260 (and 128 misaligned) are unsupported
SEG_K = (1, 3, 4, 8, 10, 12, 16, 17, 32, 33, 64, 128, 256)
SEG_K_MISALIGNED = (16, 64)
SEG_UNSUPPORTED = ((65, True), (260, True), (128, False))
F32 = np.float32


# ------------------------------------------------------------------ dispatch ---------
def seg_class(K: int, aligned: bool = True):
    """(vec, KV, LPR, C, G, T) of a segmented row sum over rows of K floats, or None where
    launch_seg returns `unsupported`.

    vec: float4 columns (K % 4 == 0, every buffer 16-byte aligned, K / 4 <= 64), else float;
    KV = K / 4 or K columns; LPR = the power of two >= KV lanes per row, at most a wave;
    C = seg_chunk<LPR>() sorted positions per chunk: 16 when LPR >= 16, else 4;
    G = 64 / LPR lane groups (accumulators of a spanning row's pieces);
    T = clamp(G, 8, 16): most pieces one lane group of seg_combine_apply_kernel sums alone."""
    vec = K % 4 == 0 and aligned and K // 4 <= 64
    KV = K // 4 if vec else K
    LPR = 1
    while LPR < KV:
        LPR *= 2
    if LPR > WAVE:
        return None
    C = 16 if LPR >= 16 else 4
    G = WAVE // LPR
    T = min(max(G, 8), 16)
    return vec, KV, LPR, C, G, T


def seg_classes():
    """{(C, G, T): [(K, aligned), ...]} over SEG_K aligned and SEG_K_MISALIGNED misaligned."""
    out: dict = {}
    for K, al in [(K, True) for K in SEG_K] + [(K, False) for K in SEG_K_MISALIGNED]:
        out.setdefault(seg_class(K, al)[3:], []).append((K, al))
    return out


# ------------------------------------------------------------------- layouts ---------
def row_pieces(runs, C: int):
    """(off0, off1, P) per row: its run [off0, off1) of sorted positions and the number of
    C-position chunks the run touches."""
    runs = np.asarray(runs, dtype=np.int64)
    assert runs.ndim == 1 and runs.size > 0 and (runs > 0).all()
    off1 = np.cumsum(runs)
    off0 = off1 - runs
    return off0, off1, (off1 - 1) // C - off0 // C + 1


def edge_P(G: int, T: int):
    """The piece counts of case f: every side of the G (accumulator wrap) and T (own lane
    group / whole wave) edges, those >= 2, once each."""
    return sorted({P for P in (2, 3, G - 1, G, G + 1, T, T + 1, 2 * T + 3) if P >= 2})


class _Runs:
    """Run lengths appended one row at a time, with the position and ordinal they reach."""

    def __init__(self, C):
        self.C, self.runs, self.pos = C, [], 0

    @property
    def U(self):
        return len(self.runs)

    def add(self, n):
        assert n >= 1
        self.runs.append(int(n))
        self.pos += int(n)

    def to_offset(self, m):
        """1-slot rows until the next row starts at position m of a chunk."""
        while self.pos % self.C != m:
            self.add(1)

    def to_ordinal(self, g, G):
        """1-slot rows until the next row's ordinal is g modulo G."""
        while self.U % G != g:
            self.add(1)

    def spanning(self, P, r):
        """A row of P >= 2 pieces from the current position whose last piece holds r slots."""
        assert P >= 2 and 1 <= r <= self.C
        self.add((self.C - self.pos % self.C) + (P - 2) * self.C + r)


def edge_runs(C: int, G: int, T: int):
    """Run lengths whose rows sit on every edge of seg_chunk_kernel / seg_combine_kernel /
    seg_combine_apply_kernel for chunk size C, G lane groups and threshold T:

    a. a run of exactly C starting on a chunk boundary;
    b. a run of C + 1 starting on a boundary: 2 pieces, the first in partial slot [0];
    c. a run starting mid-chunk that ends exactly on a boundary, >= 2 pieces: the first in
       slot [1];
    d. a chunk with the tail of a spanning row, a row wholly inside, the head of the next
       spanning row, in that order;
    e. a 1-slot row on the last position of a chunk, then a row starting on the boundary;
    f. rows of every piece count of edge_P(G, T), once from a boundary and once mid-chunk;
    g. (G > 1) two rows of more than T pieces in one aligned group of G consecutive rows, with
       a 1-piece row and a 2..T-piece row between them where the group holds four rows
       (G >= 4; at G = 2 the two rows are the whole group);
    h. (G > 1) a number of rows that is no multiple of G (a tail wave with idle lane groups);
    i. a number of slots that is no multiple of C, the last row spanning into the final,
       partial chunk.

    layout_cases finds each of them again from the run lengths alone."""
    assert C >= 4 and G >= 1 and T >= 2
    L = _Runs(C)
    L.add(C)                      # a
    L.add(C + 1)                  # b: ends at offset 1
    L.add(2 * C - 1)              # c: from offset 1 to a boundary, 2 pieces
    L.add(C + 1)                  # d: tail of 1 slot in the next chunk,
    L.add(1)                      #    a row inside it,
    L.add(C)                      #    the head of a spanning row (C - 2 here, 2 in the next)
    L.to_offset(C - 1)            # e
    L.add(1)
    L.add(2)
    for P in edge_P(G, T):        # f
        L.to_offset(0)
        L.spanning(P, 1 + P % C)
        L.to_offset(1 + P % (C - 1))
        L.spanning(P, C if P % 2 else 1 + (P + 1) % C)
    if G > 1:                     # g
        L.to_ordinal(0 if G <= 4 else 1, G)
        L.spanning(T + 1, 3)
        if G >= 4:
            L.add(1)
            L.spanning(2 if G == 4 else T, 2)
        L.spanning(2 * T + 3, C)
        assert (L.U - 1) // G == (L.U - (4 if G >= 4 else 2)) // G
    L.add(3)
    if G > 1 and (L.U + 1) % G == 0:   # h
        L.add(1)
    L.spanning(2, 1)              # i: one slot into the last chunk
    assert L.pos % C != 0 and (G == 1 or L.U % G != 0)
    return L.runs


def tiny_layouts(C: int):
    """One row that is less than a chunk, a 1-slot row, and one row of C + 1."""
    return [[1], [C - 1], [C + 1]]


def long_runs(C: int, G: int, T: int, rows_before: int = 8192):
    """More than `rows_before` rows and slots (8192: the waves of the combine kernels' grid
    cap, one row each in seg_combine_kernel), with a 2..T-piece row and a row of more than T
    pieces at ordinals >= rows_before — reached only by the kernels' grid-stride loops."""
    L = _Runs(C)
    for i in range(rows_before):
        L.add(2 if i % 97 == 0 else 1)
    L.to_offset(1)
    L.spanning(3, 2)
    L.add(1)
    L.spanning(T + 2, C)
    L.add(1)
    L.spanning(2, 1)
    L.add(2)
    if G > 1 and L.U % G == 0:
        L.add(1)
    if L.pos % C == 0:
        L.add(1)
    return L.runs


def layout_cases(runs, C: int, G: int, T: int) -> dict:
    """{case letter: True / False} for the cases of edge_runs, found from the run lengths
    alone (off0, off1 and P per row), and 'f': the set of (P, starts on a boundary) present."""
    off0, off1, P = row_pieces(runs, C)
    U, S = len(runs), int(off1[-1])
    n = off1 - off0
    on = off0 % C == 0
    res = {}
    res["a"] = bool(((n == C) & on).any())
    res["b"] = bool(((n == C + 1) & on).any())
    res["c"] = bool(((~on) & (off1 % C == 0) & (P >= 2)).any())
    # d: rows u-1, u, u+1 with u inside one chunk, u-1 spanning and ending in that chunk, u+1
    # spanning and starting in it
    d = False
    for u in range(1, U - 1):
        ch = off0[u] // C
        d |= bool(P[u] == 1 and P[u - 1] >= 2 and (off1[u - 1] - 1) // C == ch and
                  off0[u - 1] // C < ch and P[u + 1] >= 2 and off0[u + 1] // C == ch)
    res["d"] = d
    res["e"] = bool(((n[:-1] == 1) & (off0[:-1] % C == C - 1) & (off0[1:] % C == 0)).any())
    res["f"] = {(int(p), bool(b)) for p, b in zip(P, on) if p >= 2}
    g = False
    big = np.flatnonzero(P > T)
    for i, u in enumerate(big):
        for v in big[i + 1:]:
            if u // G != v // G:
                continue
            between = P[u + 1:v]
            g |= G < 4 or bool((between == 1).any() and ((between >= 2) & (between <= T)).any())
    res["g"] = g if G > 1 else True
    res["h"] = U % G != 0 if G > 1 else True
    res["i"] = bool(S % C != 0 and P[-1] >= 2)
    return res


def keys_from_runs(runs, seed: int):
    """(keys int64 [S], V): row u owns runs[u] slots. Row ids ascend with gaps (unique_rows[u]
    > u for every u) and the slots are dealt to the rows by a seeded permutation, so the
    plan's sorted_slots is no identity; rows above the last one stay unused."""
    rng = np.random.default_rng(seed)
    runs = np.asarray(runs, dtype=np.int64)
    rows = 1 + np.cumsum(rng.integers(1, 4, runs.size))
    keys = np.empty(int(runs.sum()), dtype=np.int64)
    keys[rng.permutation(keys.size)] = np.repeat(rows, runs)
    return keys, int(rows[-1]) + 3


def plan_of(keys):
    """(sorted_slots, unique_rows, seg_offsets) of the sparse plan of keys: the stable sort."""
    keys = np.asarray(keys)
    order = np.argsort(keys, kind="stable")
    rows, counts = np.unique(keys, return_counts=True)
    return order, rows, np.concatenate([[0], np.cumsum(counts)])


# ------------------------------------------------------------------- inputs ----------
def int_seg_inputs(S: int, K: int, F: int, V: int, seed: int) -> dict:
    """Integer-valued fp32 inputs of both modes: vals, d, e in [-4, 4], s in [-8, 8], g in
    [-2, 2] (B = ceil(S / F) examples, slot s belonging to example s // F)."""
    rng = np.random.default_rng(seed)
    B = -(-S // F)
    i = lambda lo, hi, *shape: rng.integers(lo, hi + 1, shape).astype(F32)  # noqa: E731
    return dict(vals=i(-4, 4, S, K), vals_lin=i(-4, 4, S), dx=i(-4, 4, S, K), emb=i(-4, 4, V, K),
                sum_e=i(-8, 8, B, K), gz=i(-2, 2, B))


def float_seg_inputs(S: int, K: int, F: int, V: int, seed: int) -> dict:
    """Normal fp32 inputs of both modes, of the sizes a training step meets."""
    rng = np.random.default_rng(seed)
    B = -(-S // F)
    n = lambda scale, *shape: (scale * rng.standard_normal(shape)).astype(F32)  # noqa: E731
    return dict(vals=n(1.0, S, K), vals_lin=n(1.0, S), dx=n(0.01, S, K), emb=n(0.1, V, K),
                sum_e=n(0.5, B, K), gz=n(0.02, B))


def int_fm_inputs(B: int, F: int, K: int, V: int, seed: int, dtype=np.int64) -> dict:
    """Integer-valued FM tables: e in [-2, 2], lin and bias in [-4, 4]; ids over all of V."""
    rng = np.random.default_rng(seed)
    return dict(x=rng.integers(0, V, (B, F)).astype(dtype),
                E=rng.integers(-2, 3, (V, K)).astype(F32),
                w=rng.integers(-4, 5, (V, 1)).astype(F32),
                b=rng.integers(-4, 5, 1).astype(F32))


def float_fm_inputs(B: int, F: int, K: int, V: int, seed: int, dtype=np.int64) -> dict:
    """Normal tables and labels. e ~ 0.3 / sqrt(F sqrt(K)) N and w ~ N / sqrt(F) keep the logits of
    order 1 up to K = 260, F = 65 — with F > V an example holds a row several times, and
    every such pair adds |e|^2 to z — so p, loss_elem and gz stay away from saturation."""
    rng = np.random.default_rng(seed)
    return dict(x=rng.integers(0, V, (B, F)).astype(dtype),
                E=(0.3 / np.sqrt(F * np.sqrt(K)) * rng.standard_normal((V, K))).astype(F32),
                w=(rng.standard_normal((V, 1)) / np.sqrt(F)).astype(F32),
                b=np.array([0.05], F32),
                y=(rng.random(B) < 0.3).astype(F32))


# ------------------------------------------------------------ segmented sums ---------
def _seg_terms64(keys, *, vals=None, vals_lin=None, F=None, gz=None, sum_e=None, emb=None,
                 dx=None):
    """Per-slot float64 (term [S, K], |summands| [S, K], linear term [S] or None)."""
    keys = np.asarray(keys, dtype=np.int64)
    S = keys.size
    if vals is not None:
        t = np.asarray(vals, dtype=np.float64)[:S]
        tl = None if vals_lin is None else np.asarray(vals_lin, dtype=np.float64)[:S]
        return t, np.abs(t), tl
    b = np.arange(S) // int(F)
    g = np.asarray(gz, dtype=np.float64)[b, None]
    s = np.asarray(sum_e, dtype=np.float64)[b]
    e = np.asarray(emb, dtype=np.float64)[keys]
    d = np.zeros_like(s) if dx is None else np.asarray(dx, dtype=np.float64)[:S]
    return g * (s - e) + d, np.abs(g * s) + np.abs(g * e) + np.abs(d), g[:, 0]


def seg_sums_f64(keys, **inputs) -> dict:
    """The per-row sums of a segmented row sum in float64, in plan (ascending row) order.

    vals mode (vals [S, K], vals_lin [S] or None): row r's sum of vals[slot] over its slots.
    FM mode (F, gz [B], sum_e [B, K], emb [V, K], dx [S, K] or None): the sum of
    g * (s - e) + d with g = gz[slot // F], s = sum_e[slot // F], e = emb[r], d = dx[slot];
    the linear sum is that of g.

    Returns rows [U], sums [U, K], cond [U, K] (the L1 norm of the summands: |vals|, or
    |g s| + |g e| + |d| — the `cond` of conftest.assert_grad_close), lin / cond_lin [U]
    (None without a linear term) and counts [U]."""
    keys = np.asarray(keys, dtype=np.int64)
    t, mag, tl = _seg_terms64(keys, **inputs)
    rows, inv, counts = np.unique(keys, return_inverse=True, return_counts=True)
    sums, cond = np.zeros((rows.size, t.shape[1])), np.zeros((rows.size, t.shape[1]))
    np.add.at(sums, inv, t)
    np.add.at(cond, inv, mag)
    lin = cond_lin = None
    if tl is not None:
        lin, cond_lin = np.zeros(rows.size), np.zeros(rows.size)
        np.add.at(lin, inv, tl)
        np.add.at(cond_lin, inv, np.abs(tl))
    return dict(rows=rows, sums=sums, cond=cond, lin=lin, cond_lin=cond_lin, counts=counts)


def _tree32(pieces, G):
    """pieces [P, ...] fp32 in chunk order -> their sum as the kernels form it: accumulator
    s of G the running fp32 sum, from zero, of pieces s, s + G, ...; then the pairwise tree
    over the accumulators in index order."""
    acc = np.zeros((G,) + pieces.shape[1:], F32)
    for i in range(pieces.shape[0]):
        acc[i % G] = acc[i % G] + pieces[i]
    w = 1
    while w < G:
        for s in range(0, G - w, 2 * w):
            acc[s] = acc[s] + acc[s + w]
        w *= 2
    return acc[0]


def seg_sums_f32_tree(keys, C: int, G: int, *, vals=None, vals_lin=None, F=None, gz=None,
                      sum_e=None, emb=None, dx=None):
    """(sums fp32 [U, K], lin fp32 [U] or None): the summation order csrc/sparse_grad.hip
    documents, emulated in fp32.

    The sorted positions (stable sort by row) are cut into chunks of C. Inside a chunk a row's
    slots are added sequentially in slot order, from zero. In FM mode a slot contributes
    fl(fl(g * s) + d) (d = 0 without dx) and g to the linear sum. A row inside one chunk is
    that sum; a row spanning P > 1 chunks is _tree32 of its P chunk sums over G accumulators,
    the linear sum alike. FM mode then subtracts the row term once, where the row completes:
    fl(acc - fl(c * e)) with c the row's fp32 linear sum."""
    keys = np.asarray(keys, dtype=np.int64)
    order, rows, off = plan_of(keys)
    S = keys.size
    fm = vals is None
    if fm:
        b = order // int(F)
        g = np.asarray(gz, F32)[b]
        term = (g[:, None] * np.asarray(sum_e, F32)[b]).astype(F32)
        if dx is not None:
            term = (term + np.asarray(dx, F32)[order]).astype(F32)
        tl = g
    else:
        term = np.asarray(vals, F32)[order]
        tl = None if vals_lin is None else np.asarray(vals_lin, F32)[order]
    K = term.shape[1]
    has_lin = tl is not None
    if not has_lin:
        tl = np.zeros(S, F32)
    sums, lin = np.zeros((rows.size, K), F32), np.zeros(rows.size, F32)
    for u in range(rows.size):
        pieces, pl = [], []
        for ch in range(off[u] // C, (off[u + 1] - 1) // C + 1):
            acc, accl = np.zeros(K, F32), F32(0)
            for pos in range(max(off[u], ch * C), min(off[u + 1], (ch + 1) * C)):
                acc = acc + term[pos]
                accl = F32(accl + tl[pos])
            pieces.append(acc)
            pl.append(accl)
        if len(pieces) == 1:
            sums[u], lin[u] = pieces[0], pl[0]
        else:
            sums[u] = _tree32(np.stack(pieces), G)
            lin[u] = _tree32(np.asarray(pl, F32), G)
    if fm:
        e = np.asarray(emb, F32)[rows]
        sums = (sums - (lin[:, None] * e).astype(F32)).astype(F32)
    return sums, (lin if has_lin else None)


def seq_sums_f32(keys, vals):
    """fp32 [U, K]: every row's vals added sequentially in slot order, from zero."""
    order, rows, off = plan_of(keys)
    v = np.asarray(vals, F32)[order]
    out = np.zeros((rows.size, v.shape[1]), F32)
    for u in range(rows.size):
        for pos in range(off[u], off[u + 1]):
            out[u] = out[u] + v[pos]
    return out


# ---------------------------------------------------------------- FM forward ---------
def fm_forward_f64(x, E, w, b, y=None, mean_div=None) -> dict:
    """The FM forward (p_model.py:40-55) in float64: z = bias + sum_f w[x_f] + 0.5 * sum_k
    ((sum_f e)^2 - sum_f e^2), sum_e [B, K], p = sigmoid(z) and, with labels, the BCE head:
    bce_f64's loss_elem and gz (mean_div = B by default). `mag` is the L1 norm of the summands
    of z (0.5 * sum_k (s_k^2 + q_k) + sum_f |w| + |bias|), the scale of z's rounding error."""
    x = np.asarray(x).astype(np.int64)
    e = np.asarray(E, dtype=np.float64)[x]                       # [B, F, K]
    wl = np.asarray(w, dtype=np.float64).reshape(-1)[x]          # [B, F]
    bias = float(np.asarray(b, dtype=np.float64).reshape(-1)[0])
    s, q = e.sum(1), (e * e).sum(1)
    z = bias + wl.sum(1) + 0.5 * (s * s - q).sum(1)
    out = dict(z=z, sum_e=s, emb=e.reshape(x.shape[0], -1),
               mag=0.5 * (s * s + q).sum(1) + np.abs(wl).sum(1) + abs(bias),
               p=1.0 / (1.0 + np.exp(-z)))
    if y is not None:
        out.update(bce_f64(z, y, x.shape[0] if mean_div is None else mean_div))
    return out


def bce_f64(z, y, mean_div) -> dict:
    """p, loss_elem and gz of the sigmoid + BCE(mean) head at logits z, in float64, by the
    formulas of torch's binary_cross_entropy and its backward (the logs clamped at -100, the
    denominator (1 - p) p at 1e-12): gz = (p - y) / mean_div unless p saturates, then 0."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    p = 1.0 / (1.0 + np.exp(-z))
    with np.errstate(divide="ignore"):
        loss = -(y * np.maximum(np.log(p), -100.0) + (1 - y) * np.maximum(np.log1p(-p), -100.0))
    g_p = (p - y) / np.maximum((1 - p) * p, 1e-12) / float(mean_div)
    return dict(p=p, loss_elem=loss, gz=g_p * (1 - p) * p)


def fm_forward_int(x, E, w, b) -> dict:
    """The FM forward of integer-valued tables in int64, exactly: z = bias + sum_f w[x_f] +
    sum_{f < f'} <e_f, e_f'> (half of sum_k (s_k^2 - q_k), which is even), sum_e, and
    `l1` = sum_k (s_k^2 + q_k) + sum_f |w| + |bias|: below 2^23 every partial sum of any fp32
    evaluation order is an integer fp32 holds exactly."""
    x = np.asarray(x).astype(np.int64)
    Ei, wi, bi = (np.asarray(a) for a in (E, w, b))
    assert all((a == np.round(a)).all() for a in (Ei, wi, bi)), "integer-valued tables only"
    e = Ei.astype(np.int64)[x]
    wl = wi.astype(np.int64).reshape(-1)[x]
    bias = int(bi.reshape(-1)[0])
    s, q = e.sum(1), (e * e).sum(1)
    ix = (s * s - q).sum(1)
    assert (ix % 2 == 0).all()
    return dict(z=bias + wl.sum(1) + ix // 2, sum_e=s, emb=e.reshape(x.shape[0], -1),
                l1=(s * s + q).sum(1) + np.abs(wl).sum(1) + abs(bias))
