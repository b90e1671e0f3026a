"""Plain numpy references for the GEMM entry points' contract (include/ctr_hip.h:
ctr_gemm_f32_ex, ctr_gemm_planes, ctr_gemm_planes_lastcol) and the poisoned, strided
operand slabs their tests run in. Nothing here touches the library.

* hash_u32 / dropout_keep / drop_scale: the stateless dropout mask, in uint64 arithmetic
  (csrc/ctr_common.h hash_u32; the host's threshold and scale in ctr_gemm_f32_ex);
* epilogue_ref: the five epilogues on an fp64 accumulator, rounded to fp32 exactly where
  the kernels round (apply_epi, csrc/gemm_common.h);
* carve: an fp32 [rows, cols] view with row stride ld inside one flat buffer whose every
  other element is poison (NaN for inputs, 777.0 for outputs).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

EPI_NONE, EPI_BIAS, EPI_BIAS_RELU, EPI_BIAS_RELU_DROP, EPI_GRAD_MASK = range(5)
MASK64 = (1 << 64) - 1
SENTINEL = 777.0
HEAD = 64  # floats in front of every carved view


def splitmix64(seed: int, ctr) -> np.ndarray:
    """The (ctr + 1)-th output of the splitmix64 generator whose state starts at `seed`
    (uint64, wrapping): the state after ctr + 1 increments is seed + (ctr + 1) * gamma."""
    c = np.atleast_1d(np.asarray(ctr, dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = np.uint64(seed & MASK64) + np.uint64(0x9E3779B97F4A7C15) * (c + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z.reshape(np.shape(ctr))


def hash_u32(seed: int, ctr) -> np.ndarray:
    """csrc/ctr_common.h hash_u32: the high 32 bits of splitmix64(seed, ctr)."""
    return (splitmix64(seed, ctr) >> np.uint64(32)).astype(np.uint32)


def drop_threshold(p: float) -> int:
    """keep iff hash >= this: p as the fp32 the entry point receives, times 2^32 in double,
    clamped to 2^32 - 1, truncated (0.2 -> 858993472, not double 0.2's 858993459)."""
    return int(min(float(np.float32(p)) * 4294967296.0, 4294967295.0))


def drop_scale(p: float) -> np.float32:
    return np.float32(1.0 / (1.0 - float(np.float32(p))))


def dropout_keep(M: int, N: int, p: float, seed: int, offset: int, step=None) -> np.ndarray:
    """bool [M, N]: element (m, n) is kept iff
    hash_u32(seed, (offset + (step << 32) + m*N + n) mod 2^64) >= drop_threshold(p).
    The counter runs over the logical [M, N] matrix, whatever C's row stride is."""
    base = (int(offset) + ((int(step) & MASK64) << 32 if step is not None else 0)) & MASK64
    with np.errstate(over="ignore"):
        ctr = np.arange(M * N, dtype=np.uint64) + np.uint64(base)
    return (hash_u32(seed, ctr) >= np.uint32(drop_threshold(p))).reshape(M, N)


def epilogue_ref(acc64, epi, bias=None, aux=None, scale=1.0, keep=None, drop_scale=1.0):
    """apply_epi on an fp64 accumulator [M, N], as float32: the accumulator is rounded to
    fp32 first (the kernels accumulate in fp32), and every later operation is one fp32
    operation, formed here in fp64 and rounded once (exact for + and * of two fp32)."""
    acc = np.asarray(acc64, dtype=np.float64).astype(np.float32)
    if epi == EPI_NONE:
        return acc
    if epi == EPI_GRAD_MASK:
        v = (acc.astype(np.float64) * float(np.float32(scale))).astype(np.float32)
        return np.where(np.asarray(aux, dtype=np.float32) > 0, v, np.float32(0))
    v = (acc.astype(np.float64) + np.asarray(bias, dtype=np.float32).astype(np.float64)[None, :])
    v = v.astype(np.float32)
    if epi == EPI_BIAS:
        return v
    v = np.where(v > 0, v, np.float32(0))  # NaN and -0.0 become +0.0, as `v > 0.f ? v : 0.f`
    if epi == EPI_BIAS_RELU:
        return v
    assert epi == EPI_BIAS_RELU_DROP and keep is not None
    s = (v.astype(np.float64) * float(np.float32(drop_scale))).astype(np.float32)
    return np.where(keep, s, np.float32(0))


@dataclass
class Slab:
    view: torch.Tensor  # [rows, cols], row stride ld, starts HEAD + off floats into buf
    buf: torch.Tensor   # the flat allocation
    mask: torch.Tensor  # bool over buf: the view's elements
    fill: float
    ld: int

    def ptr(self) -> int:
        return self.view.data_ptr() if self.view.numel() else self.buf.data_ptr()

    def pad(self) -> torch.Tensor:
        """Everything outside the valid region, as one flat tensor."""
        return self.buf[~self.mask]

    def pad_intact(self) -> bool:
        p = self.pad()
        want = torch.full_like(p, self.fill)
        return bool(torch.equal(p, want)) if self.fill == self.fill else bool(p.isnan().all())


def carve(rows: int, cols: int, ld: int, off: int, dev, fill: float = float("nan"),
          values=None) -> Slab:
    """An fp32 [rows, cols] view with row stride ld >= cols that starts HEAD + off floats into
    a flat buffer filled with `fill` (NaN: an input, any use of out-of-extent data poisons C;
    SENTINEL: an output, any stray store shows). At least 64*ld + 64 floats follow the last
    valid element, so a reader that runs a whole k-tile past an operand stays inside this
    allocation. off % 4 != 0 puts the view off a 16-byte boundary."""
    assert ld >= cols and rows >= 0 and cols >= 0 and off >= 0
    span = (max(rows, 1) - 1) * ld + cols
    n = HEAD + off + span + 64 * ld + 64
    buf = torch.full((n,), fill, dtype=torch.float32, device=dev)
    start = HEAD + off
    view = buf[start:start + max(rows, 1) * ld].view(max(rows, 1), ld)[:rows, :cols]
    mask = torch.zeros(n, dtype=torch.bool, device=dev)
    mask[start:start + max(rows, 1) * ld].view(max(rows, 1), ld)[:rows, :cols] = True
    if values is not None:
        view.copy_(torch.as_tensor(values, dtype=torch.float32).to(dev))
    return Slab(view, buf, mask, fill, ld)
