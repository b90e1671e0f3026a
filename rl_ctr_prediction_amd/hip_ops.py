"""Tensor-level wrappers over the libctr_hip.so C ABI.

PyTorch only provides device memory and the current HIP stream here; every computation
is a kernel of libctr_hip.so. Inputs must already be on a ROCm device: a CPU tensor is
an error, never a silent fallback.
"""
from __future__ import annotations

import contextlib
import os
import ctypes
import threading
from dataclasses import dataclass

import torch

from ._lib import (CTR_EFLAG_CAPACITY, CTR_EFLAG_INDEX, CTR_ENSEMBLE_TIE_REWARDS, CTR_IDX_I32, CTR_IDX_I64, CTR_LABEL_F32,
                   CTR_LABEL_I32, CTR_LABEL_I64, EPI_BIAS, EPI_BIAS_RELU,
                   EPI_BIAS_RELU_DROP, EPI_GRAD_MASK, EPI_NONE, PlanesDesc, PlaneViewDesc, SparsePlan,
                   CtrHipError, GradEntry, lib)

__all__ = [
    "embedding_gather", "fm_forward", "fm_forward_planes", "bce_sigmoid", "deepfm_head", "gemm", "linear",
    "tensor_sum", "colsum", "transpose", "Planes", "split_planes", "gemm_planes", "SparsePlanBuffers", "fm_embedding_grad", "segment_sum_rows",
    "fm_embedding_grad_adam", "segment_sum_rows_adam",
    "rows_to_dense", "adam_dense", "fm_step_tail", "adam_embedding", "adam_scalars", "feature_embedding",
    "dcn_cross_forward", "dcn_cross_backward", "afm_forward", "afm_backward",
    "afm_head", "afm_step_seed",
    "wd_forward", "wd_embedding_grad", "wd_embedding_grad_adam",
    "AFM_BWD_MAX_BLOCKS",
    "lr_forward", "ensemble_preds", "ensemble_preds_ex", "per_store_step",
    "per_add", "per_update", "per_keys", "per_sample", "PER_STOCHASTIC", "PER_GREEDY", "PER_MAX_K",
    "metrics_workspace_bytes", "metrics_reset", "metrics_append", "metrics_auc", "METRICS_TILE",
    "METRICS_STATE_WORDS",
    "bn_forward", "bn_backward", "td3_noise", "td3_act", "td3_smooth", "td3_critic_loss",
    "SoftUpdateTable", "soft_update_multi", "TD3_NOISE_NONE", "TD3_NOISE_PTR", "TD3_NOISE_SEED",
    "TD3_MAX_A",
    "td3v10_uniform", "td3v10_heads", "td3v10_rank_mask", "td3v10_heads_backward",
    "clip_grad_norm_", "td3v10_add", "td3v10_store_seeded", "td3v10_keys", "td3v10_sample", "td3v10_update",
    "bn_eval_backward", "V10_ACT", "V10_PLAIN", "V10_RANDOM", "V10_BEST", "GRAD_CLIP_MAX_TENSORS",
    "AdamStepTable", "adam_deferred_rows", "adam_deferred_flush", "adam_deferred_catchup_ids",
    "step_begin", "step_end", "ids_add_", "shard_pack_ids", "shard_runs_copy",
    "softmax_rows", "pg_discount_norm", "pg_loss_grad", "pg_vt_mean", "pg_loss_grad_global", "check_index_error", "Workspace",
    "EPI_NONE", "EPI_BIAS", "EPI_BIAS_RELU", "EPI_BIAS_RELU_DROP", "EPI_GRAD_MASK",
]


# ----------------------------------------------------------------------- plumbing ----
class HostTensorError(RuntimeError, TypeError):
    """A host tensor where a kernel needs a device one: the RuntimeError every wrapper has
    always raised for it, and a TypeError (an argument of the wrong kind, refused before any
    launch) for callers that catch argument errors as TypeError / ValueError."""


def _dev(t: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor")
    if t.device.type != "cuda":
        raise HostTensorError(f"{name} is on {t.device}: the HIP hot path needs ROCm device "
                              "tensors (there is no CPU fallback)")
    return t


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    _dev(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _f32_rows(t: torch.Tensor, name: str) -> int:
    """A float32 [M, N] device matrix whose rows are contiguous (a column slice of a wider
    matrix is fine); returns its leading dimension."""
    _dev(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    M, N = t.shape
    if t.numel() == 0:
        return max(N, 1)
    if N > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must be contiguous")
    if M == 1:  # a single row's stride is arbitrary (torch keeps any value)
        return N
    if t.stride(0) < N:
        raise ValueError(f"{name}: row stride {t.stride(0)} < N = {N}")
    return t.stride(0)


def _p(t):
    return None if t is None else t.data_ptr()


_cuda_device = torch._C._cuda_getDevice
_raw_stream = torch._C._cuda_getCurrentRawStream
_cur_stream = torch._C._cuda_getCurrentStream


def _stream() -> int:
    """The current stream's HIP handle, without torch.cuda.current_stream()'s Python-level
    device lookup (~4 us a call: the host paces C2's steps)."""
    return _raw_stream(_cuda_device())


def current_stream() -> torch.cuda.Stream:
    """torch.cuda.current_stream() for the current device, minus its device-index lookup."""
    d = _cur_stream(_cuda_device())
    return torch.cuda.Stream(stream_id=d[0], device_index=d[1], device_type=d[2])


def _idx(t: torch.Tensor, name: str = "idx") -> tuple[torch.Tensor, int]:
    _dev(t, name)
    if t.dtype == torch.int64:
        it = CTR_IDX_I64
    elif t.dtype == torch.int32:
        it = CTR_IDX_I32
    else:
        raise TypeError(f"{name}: feature ids must be int64 or int32, got {t.dtype}")
    return t.contiguous(), it


class Workspace:
    """Grow-only scratch buffers of ONE owner, one per (device, stream) inside it: kernels
    on one stream are ordered, so consecutive ops of the owner can share a buffer. A buffer
    outgrown is retired, never freed: HIP graphs captured earlier still hold its address.

    Every trainer (and PolicyGradient) owns a Workspace and enters it (``with ws.scope():``)
    around the launches it enqueues or captures, so no captured graph references scratch
    that another object's launches also use — two objects' streams may share a HIP handle
    (torch hands streams out of a small pool round-robin) without sharing scratch. Calls
    made outside any scope (one-off op calls, tests) use the process-wide default owner."""

    _default: "Workspace | None" = None
    _tls = threading.local()

    def __init__(self):
        self._pool: dict = {}
        self._retired: list = []

    @contextlib.contextmanager
    def scope(self):
        stack = getattr(Workspace._tls, "stack", None)
        if stack is None:
            stack = Workspace._tls.stack = []
        stack.append(self)
        try:
            yield self
        finally:
            stack.pop()

    @classmethod
    def current(cls) -> "Workspace":
        stack = getattr(cls._tls, "stack", None)
        if stack:
            return stack[-1]
        if cls._default is None:
            cls._default = Workspace()
        return cls._default

    def buffer(self, nbytes: int, device: torch.device) -> torch.Tensor | None:
        if nbytes <= 0:
            return None
        key = (device.index, _stream())
        buf = self._pool.get(key)
        if buf is None or buf.numel() < nbytes:
            if buf is not None:
                self._retired.append(buf)
            buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            self._pool[key] = buf
        return buf

    def buffers(self) -> list:
        """Every buffer this owner holds (tests: owners never share one)."""
        return list(self._pool.values()) + list(self._retired)

    @classmethod
    def get(cls, nbytes: int, device: torch.device) -> torch.Tensor | None:
        """Scratch of nbytes on the current stream, from the current owner."""
        return cls.current().buffer(nbytes, device)


def check_index_error(err_flag: torch.Tensor) -> None:
    """Raise like nn.Embedding does when a kernel saw an id outside [0, V). Syncs."""
    v = int(err_flag.item())
    if v & CTR_EFLAG_CAPACITY:  # a library invariant broke (the host sizes the capacity)
        err_flag.zero_()
        raise RuntimeError("row-sharded exchange: a run exceeded its capacity")
    if v & CTR_EFLAG_INDEX:
        err_flag.zero_()
        raise IndexError("index out of range in self")


# ------------------------------------------------------------------------ forward ----
def embedding_gather(table: torch.Tensor, idx: torch.Tensor, err_flag=None,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    _f32(table, "table")
    idx, it = _idx(idx)
    V, K = table.shape
    if out is None:
        out = torch.empty(*idx.shape, K, dtype=torch.float32, device=table.device)
    elif out.numel() < idx.numel() * K or not out.is_contiguous():
        raise ValueError("embedding_gather: out must be contiguous with idx.numel() * K floats")
    lib.ctr_embedding_gather(_p(table), V, K, _p(idx), it, idx.numel(), _p(out), _p(err_flag),
                             _stream())
    return out


@dataclass
class FMForward:
    z: torch.Tensor
    sum_e: torch.Tensor | None
    emb_out: torch.Tensor | None
    p: torch.Tensor | None
    loss_elem: torch.Tensor | None
    gz: torch.Tensor | None


def fm_forward(idx: torch.Tensor, emb: torch.Tensor, lin: torch.Tensor, bias: torch.Tensor, *,
               want_sum: bool = True, want_emb: bool = False, labels: torch.Tensor | None = None,
               mean_div: float | None = None, want_p: bool = True, err_flag=None,
               out: FMForward | None = None) -> FMForward:
    """Fused gather + FM second order + linear term (+ BCE head when labels are given)."""
    idx, it = _idx(idx)
    B, F = idx.shape
    _f32(emb, "feature_embedding.weight")
    _f32(lin, "linear.weight")
    _f32(bias, "bias")
    V, K = emb.shape
    dev = emb.device
    if out is None:
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        out = FMForward(z=e(B), sum_e=e(B, K) if want_sum else None,
                        emb_out=e(B, F * K) if want_emb else None,
                        p=e(B) if want_p else None,
                        loss_elem=e(B) if labels is not None else None,
                        gz=e(B) if labels is not None else None)
    if labels is not None:
        _f32(labels, "labels")
        mean_div = float(B if mean_div is None else mean_div)
    lib.ctr_fm_forward(_p(idx), it, B, F, K, V, _p(emb), _p(lin), _p(bias), _p(out.z),
                       _p(out.sum_e), _p(out.emb_out), _p(labels), float(mean_div or 1.0),
                       _p(out.p), _p(out.loss_elem), _p(out.gz), _p(err_flag), _stream())
    return out


def lr_forward(idx: torch.Tensor, lin: torch.Tensor, bias: torch.Tensor, *,
               labels: torch.Tensor | None = None, mean_div: float | None = None,
               want_p: bool = True, err_flag=None) -> dict:
    """LR (p_model.py:18-26): z = bias + sum_f lin[x_f] in field order and p = sigmoid(z), with
    the BCE head (loss_elem, gz) when labels are given: dict(z, p, loss_elem, gz), one launch."""
    idx, it = _idx(idx)
    if idx.dim() != 2:
        raise ValueError("lr_forward: idx must be [B, F]")
    B, F = idx.shape
    if not 1 <= F <= 64:
        raise ValueError(f"lr_forward: F={F} outside [1, 64]")
    _f32(lin, "linear.weight")
    _f32(bias, "bias")
    if lin.dim() != 2 or lin.shape[1] != 1 or bias.numel() != 1:
        raise ValueError("lr_forward: linear.weight must be [V, 1] and bias [1]")
    V, dev = lin.shape[0], lin.device
    e = lambda: torch.empty(B, dtype=torch.float32, device=dev)  # noqa: E731
    out = dict(z=e(), p=e() if want_p else None, loss_elem=None, gz=None)
    if labels is not None:
        _f32(labels, "labels")
        if labels.numel() != B:
            raise ValueError(f"lr_forward: labels must hold {B} values")
        mean_div = float(B if mean_div is None else mean_div)
        out["loss_elem"], out["gz"] = e(), e()
    lib.ctr_lr_forward(_p(idx), it, B, F, V, _p(lin), _p(bias), _p(out["z"]), _p(out["p"]),
                       _p(labels), float(mean_div or 1.0), _p(out["loss_elem"]), _p(out["gz"]),
                       _p(err_flag), _stream())
    return out


def fm_forward_planes(idx: torch.Tensor, emb: torch.Tensor, lin: torch.Tensor,
                      bias: torch.Tensor, x_planes: "Planes", z: torch.Tensor,
                      sum_e: torch.Tensor, err_flag=None) -> None:
    """DeepFM's FM part (z, sum_e) with the flattened embeddings written as the MLP input's
    three bf16 planes (no fp32 copy): ctr_fm_forward_planes."""
    idx, it = _idx(idx)
    B, F = idx.shape
    _f32(emb, "feature_embedding.weight")
    _f32(lin, "linear.weight")
    V, K = emb.shape
    if (x_planes.rows, x_planes.cols) != (B, F * K):
        raise ValueError(f"fm_forward_planes: planes must be [{B}, {F * K}]")
    lib.ctr_fm_forward_planes(_p(idx), it, B, F, K, V, _p(emb), _p(lin), _p(bias), _p(z),
                              _p(sum_e), x_planes.desc, _p(err_flag), _stream())


def fm_forward_planes_ok(K: int, F: int) -> bool:
    return K % 4 == 0 and 64 % (K // 4 or 1) == 0 and K <= 256 and F <= 64


def bce_sigmoid(z: torch.Tensor, labels: torch.Tensor, mean_div: float | None = None):
    _f32(z, "z")
    _f32(labels, "labels")
    B = z.numel()
    p, loss, gz = (torch.empty_like(z) for _ in range(3))
    lib.ctr_bce_sigmoid(_p(z), _p(labels), B, float(B if mean_div is None else mean_div), _p(p),
                        _p(loss), _p(gz), _stream())
    return p, loss, gz


def deepfm_head(h, w_out, b_out, z_fm, labels=None, mean_div=None, drop_scale=1.0, out=None,
                dh_planes: "Planes | None" = None):
    """dh_planes: also write dh_pre as its three bf16 planes (ctr_deepfm_head_planes)."""
    _f32(h, "h")
    B, H = h.shape
    dev = h.device
    if out is None:
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        out = dict(z=e(B), p=e(B), loss_elem=e(B) if labels is not None else None,
                   gz=e(B) if labels is not None else None,
                   dh_pre=e(B, H) if labels is not None else None)
    if dh_planes is not None:
        if labels is None or (dh_planes.rows, dh_planes.cols) != (B, H):
            raise ValueError(f"deepfm_head: dh_planes needs labels and [{B}, {H}] planes")
        lib.ctr_deepfm_head_planes(_p(h), B, H, _p(w_out), _p(b_out), _p(z_fm), _p(labels),
                                   float(B if mean_div is None else mean_div), float(drop_scale),
                                   _p(out["z"]), _p(out["p"]), _p(out["loss_elem"]),
                                   _p(out["gz"]), _p(out["dh_pre"]), dh_planes.desc, _stream())
        return out
    lib.ctr_deepfm_head(_p(h), B, H, _p(w_out), _p(b_out), _p(z_fm), _p(labels),
                        float(B if mean_div is None else mean_div), float(drop_scale),
                        _p(out["z"]), _p(out["p"]), _p(out["loss_elem"]), _p(out["gz"]),
                        _p(out["dh_pre"]), _stream())
    return out


# --------------------------------------------------------------------------- GEMM ----
GEMM_AUTO, GEMM_EXACT_F32, GEMM_SPLIT_BF16 = 0, 1, 2  # enum ctr_gemm_algo


def gemm(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False, *,
         epi: int = EPI_NONE, bias=None, aux=None, scale: float = 1.0, drop_p: float = 0.0,
         seed: int = 0, offset: int = 0, step_dev: torch.Tensor | None = None,
         out: torch.Tensor | None = None, algo: int = GEMM_AUTO) -> torch.Tensor:
    """C = op(a) @ op(b) on the MFMA units with a fused epilogue (see include/ctr_hip.h):
    algo GEMM_EXACT_F32 (fp32 MFMA) or GEMM_SPLIT_BF16 (three-plane bf16 split, fp32
    accurate); GEMM_AUTO = the library default. step_dev (device int32): the dropout stream
    of that step (offset += step << 32)."""
    _f32(a, "A")
    _f32(b, "B")
    M, K = (a.shape[1], a.shape[0]) if trans_a else a.shape
    Kb, N = (b.shape[1], b.shape[0]) if trans_b else b.shape
    if K != Kb:
        raise ValueError(f"gemm: inner dims differ ({K} vs {Kb})")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    else:
        _f32(out, "out")
        if tuple(out.shape) != (M, N):
            raise ValueError("gemm: bad out shape")
    if aux is not None:
        _f32(aux, "aux")
    nbytes = lib.ctr_gemm_f32_ex_workspace_bytes(int(algo), int(trans_a), int(trans_b), M, N, K)
    ws = Workspace.get(nbytes, a.device)
    lib.ctr_gemm_f32_ex(int(algo), int(trans_a), int(trans_b), M, N, K, _p(a), a.stride(0), _p(b),
                        b.stride(0), _p(out), out.stride(0), int(epi), _p(bias), _p(aux),
                        aux.stride(0) if aux is not None else 0, float(scale), float(drop_p),
                        int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), _p(step_dev), _p(ws),
                        0 if ws is None else ws.numel(), _stream())
    return out


class Planes:
    """An fp32 matrix [rows, cols] held as its exact three-plane bf16 split (ctr_planes):
    one bf16 tensor [3, rows_pad, cols_pad], both extents padded to multiples of 32 with
    zeros (allocated zeroed; producers write only the valid region, so the pad stays zero).
    x = x0 + (x1 + x2) recovers every fp32 element exactly (to_float)."""

    def __init__(self, rows: int, cols: int, device, pad: int = 32, ones_col: bool = False):
        self.rows, self.cols = int(rows), int(cols)
        self.rows_pad = -(-max(self.rows, 1) // pad) * pad
        self.cols_pad = -(-max(self.cols + int(ones_col), 1) // pad) * pad
        self.t = torch.zeros(3, self.rows_pad, self.cols_pad, dtype=torch.bfloat16, device=device)
        # ones_col: column `cols` (in the padding) holds 1.0 — exact in plane 0, zero in the
        # others — so a GEMM reading this matrix as B with N = cols + 1 also returns the
        # column sums of A (gemm_planes(last_col=...)); GEMMs with K = cols never read it.
        self.ones_col = bool(ones_col)
        if ones_col:
            self.t[0, :self.rows, self.cols] = 1.0
        self.desc = PlanesDesc(self.t.data_ptr(), self.cols_pad, self.rows_pad * self.cols_pad,
                               self.rows_pad, self.cols_pad)

    @property
    def device(self):
        return self.t.device

    def to_float(self) -> torch.Tensor:
        """The fp32 matrix (x0 + (x1 + x2), exact)."""
        p = self.t[:, :self.rows, :self.cols].float()
        return p[0] + (p[1] + p[2])


def split_planes(src: torch.Tensor, out: Planes | None = None) -> Planes:
    """The exact three-plane bf16 split of an fp32 [rows, cols] matrix (row-contiguous)."""
    _dev(src, "src")
    if src.dtype != torch.float32 or src.dim() != 2 or (src.numel() and src.stride(1) != 1):
        raise ValueError("split_planes: src must be a float32 [rows, cols] row-contiguous matrix")
    R, Cn = src.shape
    if out is None:
        out = Planes(R, Cn, src.device)
    elif out.rows != R or out.cols != Cn:
        raise ValueError(f"split_planes: out planes are [{out.rows}, {out.cols}], src [{R}, {Cn}]")
    lib.ctr_split_planes(_p(src), R, Cn, src.stride(0) if R > 1 else Cn, out.desc, _stream())
    return out


def gemm_planes(a: Planes, b: Planes, a_rc: bool, b_rc: bool, *, out: torch.Tensor | None = None,
                out_planes: Planes | None = None, epi: int = EPI_NONE, bias=None, aux=None,
                scale: float = 1.0, drop_p: float = 0.0, seed: int = 0, offset: int = 0,
                step_dev: torch.Tensor | None = None,
                last_col: torch.Tensor | None = None) -> torch.Tensor | None:
    """C = A.B on pre-split planes (ctr_gemm_planes). a_rc: A holds A^T ([K, M]); b_rc: B holds
    B itself ([K, N]) rather than the nn.Linear form [N, K]. Writes `out` (fp32 [M, N]) and/or
    `out_planes` (the planes of the epilogue's result).
    last_col ([M]): B (b_rc, built with ones_col) gets its ones column appended, and the
    extra result column — the row sums of A^T's rows, i.e. colsum of the stored A — lands
    here (ctr_gemm_planes_lastcol)."""
    M, K = (a.cols, a.rows) if a_rc else (a.rows, a.cols)
    N, Kb = (b.cols, b.rows) if b_rc else (b.rows, b.cols)
    if K != Kb:
        raise ValueError(f"gemm_planes: inner dims differ ({K} vs {Kb})")
    if last_col is not None:
        _f32(last_col, "last_col")
        if not (b_rc and b.ones_col) or out is None or out_planes is not None:
            raise ValueError("gemm_planes: last_col needs b_rc planes with ones_col and an fp32 out")
        if last_col.numel() != M or not last_col.is_contiguous():
            raise ValueError(f"gemm_planes: last_col must be {M} contiguous floats")
        if tuple(out.shape) != (M, N) or (out.numel() and out.stride(1) != 1):
            raise ValueError(f"gemm_planes: out must be [{M}, {N}]")
        nbytes = lib.ctr_gemm_planes_workspace_bytes(int(a_rc), 1, M, N + 1, K)
        ws = Workspace.get(nbytes, a.device)
        lib.ctr_gemm_planes_lastcol(int(a_rc), 1, M, N + 1, K, a.desc, b.desc, _p(out),
                                    out.stride(0), None, int(epi), _p(bias), None, 0,
                                    float(scale), 0.0, 0, 0, None, _p(last_col), _p(ws),
                                    0 if ws is None else ws.numel(), _stream())
        return out
    if out is None and out_planes is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    if out is not None:
        _f32(out, "out")
        if tuple(out.shape) != (M, N):
            raise ValueError(f"gemm_planes: out must be [{M}, {N}]")
    if out_planes is not None and (out_planes.rows, out_planes.cols) != (M, N):
        raise ValueError(f"gemm_planes: out_planes must be [{M}, {N}]")
    if aux is not None:
        _f32(aux, "aux")
    nbytes = lib.ctr_gemm_planes_workspace_bytes(int(a_rc), int(b_rc), M, N, K)
    ws = Workspace.get(nbytes, a.device)
    lib.ctr_gemm_planes(int(a_rc), int(b_rc), M, N, K, a.desc, b.desc, _p(out),
                        out.stride(0) if out is not None else 0,
                        out_planes.desc if out_planes is not None else None, int(epi), _p(bias),
                        _p(aux), aux.stride(0) if aux is not None else 0, float(scale),
                        float(drop_p), int(seed) & (2**64 - 1), int(offset) & (2**64 - 1),
                        _p(step_dev), _p(ws), 0 if ws is None else ws.numel(), _stream())
    return out


def gemm_planes_config(a_rc: bool, b_rc: bool, M: int, N: int, K: int) -> dict:
    """The tiling ctr_gemm_planes picks for a shape (tuning / tests)."""
    import ctypes
    v = [ctypes.c_int(0) for _ in range(4)]
    lib.ctr_gemm_planes_config(int(a_rc), int(b_rc), M, N, K, *(ctypes.byref(x) for x in v))
    return dict(tile=v[0].value, splits=v[1].value, bm=v[2].value, bn=v[3].value)


def linear(x, weight, bias, *, relu=False, drop_p=0.0, seed=0, offset=0, step_dev=None, out=None):
    """nn.Linear (+ReLU +Dropout) forward: x @ weight.T + bias, fused epilogue."""
    if relu:
        epi = EPI_BIAS_RELU_DROP if drop_p > 0 else EPI_BIAS_RELU
    else:
        epi = EPI_BIAS
    return gemm(x, weight, False, True, epi=epi, bias=bias, drop_p=drop_p, seed=seed,
                offset=offset, step_dev=step_dev, out=out)


def tensor_sum(x: torch.Tensor, scale: float = 1.0, out=None) -> torch.Tensor:
    _f32(x, "x")
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = Workspace.get(lib.ctr_reduce_workspace_bytes(x.numel(), 1), x.device)
    lib.ctr_sum_f32(_p(x), x.numel(), float(scale), _p(out), _p(ws), ws.numel(), _stream())
    return out


def colsum_multi(jobs) -> None:
    """Several colsum() calls in one launch pair: jobs = [(X [M,N], row_w or None, out [N]
    [, scale])]; each out is bitwise what colsum(X, row_w, scale, out=out) writes."""
    from ._lib import ColsumJob
    arr = (ColsumJob * len(jobs))()
    for i, job in enumerate(jobs):
        X, row_w, out = job[:3]
        scale = float(job[3]) if len(job) > 3 else 1.0
        if X.dim() != 2 or out.numel() != X.shape[1]:
            raise ValueError("colsum_multi: X must be [M, N] and out N elements")
        ldx = _f32_rows(X, "X")
        arr[i] = ColsumJob(_p(X), X.shape[0], X.shape[1], ldx, _p(row_w), scale, _p(out))
    nbytes = lib.ctr_colsum_multi_workspace_bytes(len(jobs), arr)
    if nbytes < 0:  # refused (job count, a bad job): nothing is launched
        raise CtrHipError("ctr_colsum_multi_workspace_bytes failed: "
                          + lib.ctr_last_error().decode(errors="replace"))
    ws = Workspace.get(nbytes, jobs[0][0].device)
    lib.ctr_colsum_multi_f32(len(jobs), arr, _p(ws), ws.numel(), _stream())


def colsum(X: torch.Tensor, row_w: torch.Tensor | None = None, scale: float = 1.0,
           out=None) -> torch.Tensor:
    ldx = _f32_rows(X, "X")
    M, N = X.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=X.device)
    ws = Workspace.get(lib.ctr_reduce_workspace_bytes(M, N), X.device)
    lib.ctr_colsum_f32(_p(X), M, N, ldx, _p(row_w), float(scale), _p(out), _p(ws),
                       ws.numel(), _stream())
    return out


def transpose(src: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out[c, r] = src[r, c] (bit-exact; src rows may be strided, out contiguous)."""
    _dev(src, "src")
    if src.dtype != torch.float32:
        raise TypeError(f"src: expected float32, got {src.dtype}")
    R, Cn = src.shape
    if src.numel() and src.stride(1) != 1:
        raise ValueError("transpose: src rows must be contiguous")
    if R > 1 and src.stride(0) < Cn:  # a stride-0 / overlapping row view (x.expand(R, C))
        raise ValueError("transpose: src rows must not overlap (stride(0) >= columns)")
    if out is None:
        out = torch.empty(Cn, R, dtype=torch.float32, device=src.device)
    if tuple(out.shape) != (Cn, R) or (out.numel() and out.stride(1) != 1):
        raise ValueError(f"transpose: out must be a row-contiguous [{Cn}, {R}] tensor")
    lib.ctr_transpose_f32(_p(src), R, Cn, src.stride(0) if R > 1 else Cn, _p(out), max(out.stride(0), R),
                          _stream())
    return out


# ---------------------------------------------------------------- scatter-add -------
# CTR_PLAN_COLS=0: the LSD plan for [B, F] ids too (A/B)
_PLAN_COLS = os.environ.get("CTR_PLAN_COLS", "1") != "0"


class SparsePlanBuffers:
    """Device buffers of a ctr_sparse_plan for up to `capacity` slots."""

    def __init__(self, capacity: int, device: torch.device):
        self.capacity = int(capacity)
        self.device = device
        i32 = dict(dtype=torch.int32, device=device)
        c = max(self.capacity, 1)
        self.sorted_slots = torch.empty(c, **i32)
        self.sorted_rows = torch.empty(c, **i32)
        self.pos_seg = torch.empty(c, **i32)
        self.unique_rows = torch.empty(c, **i32)
        self.seg_offsets = torch.empty(c + 1, **i32)
        self.num_unique = torch.zeros(1, **i32)
        self.S = 0
        self._n_unique = None  # num_unique as the host last read it for the current build
        self._struct = SparsePlan()
        # the plan's own radix scratch (not the per-stream Workspace): plans are built on the
        # plan streams concurrently with steps, and their captured graphs replay there, so
        # their scratch must be private to the plan
        self._ws = None

    def struct(self, rows_are_segments: bool = False) -> SparsePlan:
        """The ctr_sparse_plan of these buffers. rows_are_segments: present each position's
        unique-row ordinal as its row (a table compacted in unique order, row sharding)."""
        s = self._struct
        s.S = self.S
        s.sorted_slots = _p(self.sorted_slots)
        s.sorted_rows = _p(self.pos_seg if rows_are_segments else self.sorted_rows)
        s.pos_seg, s.unique_rows = _p(self.pos_seg), _p(self.unique_rows)
        s.seg_offsets, s.num_unique = _p(self.seg_offsets), _p(self.num_unique)
        return s

    def build(self, idx: torch.Tensor, V: int, err_flag=None) -> "SparsePlanBuffers":
        """idx [B, F] (a batch: the column plan, ctr_sparse_plan_build_cols) or flat ids
        (the LSD plan); both give the same plan bit for bit."""
        F = int(idx.shape[1]) if idx.dim() == 2 and _PLAN_COLS else 0
        idx, it = _idx(idx)
        S = idx.numel()
        if S > self.capacity:
            raise ValueError(f"sparse plan: {S} slots > capacity {self.capacity}")
        self.S = S
        self._n_unique = None
        need = lib.ctr_sparse_plan_workspace_bytes(S, int(V))
        if need < 0:
            raise RuntimeError(lib.load().ctr_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("sparse plan: scratch grown inside a graph capture (build "
                                   "these buffers once eagerly first)")
            full = lib.ctr_sparse_plan_workspace_bytes(max(self.capacity, 1), int(V))
            self._ws = torch.empty(max(need, full, 256), dtype=torch.uint8, device=self.device)
        if F > 0:
            lib.ctr_sparse_plan_build_cols(_p(idx), it, int(V), F, self.struct(), _p(self._ws),
                                           self._ws.numel(), _p(err_flag), _stream())
        else:
            lib.ctr_sparse_plan_build(_p(idx), it, int(V), self.struct(), _p(self._ws),
                                      self._ws.numel(), _p(err_flag), _stream())
        return self

    def build_runs(self, ids: torch.Tensor, n_runs: int, n_rows: int,
                   mask: torch.Tensor) -> "SparsePlanBuffers":
        """The plan of an owner shard's received ids (ctr_sparse_plan_build_runs): n_runs <= 8
        ascending runs of equal length, each row at most once per run, padded with the spare
        row n_rows - 1; bit-identical to build(). mask: int32[ceil(n_rows / 4)] zeros (left
        zero)."""
        _dev(ids, "ids")
        S = ids.numel()
        if ids.dtype != torch.int32 or not ids.is_contiguous() or S % n_runs:
            raise ValueError("build_runs: ids must be contiguous int32, n_runs equal runs")
        if S > self.capacity:
            raise ValueError(f"sparse plan: {S} slots > capacity {self.capacity}")
        if mask.dtype != torch.int32 or mask.numel() < (n_rows + 3) // 4:
            raise ValueError("build_runs: mask must be int32[ceil(n_rows / 4)]")
        self.S = S
        self._n_unique = None
        need = lib.ctr_sparse_plan_runs_workspace_bytes(int(n_runs), S // n_runs, int(n_rows))
        if need < 0:
            raise RuntimeError(lib.load().ctr_last_error().decode())
        if self._ws is None or self._ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("sparse plan: scratch grown inside a graph capture")
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        lib.ctr_sparse_plan_build_runs(_p(ids), int(n_runs), S // n_runs, int(n_rows),
                                       self.struct(), _p(mask), _p(self._ws), self._ws.numel(),
                                       _stream())
        return self

    def num_unique_host(self) -> int:
        self._n_unique = int(self.num_unique.item())
        return self._n_unique

    def max_unique(self, V: int) -> int:
        """How many unique rows the plan can have, as far as the host knows without a sync:
        the count it last read for this build (num_unique_host), else min(S, V). (A plan
        rebuilt by a graph replay keeps the count read before; whoever sizes a buffer by the
        new count has read it, which refreshes this one.)"""
        return min(self.S, int(V)) if self._n_unique is None else self._n_unique

    def slot_to_unique(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """int32[S]: the unique-row ordinal of every slot."""
        if out is None:
            out = torch.empty(max(self.capacity, 1), dtype=torch.int32, device=self.device)
        lib.ctr_plan_slot_to_unique(self.struct(), _p(out), _stream())
        return out

    def shard_counts(self, shard_rows: int, n_shards: int, out: torch.Tensor | None = None,
                     max_out: torch.Tensor | None = None) -> torch.Tensor:
        """int64[n_shards]: unique rows owned by each shard (ids // shard_rows); max_out
        (int64[1], n_shards <= 15): their maximum, from the same launch."""
        if out is None:
            out = torch.empty(n_shards, dtype=torch.int64, device=self.device)
        if max_out is not None and (max_out.dtype != torch.int64 or max_out.numel() < 1):
            raise ValueError("shard_counts: max_out must be an int64 tensor")
        lib.ctr_plan_shard_counts_max(self.struct(), int(shard_rows), int(n_shards), _p(out),
                                      _p(max_out), _stream())
        return out


def shard_pack_ids(plan: SparsePlanBuffers, shard_rows: int, V: int, n_shards: int,
                   capacity: int, send: torch.Tensor, counts: torch.Tensor,
                   offsets: torch.Tensor, err_flag: torch.Tensor | None = None,
                   cyclic: bool = False) -> None:
    """The plan's unique rows, per owner shard, into the padded exchange layout
    send[j*capacity + i] (owner-local ids; the owner's spare row past each run); counts /
    offsets: int32[n_shards] (ctr_shard_pack_ids). cyclic: the plan was built over
    shard_permute_ids_ ids (each owner's spare row is then its cyclic row count)."""
    for t, n, k in ((send, "send", n_shards * capacity), (counts, "counts", n_shards),
                    (offsets, "offsets", n_shards)):
        _dev(t, n)
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < k:
            raise ValueError(f"shard_pack_ids: {n} must be contiguous int32 of >= {k}")
    lib.ctr_shard_pack_ids_layout(plan.struct(), int(shard_rows), int(V), int(n_shards),
                                  int(bool(cyclic)), int(capacity), _p(send), _p(counts),
                                  _p(offsets), _p(err_flag), _stream())


def shard_permute_ids_(ids: torch.Tensor, V: int, n_shards: int, shard_rows: int,
                       err_flag: torch.Tensor | None = None) -> torch.Tensor:
    """In place: global row ids r -> (r % n_shards) * shard_rows + r // n_shards, the cyclic
    row-sharding space in which shard j's rows are one block (ctr_shard_permute_ids); ids
    outside [0, V) raise CTR_EFLAG_INDEX in err_flag and map to row 0. int64 or int32."""
    _dev(ids, "ids")
    if ids.dtype not in (torch.int64, torch.int32) or not ids.is_contiguous():
        raise TypeError("shard_permute_ids_: contiguous int64 / int32 ids expected")
    lib.ctr_shard_permute_ids(_p(ids), int(ids.dtype == torch.int64), ids.numel(), int(V),
                              int(n_shards), int(shard_rows), _p(err_flag), _stream())
    return ids


def cu_mask_words(n_cus: int, frac: float) -> list[int]:
    """A CU mask keeping q/8 of n_cus CUs (q = round(8 * frac), 1..8), every XCD its share
    whether the driver numbers CUs XCD by XCD (XCD = c // (n_cus / 8)) or round robin over
    the XCDs (XCD = c % 8): CU c is kept when (c % 8 + c // (n_cus / 8)) % 8 < q (exactly
    balanced when n_cus is a multiple of 64, as MI355X's 256)."""
    q = max(1, min(8, round(8 * frac)))
    per = max(1, n_cus // 8)
    words = [0] * ((n_cus + 31) // 32)
    for c in range(n_cus):
        if (c % 8 + c // per) % 8 < q:
            words[c // 32] |= 1 << (c % 32)
    return words


def cu_masked_stream(words: list[int], device=None) -> torch.cuda.ExternalStream:
    """A torch stream over a HIP stream whose kernels run only on the CUs set in `words`
    (ctr_stream_create_cu_masked). It lives as long as the process."""
    arr = (ctypes.c_uint32 * len(words))(*words)
    out = ctypes.c_void_p()
    lib.ctr_stream_create_cu_masked(ctypes.addressof(arr), len(words), ctypes.addressof(out))
    return torch.cuda.ExternalStream(out.value, device=device)


_STAGE_COPY = os.environ.get("CTR_STAGE_COPY", "1") != "0"  # A/B: the runtime's copies


def batch_stage_copy(ids_dst: torch.Tensor, ids_src: torch.Tensor,
                     y_dst: torch.Tensor | None = None, y_src: torch.Tensor | None = None) -> bool:
    """Copy a batch's ids (and labels) into its input slot in one launch
    (ctr_batch_stage_copy). Only for same-dtype, same-size, contiguous device tensors: returns
    False (nothing launched) otherwise, and the caller copies with torch."""
    if not _STAGE_COPY:
        return False
    pairs = [(ids_dst, ids_src)] + ([(y_dst, y_src)] if y_dst is not None else [])
    for d, s_ in pairs:
        if not (d.is_cuda and s_.is_cuda and d.dtype == s_.dtype and d.numel() == s_.numel()
                and d.is_contiguous() and s_.is_contiguous() and d.device == s_.device):
            return False
    n0 = ids_dst.numel() * ids_dst.element_size()
    n1 = y_dst.numel() * y_dst.element_size() if y_dst is not None else 0
    lib.ctr_batch_stage_copy(_p(ids_dst), _p(ids_src), n0, _p(y_dst) if n1 else None,
                             _p(y_src) if n1 else None, n1, _stream())
    return True


def shard_runs_copy(src: torch.Tensor, dst: torch.Tensor, capacity: int, counts: torch.Tensor,
                    offsets: torch.Tensor, pack: bool) -> torch.Tensor:
    """Rows between the compact order and the padded exchange layout (ctr_shard_runs_copy):
    pack: dst[j*capacity + i] = src[offsets[j] + i] (zeros past counts[j]); else the reverse
    for the runs only."""
    _f32(src, "src")
    _f32(dst, "dst")
    n = counts.numel()
    width = src.shape[1] if src.dim() == 2 else 1
    padded, compact = (dst, src) if pack else (src, dst)
    if padded.shape[0] < n * capacity or (dst.dim() == 2 and dst.shape[1] != width):
        raise ValueError("shard_runs_copy: padded side must hold n_shards * capacity rows")
    lib.ctr_shard_runs_copy(_p(src), _p(dst), int(width), int(capacity), int(n), _p(counts),
                            _p(offsets), int(bool(pack)), _stream())
    return dst


def rows_chunk(capacity: int, K: int, lin: bool) -> int:
    """Floats per (requester, owner) chunk of the rows + linear-weight exchange layout
    (ctr_shard_gather_rows / _rows_pack / _rows_unpack): capacity rows of K floats, then the
    capacity linear weights, padded to a multiple of 4."""
    return capacity * K + ((capacity + 3) // 4 * 4 if lin else 0)


def _rows_lin_check(name, chunked, n_shards, chunk, rows, K, lin):
    _f32(chunked, name)
    if chunked.numel() < n_shards * chunk:
        raise ValueError(f"{name}: needs n_shards * chunk = {n_shards * chunk} floats")
    _f32(rows, "rows")
    if rows.dim() != 2 or rows.shape[1] != K:
        raise ValueError(f"{name}: rows must be [*, {K}]")
    if lin is not None:
        _f32(lin, "lin")


def shard_gather_rows(emb: torch.Tensor, lin: torch.Tensor | None, ids: torch.Tensor,
                      n_shards: int, capacity: int, out: torch.Tensor) -> torch.Tensor:
    """Owner side: the requested rows and their linear weights into the chunked exchange
    layout (ctr_shard_gather_rows); ids int32[n_shards * capacity]."""
    K = emb.shape[1]
    chunk = rows_chunk(capacity, K, lin is not None)
    _rows_lin_check("shard_gather_rows", out, n_shards, chunk, emb, K, lin)
    _dev(ids, "ids")
    if ids.dtype != torch.int32 or ids.numel() < n_shards * capacity:
        raise ValueError("shard_gather_rows: ids must be int32 of n_shards * capacity")
    lib.ctr_shard_gather_rows(_p(emb), _p(lin), K, _p(ids), int(n_shards), int(capacity), chunk,
                              _p(out), _stream())
    return out


def shard_rows_pack(rows: torch.Tensor, lin: torch.Tensor | None, capacity: int,
                    counts: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Compact rows (+ linear values) -> the chunked exchange layout, zeros past each run
    (ctr_shard_rows_pack)."""
    n, K = counts.numel(), rows.shape[1]
    chunk = rows_chunk(capacity, K, lin is not None)
    _rows_lin_check("shard_rows_pack", out, n, chunk, rows, K, lin)
    lib.ctr_shard_rows_pack(_p(rows), _p(lin), K, int(capacity), chunk, n, _p(counts),
                            _p(offsets), _p(out), _stream())
    return out


def shard_rows_unpack(chunked: torch.Tensor, capacity: int, counts: torch.Tensor,
                      offsets: torch.Tensor, rows: torch.Tensor,
                      lin: torch.Tensor | None = None) -> torch.Tensor:
    """The chunked exchange layout -> compact rows (+ linear values), the runs only
    (ctr_shard_rows_unpack)."""
    n, K = counts.numel(), rows.shape[1]
    chunk = rows_chunk(capacity, K, lin is not None)
    _rows_lin_check("shard_rows_unpack", chunked, n, chunk, rows, K, lin)
    lib.ctr_shard_rows_unpack(_p(chunked), K, int(capacity), chunk, n, _p(counts), _p(offsets),
                              _p(rows), _p(lin), _stream())
    return rows


def ids_add_(ids: torch.Tensor, delta: int) -> torch.Tensor:
    """In place: ids += delta (int32 device ids)."""
    _dev(ids, "ids")
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        raise TypeError("ids_add_: contiguous int32 ids expected")
    lib.ctr_ids_add(_p(ids), ids.numel(), int(delta), _stream())
    return ids


def _seg_ws(plan: SparsePlanBuffers, K: int):
    return Workspace.get(lib.ctr_segment_workspace_bytes(max(plan.S, 1), K), plan.device)


def fm_embedding_grad(plan: SparsePlanBuffers, F: int, emb, gz, sum_e, dx=None, rowmap=None,
                      grad_rows=None, grad_lin=None, compact: bool = False):
    """Per-unique-row gradient sums. compact: `emb` holds the batch's unique rows in plan
    order (row sharding) instead of the whole table."""
    V, K = emb.shape
    cap = max(plan.capacity, 1)
    if grad_rows is None:
        grad_rows = torch.empty(cap, K, dtype=torch.float32, device=emb.device)
    if grad_lin is None:
        grad_lin = torch.empty(cap, dtype=torch.float32, device=emb.device)
    ws = _seg_ws(plan, K)
    lib.ctr_fm_embedding_grad(plan.struct(compact), int(F), int(K), _p(emb), _p(gz), _p(sum_e), _p(dx),
                              _p(grad_rows), _p(grad_lin), _p(rowmap), _p(ws), ws.numel(),
                              _stream())
    return grad_rows, grad_lin


def segment_sum_rows(plan: SparsePlanBuffers, vals, vals_lin=None, rowmap=None, out=None,
                     out_lin=None):
    K = vals.shape[1]
    cap = max(plan.capacity, 1)
    if out is None:
        out = torch.empty(cap, K, dtype=torch.float32, device=vals.device)
    if vals_lin is not None and out_lin is None:
        out_lin = torch.empty(cap, dtype=torch.float32, device=vals.device)
    ws = _seg_ws(plan, K)
    lib.ctr_segment_sum_rows(plan.struct(), int(K), _p(vals), _p(vals_lin), _p(out), _p(out_lin),
                             _p(rowmap), _p(ws), ws.numel(), _stream())
    return out, out_lin


def _i32(t, name: str, n: int) -> torch.Tensor:
    """A contiguous int32 device tensor of n elements (last / rowmap / owner / step counters):
    the kernels index it without a bound of their own."""
    _dev(t, name)
    if t.dtype != torch.int32:
        raise TypeError(f"{name}: expected int32, got {t.dtype}")
    if t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{name}: expected {n} contiguous int32 elements, got shape "
                         f"{tuple(t.shape)}")
    return t


def _adam_tables(emb, m_emb, v_emb, lin, m_lin, v_lin) -> tuple[int, int]:
    """The (parameter, exp_avg, exp_avg_sq) tables of an Adam kernel: contiguous float32
    device matrices, the moments of the parameter's shape; the linear table's three (V
    elements each, [V] or [V, 1]) all given or all None. Returns (V, K)."""
    _f32(emb, "emb")
    if emb.dim() != 2:
        raise ValueError(f"emb: expected a [V, K] table, got shape {tuple(emb.shape)}")
    for t, n in ((m_emb, "m_emb"), (v_emb, "v_emb")):
        if _f32(t, n).shape != emb.shape:
            raise ValueError(f"{n}: shape {tuple(t.shape)} != emb's {tuple(emb.shape)}")
    V, K = emb.shape
    if lin is None:
        if m_lin is not None or v_lin is not None:
            raise ValueError("lin, m_lin and v_lin must be all given or all None")
    else:
        for t, n in ((lin, "lin"), (m_lin, "m_lin"), (v_lin, "v_lin")):
            if _f32(t, n).numel() != V:
                raise ValueError(f"{n}: expected {V} elements, got shape {tuple(t.shape)}")
    return V, K


def _plan_grads(plan: "SparsePlanBuffers", V: int, K: int, grad_rows, grad_lin, lin,
                names=("grad_rows", "grad_lin")) -> None:
    """The per-row gradient buffers of a plan: float32, at least as many rows as the plan
    can have unique rows (SparsePlanBuffers.max_unique: num_unique lives on the device)."""
    n = plan.max_unique(V)
    if _f32(grad_rows, names[0]).numel() < n * K:
        raise ValueError(f"{names[0]}: {tuple(grad_rows.shape)} holds fewer than the plan's "
                         f"possible {n} rows of {K}")
    if grad_lin is not None:
        if _f32(grad_lin, names[1]).numel() < n:
            raise ValueError(f"{names[1]}: fewer than the plan's possible {n} rows")
    elif lin is not None:
        raise ValueError(f"{names[1]} is needed with a linear table")


def _deferred_table(emb, m_emb, v_emb, lin, m_lin, v_lin, last):
    from ._lib import DeferredTable
    V, _ = _adam_tables(emb, m_emb, v_emb, lin, m_lin, v_lin)
    _i32(last, "last", V)
    return DeferredTable(_p(emb), _p(m_emb), _p(v_emb), _p(lin), _p(m_lin), _p(v_lin), _p(last))


def shard_row_grads(plan: SparsePlanBuffers, capacity: int, offsets: torch.Tensor,
                    out: torch.Tensor, *, K: int, F: int = 0, emb=None, gz=None, sum_e=None,
                    dx=None, vals=None, lin: bool = False) -> torch.Tensor:
    """A row-sharded requester's per-row gradient sums written straight into the exchange
    chunks (ctr_shard_row_grads; the layout of shard_rows_pack): FM mode (gz: the FM / DeepFM
    slot gradients over the compact table emb) or vals mode (IPNN's per-slot gradients)."""
    _f32(out, "out")
    n = offsets.numel()
    chunk = rows_chunk(capacity, K, lin)
    if out.numel() < n * chunk:
        raise ValueError(f"shard_row_grads: out needs {n * chunk} floats")
    if offsets.dtype != torch.int32:
        raise TypeError("shard_row_grads: offsets must be int32")
    ws = _seg_ws(plan, K)
    lib.ctr_shard_row_grads(plan.struct(gz is not None), int(F), int(K), _p(emb), _p(gz),
                            _p(sum_e), _p(dx), _p(vals), int(bool(lin)), n, _p(offsets),
                            int(capacity), chunk, _p(out), _p(ws), ws.numel(), _stream())
    return out


def fm_embedding_grad_adam(plan: SparsePlanBuffers, F: int, gz, sum_e, dx, table, step_dev,
                           step_table: "AdamStepTable", step: int, betas=(0.9, 0.999), eps=1e-8,
                           weight_decay=0.0, grad_rows=None, grad_lin=None,
                           keep_sums: bool = False) -> None:
    """fm_embedding_grad + adam_deferred_rows(sums, step = *step_dev) with the apply fused
    into the combine pass (ctr_fm_embedding_grad_adam): table = (E, m_E, v_E, w, m_w, v_w,
    last); grad_rows / grad_lin are scratch, holding every row's sum with keep_sums."""
    dtab = _deferred_table(*table)
    V, K = table[0].shape
    _i32(step_dev, "step_dev", 1)
    if int(F) < 1:
        raise ValueError("fm_embedding_grad_adam: F must be >= 1")
    B = -(-plan.S // int(F))  # slot s belongs to example s // F
    if _f32(gz, "gz").numel() < B or _f32(sum_e, "sum_e").numel() < B * K:
        raise ValueError(f"fm_embedding_grad_adam: gz [B] and sum_e [B, {K}] must cover the "
                         f"plan's {plan.S} = B * F slots")
    if dx is not None and _f32(dx, "dx").numel() < plan.S * K:
        raise ValueError(f"fm_embedding_grad_adam: dx must be [{plan.S}, {K}]")
    if grad_lin is None:
        raise ValueError("fm_embedding_grad_adam: grad_rows and grad_lin are needed")
    _plan_grads(plan, V, K, grad_rows, grad_lin, table[3])
    ws = _seg_ws(plan, K)
    tab = step_table.ensure(step)
    lib.ctr_fm_embedding_grad_adam(plan.struct(), int(F), int(K), _p(gz), _p(sum_e), _p(dx),
                                   dtab, _p(step_dev), _p(tab),
                                   float(betas[0]), float(betas[1]), float(eps),
                                   float(weight_decay), _p(grad_rows), _p(grad_lin),
                                   int(keep_sums), _p(ws), ws.numel(), _stream())


def segment_sum_rows_adam(plan: SparsePlanBuffers, vals, vals_lin, table, step_dev,
                          step_table: "AdamStepTable", step: int, betas=(0.9, 0.999), eps=1e-8,
                          weight_decay=0.0, out=None, out_lin=None, keep_sums: bool = False) -> None:
    """segment_sum_rows + adam_deferred_rows in one pass (ctr_segment_sum_rows_adam)."""
    dtab = _deferred_table(*table)
    V, K = table[0].shape
    _i32(step_dev, "step_dev", 1)
    if _f32(vals, "vals").dim() != 2 or vals.shape[1] != K or vals.shape[0] < plan.S:
        raise ValueError(f"segment_sum_rows_adam: vals must be [>= {plan.S}, {K}], got "
                         f"{tuple(vals.shape)}")
    if vals_lin is not None and _f32(vals_lin, "vals_lin").numel() < plan.S:
        raise ValueError(f"segment_sum_rows_adam: vals_lin needs {plan.S} elements")
    if out is None or (vals_lin is None) != (out_lin is None):
        raise ValueError("segment_sum_rows_adam: out is needed, and out_lin exactly when "
                         "vals_lin is given")
    _plan_grads(plan, V, K, out, out_lin, None, names=("out", "out_lin"))
    ws = _seg_ws(plan, K)
    tab = step_table.ensure(step)
    lib.ctr_segment_sum_rows_adam(plan.struct(), int(K), _p(vals), _p(vals_lin),
                                  dtab, _p(step_dev), _p(tab),
                                  float(betas[0]), float(betas[1]), float(eps),
                                  float(weight_decay), _p(out), _p(out_lin), int(keep_sums),
                                  _p(ws), ws.numel(), _stream())


def rows_to_dense(plan: SparsePlanBuffers, V: int, grad_rows, grad_lin=None):
    K = grad_rows.shape[1]
    dense = torch.zeros(V, K, dtype=torch.float32, device=grad_rows.device)
    dense_lin = (torch.zeros(V, 1, dtype=torch.float32, device=grad_rows.device)
                 if grad_lin is not None else None)
    lib.ctr_rows_to_dense(plan.struct(), int(K), _p(grad_rows), _p(grad_lin), _p(dense),
                          _p(dense_lin), _stream())
    return dense, dense_lin


# --------------------------------------------------------------------------- Adam ----
def adam_scalars(step: int, lr: float, betas=(0.9, 0.999)) -> tuple[float, float]:
    """step_size and sqrt(bias_correction2) exactly as torch/optim/adam.py computes them
    (python doubles)."""
    beta1, beta2 = betas
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    return lr / bias_correction1, bias_correction2 ** 0.5


def _step_dev_ok(name: str, step_dev, table) -> None:
    """step_dev (optional): one int32 on the device, read by the kernel; it indexes the step
    table, so the table must be given with it."""
    if step_dev is None:
        return
    _i32(step_dev, "step_dev", 1)
    if table is None:
        raise ValueError(f"{name}: step_dev needs the step table")


def adam_dense(p, g, m, v, step: int, lr: float, betas=(0.9, 0.999), eps=1e-8,
               weight_decay=0.0, step_dev=None, table=None, planes=None) -> None:
    """One Adam step; with step_dev/table the step index is read on the device (graphs).
    planes: [(offset, Planes)] — sub-matrices p[offset : offset + rows*cols] (row-major,
    the Planes' shape) whose planes are rewritten with the updated values (ctr_adam_dense_planes)."""
    for t, n in ((p, "param"), (g, "grad"), (m, "exp_avg"), (v, "exp_avg_sq")):
        if _f32(t, n).numel() != p.numel():
            raise ValueError(f"adam_dense: {n} has shape {tuple(t.shape)}, param "
                             f"{tuple(p.shape)}")
    _step_dev_ok("adam_dense", step_dev, table)
    ss, bc2s = adam_scalars(max(step, 1), lr, betas)
    tab = table.ensure(step) if table is not None else None
    args = (_p(p), _p(g), _p(m), _p(v), p.numel(), ss, bc2s, _p(tab), _p(step_dev),
            float(betas[0]), float(betas[1]), float(eps), float(weight_decay))
    if not planes:
        lib.ctr_adam_dense(*args, _stream())
        return
    views = (PlaneViewDesc * len(planes))(
        *[PlaneViewDesc(int(off), pl.rows, pl.cols, pl.desc) for off, pl in planes])
    lib.ctr_adam_dense_planes(*args, ctypes.cast(views, ctypes.c_void_p), len(planes), _stream())


def adam_embedding(emb, m_emb, v_emb, lin, m_lin, v_lin, rowmap, grad_rows, grad_lin, step: int,
                   lr: float, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step_dev=None,
                   table=None) -> None:
    V, K = _adam_tables(emb, m_emb, v_emb, lin, m_lin, v_lin)
    _i32(rowmap, "rowmap", V)
    # rowmap's entries (device values) index grad_rows / grad_lin: only their kind is known here
    if _f32(grad_rows, "grad_rows").numel() % K:
        raise ValueError(f"adam_embedding: grad_rows must hold rows of {K}")
    if lin is not None:
        _f32(grad_lin, "grad_lin")
    _step_dev_ok("adam_embedding", step_dev, table)
    ss, bc2s = adam_scalars(max(step, 1), lr, betas)
    tab = table.ensure(step) if table is not None else None
    lib.ctr_adam_embedding(_p(emb), _p(m_emb), _p(v_emb), _p(lin), _p(m_lin), _p(v_lin), V, K,
                           _p(rowmap), _p(grad_rows), _p(grad_lin), ss, bc2s, _p(tab),
                           _p(step_dev), float(betas[0]), float(betas[1]), float(eps),
                           float(weight_decay), _stream())


class AdamStepTable:
    """Device table of the per-step Adam scalars for the deferred-exact path:
    tab[2t] = -lr/(1-beta1^t), tab[2t+1] = 1/sqrt(1-beta2^t), computed in python doubles
    exactly like adam_scalars() (so dense and deferred paths see identical fp32 values)."""

    def __init__(self, lr: float, betas, device, capacity: int = 4096):
        self.lr, self.betas, self.device = float(lr), tuple(betas), device
        self.capacity = 0
        self.version = 0  # bumped when the table moves (captured HIP graphs hold its address)
        self.tab = torch.zeros(2, dtype=torch.float32, device=device)
        self.ensure(capacity)

    def _host(self, cap: int) -> torch.Tensor:
        host = torch.zeros(2 * (cap + 1), dtype=torch.float64)
        for t in range(1, cap + 1):
            ss, bc2s = adam_scalars(t, self.lr, self.betas)
            host[2 * t] = -ss
            host[2 * t + 1] = 1.0 / bc2s
        return host.to(torch.float32)

    def ensure(self, step: int) -> torch.Tensor:
        if step > self.capacity:
            cap = max(step, 2 * self.capacity, 1024)
            self.tab = self._host(cap).to(self.device)
            self.capacity = cap
            self.version += 1
        return self.tab

    def set_lr(self, lr: float) -> None:
        """A new learning rate (the driver's `learning_rate += 1e-4` before each epoch's
        Adam): the values are rewritten IN PLACE, so captured HIP graphs, which hold the
        table's address, stay valid and read the new scalars at their next replay."""
        if float(lr) == self.lr:
            return
        self.lr = float(lr)
        self.tab.copy_(self._host(self.capacity), non_blocking=False)


def adam_deferred_rows(emb, m_emb, v_emb, lin, m_lin, v_lin, last, plan: "SparsePlanBuffers",
                       step: int, table: AdamStepTable, betas=(0.9, 0.999), eps=1e-8,
                       weight_decay=0.0, grad_rows=None, grad_lin=None, step_dev=None) -> None:
    """grad_rows None: bring the plan's rows to `step`; else to step-1 and apply `step`.
    step_dev (device int32): read the step there instead (graphs); `step` then only sizes
    the table."""
    V, K = _adam_tables(emb, m_emb, v_emb, lin, m_lin, v_lin)
    _i32(last, "last", V)
    if grad_rows is not None:
        _plan_grads(plan, V, K, grad_rows, grad_lin, lin)
    if step_dev is not None:
        _i32(step_dev, "step_dev", 1)
    tab = table.ensure(max(step, 1))
    lib.ctr_adam_deferred_rows(_p(emb), _p(m_emb), _p(v_emb), _p(lin), _p(m_lin), _p(v_lin), V, K,
                               _p(last), plan.struct(), _p(grad_rows), _p(grad_lin),
                               max(int(step), 1), _p(step_dev), _p(tab), float(betas[0]),
                               float(betas[1]), float(eps), float(weight_decay), _stream())


def adam_deferred_entries(emb, m_emb, v_emb, lin, m_lin, v_lin, last, plan: "SparsePlanBuffers",
                          vals: torch.Tensor, vals_lin: torch.Tensor | None, step: int,
                          table: AdamStepTable, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                          skip_row: int = -1, step_dev=None, out=None, out_lin=None,
                          run_len: int = 0) -> None:
    """The owner side of a row-sharded step in one launch (ctr_adam_deferred_entries): each
    unique row of `plan` (over the received entries) stepped with the sequential sum of its
    entries' vals / vals_lin; skip_row left alone. run_len > 0: vals is the chunked exchange
    buffer (shard_rows_pack's layout, rows_chunk(run_len, K, lin) floats per chunk)."""
    V, K = _adam_tables(emb, m_emb, v_emb, lin, m_lin, v_lin)
    _i32(last, "last", V)
    if step_dev is not None:
        _i32(step_dev, "step_dev", 1)
    _f32(vals, "vals")
    chunk =rows_chunk(run_len, K, lin is not None) if run_len else 0
    if run_len == 0 and (vals.dim() != 2 or vals.shape[1] != K):
        raise ValueError(f"adam_deferred_entries: vals must be [entries, {K}]")
    tab = table.ensure(max(step, 1))
    lib.ctr_adam_deferred_entries(_p(emb), _p(m_emb), _p(v_emb), _p(lin), _p(m_lin), _p(v_lin),
                                  V, K, _p(last), plan.struct(), _p(vals), _p(vals_lin),
                                  int(run_len), int(chunk), int(skip_row), max(int(step), 1),
                                  _p(step_dev), _p(tab),
                                  float(betas[0]), float(betas[1]), float(eps),
                                  float(weight_decay), _p(out), _p(out_lin), _stream())


def adam_deferred_catchup_ids(emb, m_emb, v_emb, lin, m_lin, v_lin, last, idx: torch.Tensor,
                              owner: torch.Tensor, step_dev: torch.Tensor, table: AdamStepTable,
                              step_hint: int, betas=(0.9, 0.999), eps=1e-8,
                              weight_decay=0.0) -> None:
    """Bring the rows of a batch's ids to the completed step held in step_dev (device int32),
    no sparse plan needed; owner is an int32[V] scratch. step_hint (>= the device value)
    sizes the step table."""
    V, K = _adam_tables(emb, m_emb, v_emb, lin, m_lin, v_lin)
    _i32(last, "last", V)
    _i32(owner, "owner", V)
    _i32(step_dev, "step_dev", 1)
    idx, it = _idx(idx)
    tab = table.ensure(max(step_hint, 1))
    lib.ctr_adam_deferred_catchup_ids(_p(emb), _p(m_emb), _p(v_emb), _p(lin), _p(m_lin), _p(v_lin),
                                      V, K, _p(last), _p(idx), it, idx.numel(), _p(owner),
                                      _p(step_dev), _p(tab), float(betas[0]), float(betas[1]),
                                      float(eps), float(weight_decay), _stream())


def step_begin(step_ctr: torch.Tensor) -> None:
    """ctr[1] = ctr[0] + 1 on the device (int32[2]: completed steps, step in flight)."""
    lib.ctr_step_begin(_p(step_ctr), _stream())


def step_end(step_ctr: torch.Tensor, loss: torch.Tensor | None = None,
             loss_sum: torch.Tensor | None = None) -> None:
    """ctr[0] = ctr[1] on the device; with loss / loss_sum (fp32 [1] / fp64 [1]) also
    loss_sum += loss in double (the driver's epoch loss, no host sync per step)."""
    if loss_sum is None:
        lib.ctr_step_end(_p(step_ctr), _stream())
        return
    _f32(loss, "loss")
    if loss_sum.dtype != torch.float64 or not loss_sum.is_cuda:
        raise TypeError("step_end: loss_sum must be a float64 device tensor")
    lib.ctr_step_end_loss(_p(step_ctr), _p(loss), _p(loss_sum), _stream())


def fm_step_tail(loss_elem: torch.Tensor, gz: torch.Tensor, loss_scale: float,
                 loss_out: torch.Tensor, bias_grad: torch.Tensor, p, g, m, v,
                 table: AdamStepTable, step: int, step_ctr: torch.Tensor, betas=(0.9, 0.999),
                 eps=1e-8, weight_decay=0.0, loss_sum: torch.Tensor | None = None) -> None:
    """The FM step's dense tail in one launch: loss_out = loss_scale * sum(loss_elem),
    bias_grad = sum(gz) (bitwise tensor_sum), the Adam step of the flat dense vector p at
    step ctr[1] (bitwise adam_dense), then step_end(step_ctr) (and loss_sum += loss_out
    in double when given)."""
    if loss_sum is not None and (loss_sum.dtype != torch.float64 or not loss_sum.is_cuda):
        raise TypeError("fm_step_tail: loss_sum must be a float64 device tensor")
    for t, n in ((loss_elem, "loss_elem"), (gz, "gz"), (p, "param"), (g, "grad"),
                 (m, "exp_avg"), (v, "exp_avg_sq")):
        _f32(t, n)
    B = gz.numel()
    if loss_elem.numel() != B or bias_grad.numel() != 1 or loss_out.numel() < 1:
        raise ValueError("fm_step_tail: loss_elem / gz of B elements, one bias gradient")
    if not (g.numel() == m.numel() == v.numel() == p.numel()):
        raise ValueError("fm_step_tail: p, g, m, v of one size")
    for t, n in ((loss_out, "loss_out"), (bias_grad, "bias_grad")):
        _f32(t, n)
    _i32(step_ctr, "step_ctr", 2)
    tab = table.ensure(step)
    lib.ctr_fm_step_tail(_p(loss_elem), _p(gz), B, float(loss_scale), _p(loss_out),
                         _p(bias_grad), _p(p), _p(g), _p(m), _p(v), p.numel(), _p(tab),
                         _p(step_ctr), float(betas[0]), float(betas[1]), float(eps),
                         float(weight_decay), _p(loss_sum) if loss_sum is not None else None,
                         _stream())


def adam_deferred_flush(emb, m_emb, v_emb, lin, m_lin, v_lin, last, step: int,
                        table: AdamStepTable, betas=(0.9, 0.999), eps=1e-8,
                        weight_decay=0.0) -> None:
    V, K = _adam_tables(emb, m_emb, v_emb, lin, m_lin, v_lin)
    _i32(last, "last", V)
    tab = table.ensure(step)
    lib.ctr_adam_deferred_flush(_p(emb), _p(m_emb), _p(v_emb), _p(lin), _p(m_lin), _p(v_lin), V, K,
                                _p(last), int(step), _p(tab), float(betas[0]), float(betas[1]),
                                float(eps), float(weight_decay), _stream())


# ------------------------------------------------------------- Feature_Embedding ----
def feature_embedding(idx: torch.Tensor, emb: torch.Tensor, err_flag=None,
                      out_planes: "Planes | None" = None) -> torch.Tensor:
    """Feature_Embedding's state [B, F(F-1)/2 + F*K]; out_planes: also write its three bf16
    planes (the first planes GEMM's A operand)."""
    idx, it = _idx(idx)
    _f32(emb, "feature_embedding.weight")
    B, F = idx.shape
    V, K = emb.shape
    W = F * (F - 1) // 2 + F * K
    out = torch.empty(B, W, dtype=torch.float32, device=emb.device)
    if out_planes is None:
        lib.ctr_feature_embedding_forward(_p(idx), it, B, F, K, V, _p(emb), _p(out),
                                          _p(err_flag), _stream())
        return out
    if out_planes.rows < B or out_planes.cols < W or out_planes.device != emb.device:
        raise ValueError(f"feature_embedding: out_planes must hold [{B}, {W}] on {emb.device}")
    lib.ctr_feature_embedding_forward_planes(_p(idx), it, B, F, K, V, _p(emb), _p(out),
                                             out_planes.desc, _p(err_flag), _stream())
    return out


def _check_out_planes(who: str, out, planes, B: int, W: int) -> None:
    """The MLP-input writers' checks of the fp32 `out` and the `planes` they may write (the
    same with or without planes: the C side knows ldc only)."""
    if out is not None:
        _dev(out, "out")
        if (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] < B
                or out.shape[1] < W or out.stride(1) != 1):
            raise ValueError(f"{who}: out must be float32 [>= {B}, >= {W}], unit column stride")
    if planes is not None and (planes.rows < B or planes.cols < W):
        raise ValueError(f"{who}: planes [{planes.rows}, {planes.cols}] < [{B}, {W}]")


def ipnn_forward(idx: torch.Tensor, emb: torch.Tensor, out: torch.Tensor | None = None,
                 err_flag=None, planes: "Planes | None" = None) -> torch.Tensor | None:
    """InnerPNN MLP input [B, F*K + F(F-1)/2]: flat embeddings, then the pairwise inner
    products in row-major pair order (p_model.py:187-195). planes: also (or, with
    out=None, only) written as its three bf16 planes — the MLP GEMMs' operand, no split
    pass; returns out (None when only the planes are written)."""
    idx, it = _idx(idx)
    _f32(emb, "feature_embedding.weight")
    B, F = idx.shape
    V, K = emb.shape
    W = F * K + F * (F - 1) // 2
    _check_out_planes("ipnn_forward", out, planes, B, W)
    if planes is not None:
        lib.ctr_ipnn_forward_planes(_p(idx), it, B, F, K, V, _p(emb), _p(out),
                                    out.stride(0) if out is not None else 0, planes.desc,
                                    _p(err_flag), _stream())
        return out
    if out is None:
        out = torch.empty(B, W, dtype=torch.float32, device=emb.device)
    lib.ctr_ipnn_forward(_p(idx), it, B, F, K, V, _p(emb), _p(out), out.stride(0), _p(err_flag),
                         _stream())
    return out


def ipnn_backward(idx: torch.Tensor, emb: torch.Tensor, dcat: torch.Tensor,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-slot embedding gradients [B*F, K] (slot order) from dL/dcat."""
    idx, it = _idx(idx)
    _f32(emb, "feature_embedding.weight")
    _f32(dcat, "dcat")
    B, F = idx.shape
    V, K = emb.shape
    if dcat.shape[0] < B or dcat.shape[1] < F * K + F * (F - 1) // 2 or dcat.stride(1) != 1:
        raise ValueError("ipnn_backward: dcat must be [B, F*K + F(F-1)/2]")
    if out is None:
        out = torch.empty(B * F, K, dtype=torch.float32, device=emb.device)
    else:
        _f32(out, "out")
        if out.numel() < B * F * K:
            raise ValueError(f"ipnn_backward: out must hold [{B * F}, {K}]")
    lib.ctr_ipnn_backward(_p(idx), it, B, F, K, V, _p(emb), _p(dcat), dcat.stride(0), _p(out),
                          _stream())
    return out


def opnn_forward(idx: torch.Tensor, emb: torch.Tensor, ksum: torch.Tensor,
                 out: torch.Tensor | None = None, err_flag=None, planes: "Planes | None" = None,
                 sum_e: torch.Tensor | None = None) -> torch.Tensor | None:
    """OuterPNN MLP input [B, F*K + K]: flat embeddings, then ksum * (sum_f e_f)^2 — the
    reference's kernel-weighted outer-product term, ksum = kernel.sum(0) (p_model.py:244-251).
    planes: also (or, with out=None, only) written as its three bf16 planes; sum_e [B, K]
    (optional) receives the field sum the backward reads. Returns out (None when only the
    planes are written)."""
    idx, it = _idx(idx)
    _f32(emb, "feature_embedding.weight")
    _f32(ksum, "ksum")
    B, F = idx.shape
    V, K = emb.shape
    W = F * K + K
    if ksum.numel() != K:
        raise ValueError(f"opnn_forward: ksum must hold K = {K} values, got {ksum.numel()}")
    _check_out_planes("opnn_forward", out, planes, B, W)
    if sum_e is not None:
        _f32(sum_e, "sum_e")
        if sum_e.numel() < B * K:
            raise ValueError(f"opnn_forward: sum_e must hold [{B}, {K}]")
    if out is None and planes is None:
        out = torch.empty(B, W, dtype=torch.float32, device=emb.device)
    lib.ctr_opnn_forward(_p(idx), it, B, F, K, V, _p(emb), _p(ksum), _p(out),
                         out.stride(0) if out is not None else 0,
                         planes.desc if planes is not None else None, _p(sum_e), _p(err_flag),
                         _stream())
    return out


def opnn_backward(sum_e: torch.Tensor, ksum: torch.Tensor, dcat: torch.Tensor, F: int,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-slot embedding gradients [B*F, K] (slot order) of OuterPNN's MLP input from
    dL/dcat [B, >= F*K + K], the forward's field sums sum_e [B, K] and ksum [K]."""
    _f32(sum_e, "sum_e")
    _f32(ksum, "ksum")
    _dev(dcat, "dcat")
    B, K = sum_e.shape
    F = int(F)
    if (dcat.dtype != torch.float32 or dcat.dim() != 2 or dcat.shape[0] < B
            or dcat.shape[1] < F * K + K or dcat.stride(1) != 1):
        raise ValueError("opnn_backward: dcat must be float32 [B, >= F*K + K], unit column stride")
    if ksum.numel() != K:
        raise ValueError(f"opnn_backward: ksum must hold K = {K} values, got {ksum.numel()}")
    if out is None:
        out = torch.empty(B * F, K, dtype=torch.float32, device=dcat.device)
    else:
        _f32(out, "out")
        if out.numel() < B * F * K:
            raise ValueError(f"opnn_backward: out must hold [{B * F}, {K}]")
    lib.ctr_opnn_backward(B, F, K, _p(sum_e), _p(ksum), _p(dcat), dcat.stride(0), _p(out),
                          _stream())
    return out


AFM_BWD_MAX_BLOCKS = 1024  # csrc/afm.hip kAfmMaxBlocks: the backward's grid and partial slabs


def wd_forward(idx: torch.Tensor, emb: torch.Tensor, lin: torch.Tensor, bias: torch.Tensor,
               out: torch.Tensor | None = None, err_flag=None, planes: "Planes | None" = None,
               z_lin: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Wide&Deep's input (p_model.py:140-142) in one launch: z_lin [B] = bias + sum_f lin[x_f]
    and the MLP input flat(E[x]) [B, F*K], as fp32 (out) and / or as its three bf16 planes
    (planes; with out=None, the planes only). Returns (z_lin, out); out is None when only the
    planes are written."""
    idx, it = _idx(idx)
    if idx.dim() != 2:
        raise ValueError("wd_forward: idx must be [B, F]")
    _f32(emb, "embedding.weight")
    _f32(lin, "linear.weight")
    _f32(bias, "bias")
    B, F = idx.shape
    V, K = emb.shape
    W = F * K
    if lin.numel() != V or bias.numel() != 1:
        raise ValueError(f"wd_forward: linear.weight must hold V = {V} values and bias one")
    _check_out_planes("wd_forward", out, planes, B, W)
    if z_lin is None:
        z_lin = torch.empty(B, dtype=torch.float32, device=emb.device)
    elif _f32(z_lin, "z_lin").numel() < B:
        raise ValueError(f"wd_forward: z_lin must hold {B} values")
    if out is None and planes is None:
        out = torch.empty(B, W, dtype=torch.float32, device=emb.device)
    lib.ctr_wd_forward(_p(idx), it, B, F, K, V, _p(emb), _p(lin), _p(bias), _p(out),
                       out.stride(0) if out is not None else 0,
                       planes.desc if planes is not None else None, _p(z_lin), _p(err_flag),
                       _stream())
    return z_lin, out


def _wd_grad_inputs(who: str, plan: SparsePlanBuffers, F: int, K: int, gz, dx) -> None:
    if int(F) < 1 or plan.S % int(F):
        raise ValueError(f"{who}: the plan's {plan.S} slots must be B * F, F = {F}")
    if _f32(gz, "gz").numel() < plan.S // int(F):
        raise ValueError(f"{who}: gz must hold B = {plan.S // int(F)} values")
    if _f32(dx, "dx").numel() < plan.S * K:
        raise ValueError(f"{who}: dx must be [{plan.S}, {K}]")


def wd_embedding_grad(plan: SparsePlanBuffers, F: int, K: int, gz, dx, rowmap=None,
                      grad_rows=None, grad_lin=None):
    """Wide&Deep's per-unique-row gradient sums (ctr_wd_embedding_grad): a slot's embedding
    gradient is its slice of dx [B, F*K], its linear gradient its example's gz — bitwise
    segment_sum_rows(plan, dx.view(B*F, K), vals_lin=gz.repeat_interleave(F))."""
    _wd_grad_inputs("wd_embedding_grad", plan, F, K, gz, dx)
    cap = max(plan.capacity, 1)
    if grad_rows is None:
        grad_rows = torch.empty(cap, K, dtype=torch.float32, device=dx.device)
    if grad_lin is None:
        grad_lin = torch.empty(cap, dtype=torch.float32, device=dx.device)
    ws = _seg_ws(plan, K)
    lib.ctr_wd_embedding_grad(plan.struct(), int(F), int(K), _p(gz), _p(dx), _p(grad_rows),
                              _p(grad_lin), _p(rowmap), _p(ws), ws.numel(), _stream())
    return grad_rows, grad_lin


def wd_embedding_grad_adam(plan: SparsePlanBuffers, F: int, gz, dx, table, step_dev,
                           step_table: "AdamStepTable", step: int, betas=(0.9, 0.999), eps=1e-8,
                           weight_decay=0.0, grad_rows=None, grad_lin=None,
                           keep_sums: bool = False) -> None:
    """wd_embedding_grad + adam_deferred_rows(sums, step = *step_dev) with the apply fused
    into the combine pass (ctr_wd_embedding_grad_adam): table = (E, m_E, v_E, w, m_w, v_w,
    last); grad_rows / grad_lin are scratch, holding every row's sum with keep_sums."""
    dtab = _deferred_table(*table)
    V, K = table[0].shape
    _i32(step_dev, "step_dev", 1)
    _wd_grad_inputs("wd_embedding_grad_adam", plan, F, K, gz, dx)
    if table[3] is None:
        raise ValueError("wd_embedding_grad_adam: the linear table is needed")
    if grad_lin is None:
        raise ValueError("wd_embedding_grad_adam: grad_rows and grad_lin are needed")
    _plan_grads(plan, V, K, grad_rows, grad_lin, table[3])
    ws = _seg_ws(plan, K)
    tab = step_table.ensure(step)
    lib.ctr_wd_embedding_grad_adam(plan.struct(), int(F), int(K), _p(gz), _p(dx), dtab,
                                   _p(step_dev), _p(tab), float(betas[0]), float(betas[1]),
                                   float(eps), float(weight_decay), _p(grad_rows),
                                   _p(grad_lin), int(keep_sums), _p(ws), ws.numel(), _stream())


def _afm_params(W1, b1, w2, b2, K):
    for t, name in ((W1, "W1"), (b1, "b1"), (w2, "w2"), (b2, "b2")):
        _f32(t, name)
    if W1.dim() != 2 or W1.shape[1] != K:
        raise ValueError(f"afm: W1 must be [A, {K}], got {tuple(W1.shape)}")
    A = W1.shape[0]
    if b1.numel() != A or w2.numel() != A or b2.numel() != 1:
        raise ValueError(f"afm: b1 and w2 must hold A = {A} values and b2 one")
    return A


def afm_forward(idx: torch.Tensor, emb: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor,
                w2: torch.Tensor, b2: torch.Tensor, drop_p: float = 0.0, seed: int = 0,
                want_attn: bool = True, out: torch.Tensor | None = None,
                attn: torch.Tensor | None = None, err_flag=None, step_dev=None):
    """AFM's attention pooling (p_model.py:473-482): (pooled [B, K], attn [B, F(F-1)/2] or
    None). attn is the softmax over the pairs before dropout, what afm_backward reads. Both
    dropouts (attention weights and pooled vector) use one (seed, drop_p); drop_p = 0: none.
    out: a float32 [>= B, >= K] matrix with unit column stride (rows may be strided).
    step_dev (one device int32 t, read by the kernel): the masks of
    afm_step_seed(seed, t) — a captured graph then draws new masks at every replay."""
    idx, it = _idx(idx)
    _f32(emb, "feature_embedding.weight")
    B, F = idx.shape
    V, K = emb.shape
    A = _afm_params(W1, b1, w2, b2, K)
    P = F * (F - 1) // 2
    if out is None:
        out = torch.empty(B, K, dtype=torch.float32, device=emb.device)
    else:
        _rows2d(out, "out", B, K)
    if attn is None and want_attn:
        attn = torch.empty(B, P, dtype=torch.float32, device=emb.device)
    if attn is not None:
        _f32(attn, "attn")
        if attn.numel() < B * P:
            raise ValueError(f"afm_forward: attn must hold [{B}, {P}]")
    ldp = out.stride(0) if B > 1 else K  # a lone row's stride is arbitrary
    if step_dev is None:
        lib.ctr_afm_forward(_p(idx), it, B, F, K, A, V, _p(emb), _p(W1), _p(b1), _p(w2), _p(b2),
                            float(drop_p), int(seed) & (2**64 - 1), _p(out), ldp, _p(attn),
                            _p(err_flag), _stream())
    else:
        _i32(step_dev, "step_dev", 1)
        lib.ctr_afm_forward_step(_p(idx), it, B, F, K, A, V, _p(emb), _p(W1), _p(b1), _p(w2),
                                 _p(b2), float(drop_p), int(seed) & (2**64 - 1), _p(step_dev),
                                 _p(out), ldp, _p(attn), _p(err_flag), _stream())
    return (out if out.shape == (B, K) else out[:B, :K]), attn


def afm_step_seed(seed: int, step: int) -> int:
    """The dropout seed ctr_afm_forward_step / ctr_afm_backward_step use at device step
    `step`: seed + uint32(step) * 0x9E3779B97F4A7C15 mod 2^64."""
    return (int(seed) + (int(step) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15) & (2**64 - 1)


def afm_backward(idx: torch.Tensor, emb: torch.Tensor, W1: torch.Tensor, b1: torch.Tensor,
                 w2: torch.Tensor, b2: torch.Tensor, attn: torch.Tensor, dpooled: torch.Tensor,
                 drop_p: float = 0.0, seed: int = 0, out: dict | None = None,
                 err_flag=None, step_dev=None) -> dict:
    """Backward of afm_forward from dL/dpooled [B, K] and the forward's attn: dict(dslot
    [B*F, K] in slot order, dW1 [A, K], db1 [A], dw2 [A], db2 [1]); (seed, drop_p, step_dev)
    as in the forward. One kernel over the batch plus the deterministic reduction of its
    per-block partials."""
    idx, it = _idx(idx)
    _f32(emb, "feature_embedding.weight")
    B, F = idx.shape
    V, K = emb.shape
    A = _afm_params(W1, b1, w2, b2, K)
    P = F * (F - 1) // 2
    _f32(attn, "attn")
    if attn.numel() < B * P:
        raise ValueError(f"afm_backward: attn must hold [{B}, {P}]")
    _rows2d(dpooled, "dpooled", B, K)
    if out is None:
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=emb.device)  # noqa: E731
        out = dict(dslot=e(B * F, K), dW1=e(A, K), db1=e(A), dw2=e(A), db2=e(1))
    for name, n in (("dslot", B * F * K), ("dW1", A * K), ("db1", A), ("dw2", A), ("db2", 1)):
        _f32(out[name], name)
        if out[name].numel() < n:
            raise ValueError(f"afm_backward: {name} must hold {n} values")
    ws = Workspace.get(lib.ctr_afm_workspace_bytes(B, F, K, A), emb.device)
    head = (_p(idx), it, B, F, K, A, V, _p(emb), _p(W1), _p(b1), _p(w2), _p(b2), float(drop_p),
            int(seed) & (2**64 - 1))
    tail = (_p(attn), _p(dpooled), dpooled.stride(0) if B > 1 else K, _p(out["dslot"]),
            _p(out["dW1"]), _p(out["db1"]), _p(out["dw2"]), _p(out["db2"]), _p(ws), ws.numel(),
            _p(err_flag), _stream())
    if step_dev is None:
        lib.ctr_afm_backward(*head, *tail)
    else:
        _i32(step_dev, "step_dev", 1)
        lib.ctr_afm_backward_step(*head, _p(step_dev), *tail)
    return out


def afm_head(idx: torch.Tensor, lin: torch.Tensor, bias: torch.Tensor, pooled: torch.Tensor,
             fc_w: torch.Tensor, fc_b: torch.Tensor, labels: torch.Tensor,
             mean_div: float | None = None, out: dict | None = None, err_flag=None) -> dict:
    """AFM's out head for the fused step in one launch (ctr_afm_head): z = (bias + sum_f
    lin[x_f]) + fc(pooled), the BCE head and dpooled = gz * fc_w — dict(z, p, loss_elem, gz [B],
    dpooled [B, K]); z, p, loss_elem, gz are the bits of deepfm_head(pooled, fc_w, fc_b,
    lr_forward(idx, lin, bias)["z"], labels, mean_div). pooled and out["dpooled"]: float32
    [>= B, >= K] with unit column stride (rows may be strided). out: the five buffers (z, p,
    loss_elem may be None), so a captured graph allocates nothing."""
    idx, it = _idx(idx)
    if idx.dim() != 2:
        raise ValueError("afm_head: idx must be [B, F]")
    B, F = idx.shape
    _f32(lin, "linear.weight")
    _f32(bias, "bias")
    _f32(fc_w, "fc.weight")
    _f32(fc_b, "fc.bias")
    _f32(labels, "labels")
    K, V = fc_w.numel(), lin.numel()
    if bias.numel() != 1 or fc_b.numel() != 1 or labels.numel() != B:
        raise ValueError(f"afm_head: bias and fc.bias hold one value, labels B = {B}")
    _rows2d(pooled, "pooled", B, K)
    dev = lin.device
    if out is None:
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        out = dict(z=e(B), p=e(B), loss_elem=e(B), gz=e(B), dpooled=e(B, K))
    for name in ("z", "p", "loss_elem", "gz"):
        t = out.get(name)
        if t is None and name != "gz":
            continue
        if _f32(t, name).numel() < B:
            raise ValueError(f"afm_head: {name} must hold {B} values")
    dp = _rows2d(out["dpooled"], "dpooled", B, K)
    lib.ctr_afm_head(_p(idx), it, B, F, K, V, _p(lin), _p(bias), _p(pooled),
                     pooled.stride(0) if B > 1 else K, _p(fc_w), _p(fc_b), _p(labels),
                     float(B if mean_div is None else mean_div), _p(out.get("z")),
                     _p(out.get("p")), _p(out.get("loss_elem")), _p(out["gz"]), _p(dp),
                     dp.stride(0) if B > 1 else K, _p(err_flag), _stream())
    return out


def _rows2d(t: torch.Tensor, name: str, B: int, D: int) -> torch.Tensor:
    """A float32 device matrix with >= B rows of >= D unit-stride columns (rows may be
    strided: a view into a wider buffer)."""
    _dev(t, name)
    if (t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < B or t.shape[1] < D
            or (t.numel() and t.stride(1) != 1) or (B > 1 and t.stride(0) < D)):
        raise ValueError(f"{name}: must be float32 [>= {B}, >= {D}] with unit column stride")
    return t


def _dcn_params(W, bias, w_tail):
    _f32(W, "W")
    _f32(bias, "bias")
    if W.dim() != 2 or bias.shape != W.shape:
        raise ValueError("dcn_cross: W and bias must both be [L, D]")
    L, D = W.shape
    if w_tail is not None:
        _f32(w_tail, "w_tail")
        if w_tail.numel() != D:
            raise ValueError(f"dcn_cross: w_tail must have {D} elements")
    return L, D


def dcn_cross_forward(x0: torch.Tensor, W: torch.Tensor, bias: torch.Tensor,
                      w_tail: torch.Tensor | None = None, *, want_xl: bool | None = None,
                      out: dict | None = None) -> dict:
    """DCN's cross network (p_model.py:426-429) over x0 [B, D] with the stacked W, bias [L, D]:
    dict(s [B, L], xL [B, D] or None, z [B] = <x_L, w_tail> or None). want_xl defaults to
    "no w_tail given"; with w_tail and want_xl=False x_L is never written."""
    L, D = _dcn_params(W, bias, w_tail)
    if x0.dim() != 2 or x0.shape[1] != D:
        raise ValueError(f"dcn_cross_forward: x0 must be [B, {D}]")
    B = x0.shape[0]
    _rows2d(x0, "x0", B, D)
    if want_xl is None:
        want_xl = w_tail is None
    if out is None:
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=x0.device)  # noqa: E731
        out = dict(s=e(B, L), xL=e(B, D) if want_xl else None,
                   z=e(B) if w_tail is not None else None)
    xL, z = out.get("xL"), out.get("z")
    _f32(out["s"], "s")
    if xL is not None:
        _rows2d(xL, "xL", B, D)
    if z is not None:
        _f32(z, "z")
    lib.ctr_dcn_cross_forward(B, D, L, _p(x0), x0.stride(0) if B else D, _p(W), _p(bias),
                              _p(w_tail), _p(out["s"]), _p(xL),
                              xL.stride(0) if xL is not None and B else D, _p(z), _stream())
    return out


def dcn_cross_backward(x0: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, s: torch.Tensor,
                       gL: torch.Tensor | None = None, gz: torch.Tensor | None = None,
                       w_tail: torch.Tensor | None = None, out: dict | None = None) -> dict:
    """Backward of dcn_cross_forward for dL/dx_L = gL [B, D] (optional) + gz[b] * w_tail (the
    rank-1 form of DCN's final Linear; gz and w_tail together): dict(dx0 [B, D], dW [L, D],
    dbias [L, D], dw_tail [D] or None). One kernel over the batch plus the deterministic
    reduction of its per-block partials."""
    L, D = _dcn_params(W, bias, w_tail)
    if x0.dim() != 2 or x0.shape[1] != D:
        raise ValueError(f"dcn_cross_backward: x0 must be [B, {D}]")
    B = x0.shape[0]
    _rows2d(x0, "x0", B, D)
    _f32(s, "s")
    if s.numel() != B * L:
        raise ValueError(f"dcn_cross_backward: s must be [{B}, {L}]")
    if gL is not None:
        _rows2d(gL, "gL", B, D)
    if gz is not None:
        _f32(gz, "gz")
        if gz.numel() != B:
            raise ValueError(f"dcn_cross_backward: gz must have {B} elements")
    if out is None:
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=x0.device)  # noqa: E731
        out = dict(dx0=e(B, D), dW=e(L, D), dbias=e(L, D), dw_tail=e(D) if gz is not None else None)
    dx0 = _rows2d(out["dx0"], "dx0", B, D)
    _f32(out["dW"], "dW")
    _f32(out["dbias"], "dbias")
    if out.get("dw_tail") is not None:
        _f32(out["dw_tail"], "dw_tail")
    ws = Workspace.get(lib.ctr_dcn_cross_workspace_bytes(B, D, L), x0.device)
    lib.ctr_dcn_cross_backward(B, D, L, _p(x0), x0.stride(0) if B else D, _p(W), _p(bias), _p(s),
                               _p(gL), gL.stride(0) if gL is not None and B else D, _p(gz),
                               _p(w_tail), _p(dx0), dx0.stride(0) if B else D, _p(out["dW"]),
                               _p(out["dbias"]), _p(out.get("dw_tail")), _p(ws), ws.numel(),
                               _stream())
    return out


# ------------------------------------------------- prioritized replay memory (PER) ----
PER_STOCHASTIC, PER_GREEDY = 0, 1
PER_MAX_K = 8192
_per_ws: dict = {}  # (device index, stream, N, k) -> scratch of ctr_per_workspace_bytes(N, k)


def _per_store(memory: torch.Tensor, prio: torch.Tensor) -> tuple[int, int]:
    _f32(memory, "memory")
    _f32(prio, "prio")
    if memory.dim() != 2 or prio.numel() != memory.shape[0]:
        raise ValueError("per: memory must be [N, T] and prio must hold N priorities")
    return memory.shape[0], memory.shape[1]


def _per_td(td: torch.Tensor, n: int) -> torch.Tensor:
    _f32(td, "td")
    if td.numel() != n:
        raise ValueError(f"per: td must hold {n} errors, got {tuple(td.shape)}")
    return td


def per_add(memory: torch.Tensor, prio: torch.Tensor, start: int, transitions: torch.Tensor,
            td: torch.Tensor, eps: float, alpha: float) -> None:
    """Memory.add's writes (Hybrid_TD3_model_PER.py:44-63): transitions [n, T] go to slots
    (start + i) % N of memory [N, T]; prio = max(prio, (|td| + eps)^alpha) there. One launch."""
    N, T = _per_store(memory, prio)
    n = transitions.shape[0] if transitions.dim() == 2 else -1
    if n < 0 or transitions.shape[1] != T:
        raise ValueError(f"per_add: transitions must be [n, {T}]")
    _rows2d(transitions, "transitions", n, T)
    _per_td(td, n)
    lib.ctr_per_add(N, T, start, n, _p(transitions), transitions.stride(0) if n else T, _p(td),
                    eps, alpha, _p(memory), _p(prio), _stream())


def _per_rows(t: torch.Tensor, name: str, n: int, D: int) -> int:
    """float32 [n, D] with unit column stride (a view of a wider matrix is fine): its row
    stride."""
    _dev(t, name)
    if t.dtype != torch.float32 or t.dim() != 2 or tuple(t.shape) != (n, D):
        raise ValueError(f"per_store_step: {name} must be float32 [{n}, {D}]")
    if n == 0:
        return D
    if D > 1 and t.stride(1) != 1:
        raise ValueError(f"per_store_step: {name} must have unit column stride")
    if n > 1 and t.stride(0) < D:
        raise ValueError(f"per_store_step: {name} has row stride {t.stride(0)} < {D}")
    return t.stride(0) if n > 1 else D


def per_store_step(memory: torch.Tensor, prio: torch.Tensor, start: int, features: torch.Tensor,
                   c_actions: torch.Tensor, d_values: torch.Tensor, d_actions: torch.Tensor,
                   rewards: torch.Tensor, eps: float, alpha: float) -> None:
    """The driver's per-batch store as one launch: memory[(start + i) % N] = [float(features[i])
    | c_actions[i] | d_values[i] | float(d_actions[i]) | rewards[i]] and prio = max(prio,
    (1 + eps)^alpha) there — bitwise what the casts, torch.cat and per_add(ones) leave."""
    N, T = _per_store(memory, prio)
    feats, it = _idx(features, "features")
    if feats.dim() != 2:
        raise ValueError("per_store_step: features must be [n, F]")
    n, F = feats.shape
    A = c_actions.shape[1] if isinstance(c_actions, torch.Tensor) and c_actions.dim() == 2 else -1
    if A < 1 or T != F + 2 * A + 2:
        raise ValueError(f"per_store_step: T={T} is not F + 2A + 2 (F={F}, A={A})")
    if n > N:
        raise ValueError(f"per_store_step: {n} transitions do not fit a memory of {N}")
    ldc = _per_rows(c_actions, "c_actions", n, A)
    ldd = _per_rows(d_values, "d_values", n, A)
    ldr = _per_rows(rewards.view(n, 1) if rewards.dim() == 1 else rewards, "rewards", n, 1)
    if d_actions.numel() != n:
        raise ValueError(f"per_store_step: d_actions must hold {n} actions")
    act, at = _idx(d_actions.reshape(n), "d_actions")
    lib.ctr_per_store_step(N, T, start, n, F, A, _p(feats), it, _p(c_actions), ldc, _p(d_values),
                           ldd, _p(act), at, _p(rewards), ldr, eps, alpha, _p(memory), _p(prio),
                           _stream())


def per_update(prio: torch.Tensor, idx: torch.Tensor, td: torch.Tensor, eps: float,
               alpha: float) -> None:
    """Memory.batch_update: prio[idx] = (|td| + eps)^alpha (duplicate indices: undefined)."""
    _f32(prio, "prio")
    _dev(idx, "idx")
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError("per_update: idx must be a contiguous int64 vector")
    _per_td(td, idx.numel())
    lib.ctr_per_update(prio.numel(), idx.numel(), _p(idx), _p(td), eps, alpha, _p(prio),
                       _stream())


def per_keys(prio: torch.Tensor, n_valid: int, mode: int, seed: int,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """The selection keys of prio[:n_valid] (include/ctr_hip.h), bitwise what per_sample
    orders by."""
    _f32(prio, "prio")
    if not 0 <= n_valid <= prio.numel():
        raise ValueError(f"per_keys: n_valid {n_valid} outside [0, {prio.numel()}]")
    if out is None:
        out = torch.empty(n_valid, dtype=torch.float32, device=prio.device)
    _f32(out, "keys")
    if out.numel() < n_valid:
        raise ValueError("per_keys: out is shorter than n_valid")
    lib.ctr_per_keys(n_valid, _p(prio), mode, seed, _p(out), _stream())
    return out


def per_sample(memory: torch.Tensor, prio: torch.Tensor, n_valid: int, k: int, mode: int,
               seed: int, beta: float, out: dict | None = None) -> dict:
    """The k largest selection keys of the filled prefix [0, n_valid), in descending order:
    dict(idx [k] int64, batch [k, T] = memory[idx], isw [k, 1] = (prio[idx] / min_p)^(-beta),
    min_p [1]). mode PER_STOCHASTIC draws by priority without replacement (seed picks the
    draw), PER_GREEDY takes the largest priorities. Nothing is copied to the host."""
    N, T = _per_store(memory, prio)
    if not 1 <= k <= min(n_valid, PER_MAX_K) or n_valid > N:
        raise ValueError(f"per_sample: k={k} outside [1, min(n_valid={n_valid}, {PER_MAX_K})] "
                         f"or n_valid > N={N}")
    dev = memory.device
    if out is None:
        out = dict(idx=torch.empty(k, dtype=torch.int64, device=dev),
                   batch=torch.empty(k, T, dtype=torch.float32, device=dev),
                   isw=torch.empty(k, 1, dtype=torch.float32, device=dev),
                   min_p=torch.empty(1, dtype=torch.float32, device=dev))
    idx, batch, isw, min_p = _dev(out["idx"], "idx"), _f32(out["batch"], "batch"), \
        _f32(out["isw"], "isw"), out.get("min_p")
    if (idx.dtype != torch.int64 or not idx.is_contiguous() or idx.numel() != k
            or batch.numel() != k * T or isw.numel() != k):
        raise ValueError(f"per_sample: out must hold idx [{k}] int64, batch [{k}, {T}], isw [{k}]")
    if min_p is not None:
        _f32(min_p, "min_p")
    key = (dev.index, _stream(), N, k)  # launches on one stream are ordered: they may share it
    ws = _per_ws.get(key)
    if ws is None:
        ws = _per_ws[key] = torch.empty(lib.ctr_per_workspace_bytes(N, k), dtype=torch.uint8,
                                        device=dev)
    lib.ctr_per_sample(N, T, n_valid, k, mode, seed, beta, _p(memory), _p(prio), _p(idx),
                       _p(batch), _p(isw), _p(min_p), _p(ws), ws.numel(), _stream())
    return out


# --------------------------------------- evaluation metrics (csrc/metrics.hip) --------
METRICS_TILE = 4096         # records per sort / reduce tile (ctr_metrics_tile())
METRICS_STATE_WORDS = 16    # the state block, as int64 words (include/ctr_hip.h)
_LABEL_TYPES = {torch.float32: CTR_LABEL_F32, torch.int32: CTR_LABEL_I32,
                torch.int64: CTR_LABEL_I64}


def metrics_workspace_bytes(cap: int) -> int:
    n = lib.ctr_metrics_workspace_bytes(cap)
    if n <= 0:
        raise ValueError(f"metrics: capacity {cap} outside [1, 2^31)")
    return n


def _metrics_buffers(records: torch.Tensor, ws: torch.Tensor, state: torch.Tensor) -> int:
    _dev(records, "records")
    _dev(ws, "ws")
    _dev(state, "state")
    if records.dtype != torch.int64 or records.dim() != 1 or not records.is_contiguous():
        raise ValueError("metrics: records must be a contiguous int64 vector")
    if state.dtype != torch.int64 or state.numel() != METRICS_STATE_WORDS or \
            not state.is_contiguous():
        raise ValueError(f"metrics: state must be {METRICS_STATE_WORDS} contiguous int64 words")
    if ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise ValueError("metrics: ws must be a contiguous uint8 buffer")
    return records.numel()


def _metrics_stride(t: torch.Tensor, name: str) -> int:
    """Element stride of a float32 prediction tensor read in logical order: contiguous, a
    [B, 1] view, or a column of a wider matrix."""
    _dev(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if t.numel() <= 1 or t.is_contiguous():
        return 1
    dims = [(s, st) for s, st in zip(t.shape, t.stride()) if s != 1]
    if len(dims) != 1 or dims[0][1] < 1:
        raise ValueError(f"{name}: must be contiguous or a single strided column, got shape "
                         f"{tuple(t.shape)} strides {t.stride()}")
    return dims[0][1]


def metrics_reset(state: torch.Tensor) -> None:
    _dev(state, "state")
    if state.dtype != torch.int64 or state.numel() != METRICS_STATE_WORDS or \
            not state.is_contiguous():
        raise ValueError(f"metrics: state must be {METRICS_STATE_WORDS} contiguous int64 words")
    lib.ctr_metrics_reset(_p(state), _stream())


def metrics_append(records: torch.Tensor, offset: int, y_pred: torch.Tensor,
                   labels: torch.Tensor, rewards: torch.Tensor | None, with_loss: bool,
                   ws: torch.Tensor, state: torch.Tensor) -> int:
    """One batch into records[offset : offset + n] (include/ctr_hip.h, ctr_metrics_append);
    returns n. Nothing is read back."""
    cap = _metrics_buffers(records, ws, state)
    stride = _metrics_stride(y_pred, "y_pred")
    n = y_pred.numel()
    _dev(labels, "labels")
    if labels.dtype not in _LABEL_TYPES:
        raise TypeError(f"labels: expected float32, int32 or int64, got {labels.dtype}")
    if labels.numel() != n:
        raise ValueError(f"metrics: {n} predictions but {labels.numel()} labels")
    if not labels.is_contiguous():
        raise ValueError("labels: must be contiguous")
    if rewards is not None:
        _f32(rewards, "rewards")
        if rewards.numel() != n:
            raise ValueError(f"metrics: {n} predictions but {rewards.numel()} rewards")
    if offset < 0 or offset + n > cap:
        raise ValueError(f"metrics: offset {offset} + n {n} exceeds the capacity {cap}")
    lib.ctr_metrics_append(cap, offset, n, _p(y_pred), stride, _p(labels),
                           _LABEL_TYPES[labels.dtype], _p(rewards), 1 if with_loss else 0,
                           _p(records), _p(ws), ws.numel(), _p(state), _stream())
    return n


def metrics_auc(records: torch.Tensor, count: int, ws: torch.Tensor,
                state: torch.Tensor) -> None:
    """Sort records[:count] in place and leave U2, P, N in the state block."""
    cap = _metrics_buffers(records, ws, state)
    if not 0 <= count <= cap:
        raise ValueError(f"metrics: count {count} outside [0, {cap}]")
    lib.ctr_metrics_auc(cap, count, _p(records), _p(ws), ws.numel(), _p(state), _stream())


# --------------------------------------------- hybrid TD3 agent (csrc/td3.hip) ---------
TD3_NOISE_NONE, TD3_NOISE_PTR, TD3_NOISE_SEED = 0, 1, 2
TD3_MAX_A = 64


def _ld2(t: torch.Tensor, name: str) -> int:
    """A float32 [B, N] device matrix with unit column stride (a column block of a wider
    matrix is fine); returns its row stride."""
    _dev(t, name)
    if t.dtype != torch.float32 or t.dim() != 2:
        raise TypeError(f"{name}: expected a float32 matrix, got {t.dtype} {tuple(t.shape)}")
    B, N = t.shape
    if N > 1 and t.stride(1) != 1:
        raise ValueError(f"{name}: rows must be contiguous")
    ld = t.stride(0) if B > 1 else N
    if ld < N:
        raise ValueError(f"{name}: row stride {ld} < N = {N}")
    return ld


def _vecN(t: torch.Tensor | None, name: str, n: int):
    if t is not None:
        _f32(t, name)
        if t.numel() != n:
            raise ValueError(f"{name}: must hold {n} elements, got {tuple(t.shape)}")
    return t


def bn_forward(x: torch.Tensor, gamma, beta, running_mean, running_var, *, eps: float = 1e-5,
               momentum: float = 0.1, training: bool = True, relu: bool = False,
               out: torch.Tensor | None = None, save: bool = True) -> dict:
    """nn.BatchNorm1d (+ReLU) on x [B, N]: dict(y, mean, mean_lo, invstd, invstd_lo).
    Training mode normalises with the batch statistics (fp64 two-pass), updates the running
    statistics in place and, with save, returns what bn_backward needs (the *_lo vectors are
    the parts of the fp64 statistics that fp32 drops); eval mode reads the running ones.
    out: where y goes, e.g. the first N columns of a wider matrix."""
    ldx = _ld2(x, "x")
    B, N = x.shape
    if out is None:
        out = torch.empty(B, N, dtype=torch.float32, device=x.device)
    ldy = _ld2(out, "out")
    if tuple(out.shape) != (B, N):
        raise ValueError(f"bn_forward: out must be [{B}, {N}]")
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"),
                  (running_var, "running_var")):
        _vecN(t, nm, N)
    mean = lo = inv = inv_lo = None
    if training and save:
        stats = torch.empty(4, N, dtype=torch.float32, device=x.device)
        mean, lo, inv, inv_lo = stats[0], stats[1], stats[2], stats[3]
    lib.ctr_bn_forward(B, N, _p(x), ldx, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                       float(eps), float(momentum), int(training), int(relu), _p(out), ldy,
                       _p(mean), _p(lo), _p(inv), _p(inv_lo), _stream())
    return dict(y=out, mean=mean, mean_lo=lo, invstd=inv, invstd_lo=inv_lo)


def bn_backward(dy: torch.Tensor, x: torch.Tensor, mean, invstd, gamma, *, y=None,
                relu: bool = False, mean_lo=None, invstd_lo=None, want_dx: bool = True,
                dx: torch.Tensor | None = None) -> dict:
    """Training-mode BatchNorm1d (+ReLU) backward in one launch: dict(dgamma, dbeta, dx)."""
    lddy = _ld2(dy, "dy")
    B, N = dy.shape
    ldx = _ld2(x, "x")
    if tuple(x.shape) != (B, N):
        raise ValueError(f"bn_backward: x must be [{B}, {N}]")
    ldy = 0
    if relu:
        if y is None or tuple(y.shape) != (B, N):
            raise ValueError(f"bn_backward: relu needs the forward's y [{B}, {N}]")
        ldy = _ld2(y, "y")
    for t, nm in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (mean_lo, "mean_lo"),
                  (invstd_lo, "invstd_lo")):
        _vecN(t, nm, N)
    out = torch.empty(2, N, dtype=torch.float32, device=dy.device)
    ldd = 0
    if want_dx:
        if dx is None:
            dx = torch.empty(B, N, dtype=torch.float32, device=dy.device)
        ldd = _ld2(dx, "dx")
        if tuple(dx.shape) != (B, N):
            raise ValueError(f"bn_backward: dx must be [{B}, {N}]")
    else:
        dx = None
    lib.ctr_bn_backward(B, N, _p(dy), lddy, _p(y) if relu else None, ldy, int(relu), _p(x), ldx,
                        _p(mean), _p(mean_lo), _p(invstd), _p(invstd_lo), _p(gamma), _p(out[0]),
                        _p(out[1]), _p(dx), ldd, _stream())
    return dict(dgamma=out[0], dbeta=out[1], dx=dx)


def td3_noise(n: int, seed: int, offset: int = 0, out: torch.Tensor | None = None,
              device=None) -> torch.Tensor:
    """n unit-normal draws, elements offset .. offset + n - 1 of stream `seed`: bitwise what
    td3_act / td3_smooth consume in seed mode (head h of a [B, A] pair starts at h * B * A)."""
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=device if device is not None else "cuda")
    _f32(out, "out")
    if out.numel() < n:
        raise ValueError("td3_noise: out is shorter than n")
    lib.ctr_td3_noise(n, int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), _p(out), _stream())
    return out


def _td3_noise_args(noise, seed, B: int, A: int):
    if noise is not None:
        n_c, n_d = noise
        for t, nm in ((n_c, "noise_c"), (n_d, "noise_d")):
            _f32(t, nm)
            if tuple(t.shape) != (B, A):
                raise ValueError(f"{nm}: must be [{B}, {A}]")
        return TD3_NOISE_PTR, n_c, n_d, 0
    if seed is not None:
        return TD3_NOISE_SEED, None, None, int(seed) & (2**64 - 1)
    return TD3_NOISE_NONE, None, None, 0


def td3_act(pre_c: torch.Tensor, pre_d: torch.Tensor, *, noise=None, seed=None,
            sigma: float = 0.1, want_softmax: bool = True, want_index: bool = True) -> dict:
    """The action heads from their pre-activations [B, A]: tanh, then (noise=(n_c, n_d) or
    seed=) clamp(v + sigma * noise, -1, 1): dict(c_actions, c_softmax, d_actions, d_index
    [B, 1] int64 = argmax + 1, the lowest index among equal values)."""
    ldp = _ld2(pre_c, "pre_c")
    B, A = pre_c.shape
    if tuple(pre_d.shape) != (B, A) or _ld2(pre_d, "pre_d") != ldp:
        raise ValueError("td3_act: pre_c and pre_d must have one shape and row stride")
    mode, n_c, n_d, sd = _td3_noise_args(noise, seed, B, A)
    dev = pre_c.device
    c = torch.empty(B, A, dtype=torch.float32, device=dev)
    d = torch.empty(B, A, dtype=torch.float32, device=dev)
    sm = torch.empty(B, A, dtype=torch.float32, device=dev) if want_softmax else None
    ix = torch.empty(B, 1, dtype=torch.int64, device=dev) if want_index else None
    lib.ctr_td3_act(B, A, _p(pre_c), _p(pre_d), ldp, mode, _p(n_c), _p(n_d), sd, float(sigma),
                    _p(c), _p(sm), _p(d), _p(ix), _stream())
    return dict(c_actions=c, c_softmax=sm, d_actions=d, d_index=ix)


def td3_smooth(mean_c: torch.Tensor, mean_d: torch.Tensor, out_c: torch.Tensor,
               out_d: torch.Tensor, *, noise=None, seed=None, apply_tanh: bool = False) -> None:
    """Target policy smoothing of both heads, clamp(mean + clamp(0.2 * noise, -0.5, 0.5), -1, 1),
    written to out_c / out_d: two [B, A] column blocks of one matrix (the target critic's
    input). apply_tanh: the means are pre-activations."""
    ldm = _ld2(mean_c, "mean_c")
    B, A = mean_c.shape
    if tuple(mean_d.shape) != (B, A) or _ld2(mean_d, "mean_d") != ldm:
        raise ValueError("td3_smooth: mean_c and mean_d must have one shape and row stride")
    ldo = _ld2(out_c, "out_c")
    if tuple(out_c.shape) != (B, A) or tuple(out_d.shape) != (B, A) or _ld2(out_d, "out_d") != ldo:
        raise ValueError(f"td3_smooth: out_c and out_d must be [{B}, {A}] with one row stride")
    mode, n_c, n_d, sd = _td3_noise_args(noise, seed, B, A)
    lib.ctr_td3_smooth(B, A, _p(mean_c), _p(mean_d), ldm, int(apply_tanh), mode, _p(n_c), _p(n_d),
                       sd, _p(out_c), _p(out_d), ldo, _stream())


def td3_critic_loss(q1, q2, q1_t, q2_t, r: torch.Tensor, isw, gamma: float) -> dict:
    """The twin critics' importance-weighted loss and everything derived from it in one launch:
    dict(q_target, td, dq1, dq2 [B, 1], loss (0-dim)). r: [B] or [B, 1], any stride."""
    B = q1.numel()
    for t, nm in ((q1, "q1"), (q2, "q2"), (q1_t, "q1_t"), (q2_t, "q2_t"), (isw, "isw")):
        _vecN(t, nm, B)
    _dev(r, "r")
    if r.dtype != torch.float32 or r.numel() != B or r.dim() not in (1, 2) or \
            (r.dim() == 2 and r.shape[1] != 1):
        raise ValueError(f"td3_critic_loss: r must be float32 [{B}] or [{B}, 1]")
    ldr = r.stride(0) if B > 1 else 1
    if ldr < 1:
        raise ValueError("td3_critic_loss: r must have a positive stride")
    o = torch.empty(4, B, 1, dtype=torch.float32, device=q1.device)
    loss = torch.empty(1, dtype=torch.float32, device=q1.device)
    lib.ctr_td3_critic_loss(B, _p(q1), _p(q2), _p(q1_t), _p(q2_t), _p(r), ldr, _p(isw),
                            float(gamma), _p(o[0]), _p(o[1]), _p(loss), _p(o[2]), _p(o[3]),
                            _stream())
    return dict(q_target=o[0], td=o[1], dq1=o[2], dq2=o[3], loss=loss.reshape(()))


class SoftUpdateTable:
    """The device table of (target, source, numel) triples of ctr_soft_update_multi, built
    once for a list of tensor pairs and kept (it holds the tensors, so their addresses stay
    valid). matches() tells whether it still describes a given list of pairs."""

    def __init__(self, targets, sources):
        targets, sources = list(targets), list(sources)
        if len(targets) != len(sources) or not targets:
            raise ValueError("SoftUpdateTable: one source per target, at least one")
        rows = []
        for t, s in zip(targets, sources):
            _f32(t, "target")
            _f32(s, "source")
            if t.shape != s.shape or t.device != s.device:
                raise ValueError("SoftUpdateTable: a target and its source differ in shape/device")
            if t.numel():
                rows.append((t.data_ptr(), s.data_ptr(), t.numel()))
        self.tensors = (targets, sources)
        self.key = tuple(rows)
        self.count = len(rows)
        self.max_numel = max((r[2] for r in rows), default=0)
        self.device = targets[0].device
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.device) if rows else None

    def matches(self, targets, sources) -> bool:
        return self.key == tuple((t.data_ptr(), s.data_ptr(), t.numel())
                                 for t, s in zip(targets, sources) if t.numel())


def soft_update_multi(table: SoftUpdateTable, tau: float) -> None:
    """target = target * (1 - tau) + source * tau over every pair of the table, one launch."""
    if table.count == 0:
        return
    lib.ctr_soft_update_multi(table.count, _p(table.table), table.max_numel, float(tau),
                              _stream())


# ------------------------------------------ v10 hybrid TD3 agent (csrc/td3_v10.hip) ----
V10_ACT, V10_PLAIN, V10_RANDOM, V10_BEST = 0, 1, 2, 3
GRAD_CLIP_MAX_TENSORS = 64
_V10_MAX_WS_BYTES = 4096


def _ba(t, name: str, B: int, A: int):
    """An optional contiguous float32 [B, A] device tensor."""
    if t is not None:
        _f32(t, name)
        if tuple(t.shape) != (B, A):
            raise ValueError(f"{name}: must be [{B}, {A}], got {tuple(t.shape)}")
    return t


def td3v10_uniform(n: int, seed: int, offset: int = 0, out: torch.Tensor | None = None,
                   device=None) -> torch.Tensor:
    """n uniforms in (0, 1), elements offset .. offset + n - 1 of stream `seed`: the first
    uniform of td3_noise's element (draw normals and uniforms of one seed from disjoint ranges)."""
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=device if device is not None else "cuda")
    _f32(out, "out")
    if out.numel() < n:
        raise ValueError("td3v10_uniform: out is shorter than n")
    lib.ctr_td3v10_uniform(n, int(seed) & (2**64 - 1), int(offset) & (2**64 - 1), _p(out),
                           _stream())
    return out


def td3v10_heads(mode: int, pre_c=None, pre_d=None, *, noise_c=None, noise_d=None, uniform=None,
                 temperature: float = 1.0, want_softmax: bool = True, want_index: bool = True):
    """The v10 action heads in one launch (include/ctr_hip.h, ctr_td3v10_heads):
    dict(c_means, c_softmax, d_action, d_index [B, 1] int64 = argmax + 1, lowest index on ties).
    mode V10_ACT (exploration noise and Gumbel at `temperature`), V10_PLAIN (Gumbel softmax of
    the bare heads), V10_RANDOM (actions from the normals alone; pre_c / pre_d unused) or
    V10_BEST (no d_action; the index of the largest d_q + Gumbel)."""
    if mode not in (V10_ACT, V10_PLAIN, V10_RANDOM, V10_BEST):
        raise ValueError(f"td3v10_heads: unknown mode {mode}")
    if mode == V10_RANDOM:
        if noise_c is None or noise_c.dim() != 2:
            raise ValueError("td3v10_heads: the random mode needs noise_c, noise_d [B, A]")
        _dev(noise_c, "noise_c")
        B, A = noise_c.shape
        ldp = A
        pre_c = pre_d = uniform = None
    else:
        ldp = _ld2(pre_c, "pre_c")
        B, A = pre_c.shape
        if tuple(pre_d.shape) != (B, A) or _ld2(pre_d, "pre_d") != ldp:
            raise ValueError("td3v10_heads: pre_c and pre_d must have one shape and row stride")
        if uniform is None:
            raise ValueError("td3v10_heads: uniform [B, A] is needed (the Gumbel draw)")
    if not 1 <= A <= TD3_MAX_A:
        raise ValueError(f"td3v10_heads: A={A} outside [1, {TD3_MAX_A}]")
    if mode in (V10_ACT, V10_RANDOM) and (noise_c is None or noise_d is None):
        raise ValueError("td3v10_heads: noise_c and noise_d [B, A] are needed in this mode")
    _ba(noise_c, "noise_c", B, A)
    _ba(noise_d, "noise_d", B, A)
    _ba(uniform, "uniform", B, A)
    dev = noise_c.device if pre_c is None else pre_c.device
    c = torch.empty(B, A, dtype=torch.float32, device=dev)
    sm = torch.empty(B, A, dtype=torch.float32, device=dev) if want_softmax else None
    d = torch.empty(B, A, dtype=torch.float32, device=dev) if mode != V10_BEST else None
    ix = torch.empty(B, 1, dtype=torch.int64, device=dev) if want_index else None
    lib.ctr_td3v10_heads(B, A, mode, _p(pre_c), _p(pre_d), ldp, _p(noise_c), _p(noise_d),
                         _p(uniform), float(temperature), _p(c), _p(sm), _p(d), _p(ix), _stream())
    return dict(c_means=c, c_softmax=sm, d_action=d, d_index=ix)


def td3v10_rank_mask(d: torch.Tensor, c: torch.Tensor, *, noise=None, out_c=None, out_d=None,
                     want_keep: bool = True) -> dict:
    """The rank mask of the continuous actions under the discrete choice, one launch:
    dict(c [B, A], keep [B, A] uint8). Row b keeps column m when m is among the top
    argmax(d[b]) + 1 columns of c by value (ties: the lower index first); a kept element is
    clamp(c, -1, 1), or clamp(c + (0.2 noise + c), -1, 1) with noise, the others 0. out_c /
    out_d (one row stride): the c and d column blocks of a critic's input; out_d gets d."""
    ldd = _ld2(d, "d")
    B, A = d.shape
    ldc = _ld2(c, "c")
    if tuple(c.shape) != (B, A) or not 1 <= A <= TD3_MAX_A:
        raise ValueError(f"td3v10_rank_mask: d and c must be [B, A] with A in [1, {TD3_MAX_A}]")
    _ba(noise, "noise", B, A)
    if out_c is None:
        out_c = torch.empty(B, A, dtype=torch.float32, device=d.device)
    ldo = _ld2(out_c, "out_c")
    if tuple(out_c.shape) != (B, A):
        raise ValueError(f"td3v10_rank_mask: out_c must be [{B}, {A}]")
    if out_d is not None and (tuple(out_d.shape) != (B, A) or _ld2(out_d, "out_d") != ldo):
        raise ValueError(f"td3v10_rank_mask: out_d must be [{B}, {A}] with out_c's row stride")
    keep = torch.empty(B, A, dtype=torch.uint8, device=d.device) if want_keep else None
    lib.ctr_td3v10_rank_mask(B, A, _p(d), ldd, _p(c), ldc, _p(noise), _p(out_c), _p(out_d), ldo,
                             _p(keep), _stream())
    return dict(c=out_c, keep=keep)


def td3v10_heads_backward(g_c: torch.Tensor, g_d: torch.Tensor, keep: torch.Tensor,
                          c_means: torch.Tensor, d_q: torch.Tensor, d_soft: torch.Tensor,
                          temperature: float, reg: float):
    """The actor loss's gradients at the heads' pre-activations (d_pre_c, d_d_q) from the critic
    input's gradients of the c and d columns (include/ctr_hip.h), one launch."""
    ldg = _ld2(g_c, "g_c")
    B, A = g_c.shape
    if tuple(g_d.shape) != (B, A) or _ld2(g_d, "g_d") != ldg:
        raise ValueError("td3v10_heads_backward: g_c and g_d must have one shape and row stride")
    if not 1 <= A <= TD3_MAX_A:
        raise ValueError(f"td3v10_heads_backward: A={A} outside [1, {TD3_MAX_A}]")
    ldq = _ld2(d_q, "d_q")
    _dev(keep, "keep")
    if keep.dtype != torch.uint8 or tuple(keep.shape) != (B, A) or not keep.is_contiguous():
        raise ValueError(f"td3v10_heads_backward: keep must be contiguous uint8 [{B}, {A}]")
    _ba(c_means, "c_means", B, A)
    _ba(d_soft, "d_soft", B, A)
    if tuple(d_q.shape) != (B, A):
        raise ValueError(f"td3v10_heads_backward: d_q must be [{B}, {A}]")
    out = torch.empty(2, B, A, dtype=torch.float32, device=g_c.device)
    lib.ctr_td3v10_heads_backward(B, A, _p(g_c), _p(g_d), ldg, _p(keep), _p(c_means), _p(d_q),
                                  ldq, _p(d_soft), float(temperature), float(reg), _p(out[0]),
                                  _p(out[1]), _stream())
    return out[0], out[1]


_clip_ws: dict = {}  # (device index, stream, count) -> the partial sums' scratch


def clip_grad_norm_(grads, max_norm: float, norm_out: torch.Tensor | None = None) -> torch.Tensor:
    """torch's clip_grad_norm_ (2-norm) over a list of float32 device tensors in two launches,
    in place: the fp64 sum of squares in a fixed order, then every element times
    min(1, max_norm / (norm + 1e-6)). Returns the norm before clipping as a device scalar;
    nothing is copied to the host or to the device (the table travels as kernel arguments)."""
    grads = [g for g in grads if g is not None and g.numel()]
    if not 1 <= len(grads) <= GRAD_CLIP_MAX_TENSORS:
        raise ValueError(f"clip_grad_norm_: {len(grads)} tensors, outside "
                         f"[1, {GRAD_CLIP_MAX_TENSORS}]")
    table = (GradEntry * len(grads))()
    for i, g in enumerate(grads):
        _f32(g, "grad")
        table[i].grad, table[i].numel = g.data_ptr(), g.numel()
    dev = grads[0].device
    if any(g.device != dev for g in grads):
        raise ValueError("clip_grad_norm_: the tensors must be on one device")
    if norm_out is None:
        norm_out = torch.empty((), dtype=torch.float32, device=dev)
    _f32(norm_out, "norm_out")
    key = (dev.index, _stream(), len(grads))
    ws = _clip_ws.get(key)
    if ws is None:
        ws = _clip_ws[key] = torch.empty(lib.ctr_grad_clip_workspace_bytes(len(grads)),
                                         dtype=torch.uint8, device=dev)
    mx = max(g.numel() for g in grads)
    lib.ctr_grad_sumsq(len(grads), table, mx, _p(ws), ws.numel(), _stream())
    lib.ctr_grad_clip_scale(len(grads), table, mx, float(max_norm), _p(ws), ws.numel(),
                            _p(norm_out), _stream())
    return norm_out


def _v10_store_args(memory: torch.Tensor, prio2: torch.Tensor, transitions: torch.Tensor):
    _f32(memory, "memory")
    _f32(prio2, "prio2")
    if memory.dim() != 2 or tuple(prio2.shape) != (memory.shape[0], 2):
        raise ValueError("td3v10: memory must be [N, T] and prio2 [N, 2]")
    N, T = memory.shape
    _dev(transitions, "transitions")
    if transitions.dtype != torch.float32 or transitions.dim() != 2 or transitions.shape[1] != T:
        raise ValueError(f"td3v10: transitions must be float32 [n, {T}]")
    n = transitions.shape[0]
    if n > N:
        raise ValueError(f"td3v10: {n} transitions do not fit a memory of {N}")
    return N, T, n, (_ld2(transitions, "transitions") if n else T)


def td3v10_add(memory: torch.Tensor, prio2: torch.Tensor, start: int, transitions: torch.Tensor,
               td2: torch.Tensor) -> None:
    """v10 Memory.add: rows to slots (start + i) % N, both priority columns OVERWRITTEN by
    td2 [n, 2]. One launch."""
    N, T, n, ldt = _v10_store_args(memory, prio2, transitions)
    _f32(td2, "td2")
    if tuple(td2.shape) != (n, 2):
        raise ValueError(f"td3v10_add: td2 must be [{n}, 2]")
    lib.ctr_td3v10_store(N, T, start, n, _p(transitions), ldt, _p(td2), None, 0, _p(memory),
                         _p(prio2), None, _stream())


def td3v10_store_seeded(memory: torch.Tensor, prio2: torch.Tensor, start: int,
                        transitions: torch.Tensor, ws: torch.Tensor,
                        seed_out: torch.Tensor | None = None) -> None:
    """v10 store_transition in two launches of one entry point, nothing read back: the max of the WHOLE prio2
    (both columns, unfilled rows included), then the rows with priorities (1 if that max is 0
    else the max, the row's reward). ws: >= 4096 bytes of device scratch."""
    N, T, n, ldt = _v10_store_args(memory, prio2, transitions)
    _dev(ws, "ws")
    if ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < _V10_MAX_WS_BYTES:
        raise ValueError(f"td3v10_store_seeded: ws must hold {_V10_MAX_WS_BYTES} bytes (uint8)")
    if seed_out is not None:
        _f32(seed_out, "seed_out")
    if n == 0:
        return
    lib.ctr_td3v10_store(N, T, start, n, _p(transitions), ldt, None, _p(ws), ws.numel(),
                         _p(memory), _p(prio2), _p(seed_out), _stream())


def _v10_prio2(prio2: torch.Tensor, n_valid: int, who: str) -> int:
    _f32(prio2, "prio2")
    if prio2.dim() != 2 or prio2.shape[1] != 2 or not 0 <= n_valid <= prio2.shape[0]:
        raise ValueError(f"{who}: prio2 must be [N, 2] and n_valid within [0, N]")
    return prio2.shape[0]


def td3v10_keys(prio2: torch.Tensor, n_valid: int, eps: float, alpha: float, seed: int,
                out: torch.Tensor | None = None) -> torch.Tensor:
    """The selection keys of rows [0, n_valid) of the v10 memory, bitwise what td3v10_sample
    orders by: per_keys on (|prio2[:, 0]| + eps)^alpha, evaluated on the fly."""
    _v10_prio2(prio2, n_valid, "td3v10_keys")
    if out is None:
        out = torch.empty(n_valid, dtype=torch.float32, device=prio2.device)
    _f32(out, "keys")
    if out.numel() < n_valid:
        raise ValueError("td3v10_keys: out is shorter than n_valid")
    lib.ctr_td3v10_keys(n_valid, _p(prio2), float(eps), float(alpha), int(seed) & (2**64 - 1),
                        _p(out), _stream())
    return out


def td3v10_sample(memory: torch.Tensor, prio2: torch.Tensor, n_valid: int, k: int, seed: int,
                  beta: float, eps: float, alpha: float) -> dict:
    """per_sample's stochastic draw on the v10 memory: k distinct rows of the filled prefix by
    the priorities (|prio2[:, 0]| + eps)^alpha, which are computed where they are read (keys,
    minimum, isw) and never stored: dict(idx [k] int64, batch [k, T], isw [k, 1], min_p [1])."""
    _f32(memory, "memory")
    N = _v10_prio2(prio2, n_valid, "td3v10_sample")
    if memory.dim() != 2 or memory.shape[0] != N:
        raise ValueError("td3v10_sample: memory must be [N, T] beside prio2 [N, 2]")
    T = memory.shape[1]
    if not 1 <= k <= min(n_valid, PER_MAX_K):
        raise ValueError(f"td3v10_sample: k={k} outside [1, min(n_valid={n_valid}, {PER_MAX_K})]")
    dev = memory.device
    out = dict(idx=torch.empty(k, dtype=torch.int64, device=dev),
               batch=torch.empty(k, T, dtype=torch.float32, device=dev),
               isw=torch.empty(k, 1, dtype=torch.float32, device=dev),
               min_p=torch.empty(1, dtype=torch.float32, device=dev))
    key = (dev.index, _stream(), N, k)  # the select's scratch, shared with per_sample
    ws = _per_ws.get(key)
    if ws is None:
        ws = _per_ws[key] = torch.empty(lib.ctr_per_workspace_bytes(N, k), dtype=torch.uint8,
                                        device=dev)
    lib.ctr_td3v10_sample(N, T, n_valid, k, int(seed) & (2**64 - 1), float(beta), float(eps),
                          float(alpha), _p(memory), _p(prio2), _p(out["idx"]), _p(out["batch"]),
                          _p(out["isw"]), _p(out["min_p"]), _p(ws), ws.numel(), _stream())
    return out


def td3v10_update(prio2: torch.Tensor, idx: torch.Tensor, td: torch.Tensor) -> None:
    """v10 batch_update: prio2[idx, 0] = td, the raw signed error (duplicates: undefined)."""
    _f32(prio2, "prio2")
    _dev(idx, "idx")
    if prio2.dim() != 2 or prio2.shape[1] != 2:
        raise ValueError("td3v10_update: prio2 must be [N, 2]")
    if idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
        raise ValueError("td3v10_update: idx must be a contiguous int64 vector")
    _per_td(td, idx.numel())
    lib.ctr_td3v10_update(prio2.shape[0], idx.numel(), _p(idx), _p(td), _p(prio2), _stream())


def bn_eval_backward(dy: torch.Tensor, x: torch.Tensor, running_mean, running_var,
                     eps: float = 1e-5):
    """(dgamma, dbeta) of an eval-mode BatchNorm1d from dy, x [B, N] and the running
    statistics, one launch. The input's gradient is not computed."""
    lddy = _ld2(dy, "dy")
    B, N = dy.shape
    ldx = _ld2(x, "x")
    if tuple(x.shape) != (B, N):
        raise ValueError(f"bn_eval_backward: x must be [{B}, {N}]")
    _vecN(running_mean, "running_mean", N)
    _vecN(running_var, "running_var", N)
    out = torch.empty(2, N, dtype=torch.float32, device=dy.device)
    lib.ctr_bn_eval_backward(B, N, _p(dy), lddy, _p(x), ldx, _p(running_mean), _p(running_var),
                             float(eps), _p(out[0]), _p(out[1]), _stream())
    return out[0], out[1]


def ensemble_preds(preds: torch.Tensor, actions: torch.Tensor, prob_weights: torch.Tensor,
                   c_actions: torch.Tensor, labels: torch.Tensor):
    """generate_preds' arithmetic (hybrid_td3_main_per_v10.py:54-164) on [B, M] model pCTRs:
    returns (y_preds [B,1], rewards [B,1], return_c_actions [B,M])."""
    _f32(preds, "preds")
    B, M = preds.shape
    if preds.stride(1) != 1:
        preds = preds.contiguous()
    pw = _f32(prob_weights.reshape(B, M).contiguous(), "prob_weights")
    ca = _f32(c_actions.reshape(B, M).contiguous(), "c_actions")
    act, at = _idx(actions.reshape(B).contiguous(), "actions")
    lab, lt = _idx(labels.reshape(B).contiguous(), "labels")
    dev = preds.device
    y = torch.empty(B, 1, dtype=torch.float32, device=dev)
    r = torch.empty(B, 1, dtype=torch.float32, device=dev)
    rc = torch.empty(B, M, dtype=torch.float32, device=dev)
    rank = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    lib.ctr_ensemble_preds(_p(preds), B, M, preds.stride(0), _p(act), at, _p(pw), _p(ca),
                           _p(lab), lt, _p(y), _p(r), _p(rc), _p(rank), _stream())
    return y, r, rc


def ensemble_preds_ex(preds: torch.Tensor, actions: torch.Tensor, prob_weights: torch.Tensor,
                      labels: torch.Tensor, c_actions: torch.Tensor | None = None, *,
                      tie_rewards: bool = False, want_c_actions: bool = True):
    """ctr_ensemble_preds_ex: ensemble_preds with the base driver's options. c_actions=None:
    the softmax weights come from prob_weights (hybrid_td3_main_per.py:56-133); tie_rewards:
    a tie with the models' mean earns 1 (>= / <=). Returns (y_preds [B,1], rewards [B,1],
    return_c_actions [B,M] or None)."""
    _f32(preds, "preds")
    if preds.dim() != 2:
        raise ValueError("ensemble_preds_ex: preds must be [B, M]")
    B, M = preds.shape
    if not 1 <= M <= 32:
        raise ValueError(f"ensemble_preds_ex: M={M} models outside [1, 32]")
    pw = _f32(prob_weights.reshape(B, M).contiguous(), "prob_weights")
    ca = None if c_actions is None else _f32(c_actions.reshape(B, M).contiguous(), "c_actions")
    act, at = _idx(actions.reshape(B), "actions")
    lab, lt = _idx(labels.reshape(B), "labels")
    dev = preds.device
    y = torch.empty(B, 1, dtype=torch.float32, device=dev)
    r = torch.empty(B, 1, dtype=torch.float32, device=dev)
    rc = rank = None
    if want_c_actions:
        rc = torch.empty(B, M, dtype=torch.float32, device=dev)
        rank = torch.empty(max(B, 1), dtype=torch.int32, device=dev)
    lib.ctr_ensemble_preds_ex(_p(preds), B, M, M, _p(act), at, _p(pw),
                              _p(ca), _p(lab), lt, _p(y), _p(r), _p(rc), _p(rank),
                              CTR_ENSEMBLE_TIE_REWARDS if tie_rewards else 0, _stream())
    return y, r, rc


class FFMTables:
    """Device array of the F field tables' data pointers (ctr_ffm_* take `float* const*`);
    rebuilt when a table is re-allocated (Module.to(), load_state_dict into new storage)."""

    def __init__(self):
        self._key = None
        self.ptrs = None

    def get(self, tables) -> torch.Tensor:
        key = tuple(t.data_ptr() for t in tables)
        if key != self._key:
            for t in tables:
                _f32(t, "ffm table")
            self.ptrs = torch.tensor(key, dtype=torch.int64, device=tables[0].device)
            self._key = key
        return self.ptrs


def ffm_forward(idx, tables, ptrs, lin, bias, labels=None, mean_div=None, err_flag=None, out=None):
    """FFM logits z [B] (and with labels: p, per-example loss, dL/dz). out: a dict of this
    function's earlier result for the same B, written in place."""
    idx, it = _idx(idx)
    B, F = idx.shape
    V, K = tables[0].shape
    if len(tables) != F:
        raise ValueError(f"ffm_forward: {len(tables)} tables for {F} fields")
    dev = tables[0].device
    e = lambda: torch.empty(B, dtype=torch.float32, device=dev)  # noqa: E731
    if out is None:
        out = {"z": e()}
        if labels is not None:
            out.update(p=e(), loss_elem=e(), gz=e())
    z = out["z"]
    lib.ctr_ffm_forward(_p(idx), it, B, F, K, V, _p(ptrs), _p(lin), _p(bias), _p(z),
                        _p(labels), float(B if mean_div is None else mean_div), _p(out.get("p")),
                        _p(out.get("loss_elem")), _p(out.get("gz")), _p(err_flag), _stream())
    return out


def ffm_backward(idx, tables, ptrs, gz, keys=None, vals=None):
    """(keys int32 [B*F*(F-1)], vals [B*F*(F-1), K]): every example's table-row gradients
    (into keys / vals when given)."""
    idx, it = _idx(idx)
    B, F = idx.shape
    V, K = tables[0].shape
    n = B * F * (F - 1)
    if keys is None:
        keys = torch.empty(max(n, 1), dtype=torch.int32, device=gz.device)
    if vals is None:
        vals = torch.empty(max(n, 1), K, dtype=torch.float32, device=gz.device)
    if keys.numel() < n or vals.shape[0] < n or vals.shape[1] != K:
        raise ValueError("ffm_backward: keys / vals too small")
    lib.ctr_ffm_backward(_p(idx), it, B, F, K, V, _p(ptrs), _p(_f32(gz.contiguous(), "gz")),
                         _p(keys), _p(vals), _stream())
    return keys[:n], vals[:n]


def ffm_keys(idx, V: int, out=None, err_flag=None) -> torch.Tensor:
    """int32 [B*F*(F-1)]: the (table, row) keys t*V + x of ffm_backward, without values."""
    idx, it = _idx(idx)
    B, F = idx.shape
    n = B * F * (F - 1)
    if out is None:
        out = torch.empty(max(n, 1), dtype=torch.int32, device=idx.device)
    lib.ctr_ffm_keys(_p(idx), it, B, F, int(V), _p(out), _p(err_flag), _stream())
    return out[:n]


# ----------------------------------------------------------------------- REINFORCE ----
def softmax_rows(x: torch.Tensor) -> torch.Tensor:
    _f32(x, "x")
    out = torch.empty_like(x)
    lib.ctr_softmax_rows(_p(x), x.shape[0], x.shape[1], _p(out), _stream())
    return out


def pg_discount_norm(r: torch.Tensor, gamma: float, out32=None):
    """Returns (normalised returns fp64, the same as fp32, stats[mean, std] fp64); out32: a
    float32 [n] tensor to write the fp32 returns into."""
    r = _f32(r.reshape(-1).contiguous(), "rewards")
    n = r.numel()
    out = torch.empty(n, dtype=torch.float64, device=r.device)
    if out32 is None:
        out32 = torch.empty(n, dtype=torch.float32, device=r.device)
    elif (out32.dtype != torch.float32 or out32.numel() != n or not out32.is_contiguous()
          or out32.device != r.device):
        raise ValueError(f"pg_discount_norm: out32 must be a contiguous float32 [{n}] on {r.device}")
    stats = torch.empty(2, dtype=torch.float64, device=r.device)
    lib.ctr_pg_discount_norm(_p(r), n, float(gamma), _p(out), _p(out32), _p(stats), None, 0,
                             _stream())
    return out, out32, stats


def pg_loss_grad(probs: torch.Tensor, acts: torch.Tensor, vt: torch.Tensor, grad_scale=1.0):
    _f32(probs, "probs")
    acts = _dev(acts, "acts").reshape(-1).to(torch.int64).contiguous()
    vt = _f32(vt.reshape(-1).contiguous(), "vt")
    B, A = probs.shape
    loss = torch.empty(1, dtype=torch.float32, device=probs.device)
    dlogits = torch.empty_like(probs)
    lib.ctr_pg_loss_grad(_p(probs), _p(acts), _p(vt), B, A, float(grad_scale), _p(loss),
                         _p(dlogits), None, 0, _stream())
    return loss, dlogits


def pg_vt_mean(vt: torch.Tensor) -> torch.Tensor:
    """Device scalar mean(vt), summed in pg_loss_grad's order."""
    vt = _f32(vt.reshape(-1).contiguous(), "vt")
    out = torch.empty(1, dtype=torch.float32, device=vt.device)
    lib.ctr_pg_vt_mean(_p(vt), vt.numel(), _p(out), _stream())
    return out


def pg_loss_grad_global(probs: torch.Tensor, acts: torch.Tensor, vt_mean: torch.Tensor,
                        grad_scale=1.0):
    """pg_loss_grad for one rank's slice of a data-parallel episode (vt_mean = the
    episode-wide pg_vt_mean); the returned loss is this rank's share of the episode loss."""
    _f32(probs, "probs")
    _f32(vt_mean, "vt_mean")
    acts = _dev(acts, "acts").reshape(-1).to(torch.int64).contiguous()
    B, A = probs.shape
    loss = torch.empty(1, dtype=torch.float32, device=probs.device)
    dlogits = torch.empty_like(probs)
    lib.ctr_pg_loss_grad_global(_p(probs), _p(acts), B, A, _p(vt_mean), float(grad_scale),
                                _p(loss), _p(dlogits), _stream())
    return loss, dlogits
