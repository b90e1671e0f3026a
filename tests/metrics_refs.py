"""Plain numpy restatement of csrc/metrics.hip, for tests/test_gpu_metrics.py: the same 64-bit
records (key << 1) | label, sorted with np.sort, reduced to the integers (U2, P, N) in Python
ints, and the BCE sums in float64. tests/test_metrics_refs.py anchors it on the CPU to
sklearn.metrics.roc_auc_score and to torch's BCELoss in float64, so the GPU tests compare the
kernels with a reference that something else has checked."""
from __future__ import annotations

import numpy as np
import torch


def _np(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def records(pred, labels) -> np.ndarray:
    """uint64 records: key = order-preserving uint32 image of the fp32 bits of pred + 0.0f (the
    sum makes -0.0 and +0.0 one key), label in bit 0."""
    p = _np(pred).astype(np.float32).reshape(-1) + np.float32(0.0)
    b = p.view(np.uint32)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint64)
    y = (_np(labels).reshape(-1) == 1).astype(np.uint64)
    return (key << np.uint64(1)) | y


def auc_counts(pred, labels) -> tuple[int, int, int]:
    """(U2, P, N): U2 = sum over positives of (2 x negatives with a smaller prediction +
    negatives with an equal one), as Python ints; AUC = U2 / (2 P N)."""
    r = np.sort(records(pred, labels))
    key, y = r >> np.uint64(1), (r & np.uint64(1)).astype(np.int64)
    n = r.size
    neg_before = np.concatenate([[0], np.cumsum(1 - y)])[:n]      # negatives at positions < i
    start = np.ones(n, dtype=bool)
    start[1:] = key[1:] != key[:-1]
    run_first = np.maximum.accumulate(np.where(start, np.arange(n), 0))  # start of i's run
    s = neg_before[run_first]                                     # negatives below the run
    pos = y == 1
    # inside a run the negatives sort first, so neg_before[i] - s[i] = the run's negatives
    # int64 is exact here: U2 <= 2 P N < 2^63 for n < 2^31
    u2 = int(np.sum(neg_before[pos].astype(np.int64) + s[pos].astype(np.int64)))
    P = int(pos.sum())
    return u2, P, n - P


def auc(pred, labels) -> float:
    u2, P, N = auc_counts(pred, labels)
    return u2 / (2 * P * N)


def bce_terms(pred, labels) -> np.ndarray:
    """Per-example -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) in float64, log of
    the fp32 p taken in double (torch's clamp)."""
    p = _np(pred).astype(np.float32).reshape(-1).astype(np.float64)
    y = _np(labels).reshape(-1).astype(np.float64)
    with np.errstate(divide="ignore"):
        lp = np.maximum(np.log(p), -100.0)
        l1p = np.maximum(np.log(1.0 - p), -100.0)
    return -(y * lp + (1.0 - y) * l1p)


def bce_sums(pred, labels, batch_sizes=None) -> dict:
    """nll_sum (all examples), logloss (their mean), and over the batches cut by batch_sizes
    (default: one batch) loss_sum = sum of batch means and loss = their mean."""
    t = bce_terms(pred, labels)
    sizes = [t.size] if batch_sizes is None else list(batch_sizes)
    assert sum(sizes) == t.size
    means, o = [], 0
    for s in sizes:
        means.append(float(np.sum(t[o:o + s])) / s)
        o += s
    loss_sum = float(np.sum(means))
    return dict(nll_sum=float(np.sum(t)), logloss=float(np.sum(t)) / t.size, loss_sum=loss_sum,
                loss=loss_sum / len(sizes), batches=len(sizes))
