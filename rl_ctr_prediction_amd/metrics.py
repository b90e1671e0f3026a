"""Evaluation metrics that stay on the device: exact ROC AUC, BCE loss and reward totals.

The reference's test() (all_main/pretrain_main.py:86-104) reads every batch on the host: one
``.item()`` for the loss, two ``.tolist()`` for the targets and predictions, then
``sklearn.metrics.roc_auc_score`` over Python lists. :class:`DeviceMetrics` is the device
counterpart of the trainers' ``read_loss_sum``: ``add`` appends a batch with one launch and no
host read, ``compute`` sorts and reduces the records (csrc/metrics.hip) and reads ONE small
state block. The AUC is exact: three integers U2, P, N with AUC = U2 / (2 P N), the
Mann-Whitney statistic with ties counted half — what sklearn's trapezoid equals up to its own
fp64 rounding. DESIGN.md §6f.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip_ops
from ._lib import CTR_METRICS_FLAG_LABEL, CTR_METRICS_FLAG_NAN, CTR_METRICS_FLAG_RANGE

__all__ = ["DeviceMetrics", "roc_auc_score", "TILE"]

TILE = hip_ops.METRICS_TILE  # records per sort / reduce tile

_FLAG_TEXT = (
    (CTR_METRICS_FLAG_NAN, "a prediction is NaN"),
    (CTR_METRICS_FLAG_LABEL, "a label is neither 0 nor 1"),
    (CTR_METRICS_FLAG_RANGE, "a prediction lies outside [0, 1] (the BCE loss needs "
                             "probabilities; pass with_loss=False for raw scores)"),
)
# sklearn's text (metrics/_ranking.py, _binary_roc_auc_score)
_ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."


class DeviceMetrics:
    """AUC / log loss / reward accumulator for up to `capacity` examples on `device`.

    add()      one launch per batch (two past 16384 examples), no host read of device data.
    compute()  sort + reduce, then one device-to-host copy of the 128-byte state block:
               dict(auc, loss, logloss, count, pos, neg, u2, batches, reward_sum) with
               loss = mean of the per-batch mean BCE (the reference's valid loss), logloss = the
               mean over all examples; both None when no batch was added with the loss.
    """

    def __init__(self, capacity: int, device="cuda:0", _records: torch.Tensor | None = None):
        device = torch.device(device)
        if device.type != "cuda":
            raise hip_ops.HostTensorError(
                f"DeviceMetrics on {device}: the HIP hot path needs a ROCm device (there is no "
                "CPU fallback)")
        self.capacity = int(capacity)
        nbytes = hip_ops.metrics_workspace_bytes(self.capacity)  # refuses a bad capacity
        # _records: a caller's buffer (tests place a guard region behind it)
        self.records = _records if _records is not None else \
            torch.empty(self.capacity, dtype=torch.int64, device=device)
        if self.records.numel() != self.capacity:
            raise ValueError("DeviceMetrics: _records must hold `capacity` words")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.state = torch.zeros(hip_ops.METRICS_STATE_WORDS, dtype=torch.int64, device=device)
        self.count = 0

    def reset(self) -> None:
        hip_ops.metrics_reset(self.state)
        self.count = 0

    def add(self, y_pred: torch.Tensor, labels: torch.Tensor, rewards: torch.Tensor | None = None,
            with_loss: bool = True) -> None:
        n = y_pred.numel() if isinstance(y_pred, torch.Tensor) else 0
        if self.count + n > self.capacity:
            raise ValueError(f"DeviceMetrics: {self.count} + {n} examples exceed the capacity "
                             f"{self.capacity}")
        self.count += hip_ops.metrics_append(self.records, self.count, y_pred, labels, rewards,
                                             with_loss, self.ws, self.state)

    def compute(self) -> dict:
        if self.count == 0:
            raise ValueError("DeviceMetrics.compute: no examples were added")
        hip_ops.metrics_auc(self.records, self.count, self.ws, self.state)
        host = self.state.cpu().numpy()  # the one device-to-host read
        flags = int(host[8:9].view(np.int32)[0])
        raised = [text for bit, text in _FLAG_TEXT if flags & bit]
        if raised:
            raise ValueError("DeviceMetrics: " + "; ".join(raised))
        u2, pos, neg = (int(v) for v in host[:3].view(np.uint64))
        loss_sum, nll_sum, reward_sum = (float(v) for v in host[3:6].view(np.float64))
        batches, loss_count = int(host[6]), int(host[7])
        assert pos + neg == self.count, (pos, neg, self.count)
        if pos == 0 or neg == 0:
            raise ValueError(_ONE_CLASS)
        return dict(auc=u2 / (2 * pos * neg),
                    loss=loss_sum / batches if batches else None,
                    logloss=nll_sum / loss_count if loss_count else None,
                    count=self.count, pos=pos, neg=neg, u2=u2, batches=batches,
                    reward_sum=reward_sum)


def roc_auc_score(targets: torch.Tensor, predicts: torch.Tensor) -> float:
    """sklearn.metrics.roc_auc_score(targets, predicts) for two device tensors of any shape
    with equal numel (binary 0/1 targets); returns a Python float."""
    for name, t in (("targets", targets), ("predicts", predicts)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor")
        if t.device.type != "cuda":
            raise hip_ops.HostTensorError(
                f"{name} is on {t.device}: the HIP hot path needs ROCm device tensors (there is "
                "no CPU fallback)")
    if targets.numel() != predicts.numel():
        raise ValueError(f"roc_auc_score: {targets.numel()} targets but {predicts.numel()} "
                         "predictions")
    if predicts.dtype != torch.float32:
        predicts = predicts.float()
    if targets.dtype not in (torch.float32, torch.int32, torch.int64):
        targets = targets.float() if targets.is_floating_point() else targets.long()
    if not predicts.is_contiguous():
        predicts = predicts.contiguous()
    m = DeviceMetrics(max(predicts.numel(), 1), predicts.device)
    m.add(predicts, targets.contiguous(), with_loss=False)
    return m.compute()["auc"]
