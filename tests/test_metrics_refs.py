"""CPU anchors of tests/metrics_refs.py (the reference the GPU metric tests compare with):
its exact-integer AUC against sklearn.metrics.roc_auc_score, its BCE against torch's BCELoss
in float64."""
from __future__ import annotations

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score

import metrics_refs as R


def _case(n, levels, pos_rate, seed):
    rng = np.random.default_rng(seed)
    p = rng.random(n).astype(np.float32)
    if levels:
        p = (np.floor(p * levels) / levels).astype(np.float32)
    y = (rng.random(n) < pos_rate).astype(np.float32)
    y[0], y[1] = 0.0, 1.0  # both classes present
    return p, y


# sklearn accumulates its trapezoid in fp64 (worst deviation measured from this formula:
# 1.1e-16 for n <= 300,001); the bar is abs 1e-12
@pytest.mark.parametrize("n", [2, 65, 4097, 300001])
@pytest.mark.parametrize("levels", [0, 3, 4, 4096])
@pytest.mark.parametrize("pos_rate", [0.5, 0.02])
def test_auc_matches_sklearn(n, levels, pos_rate):
    p, y = _case(n, levels, pos_rate, seed=n + levels)
    u2, P, N = R.auc_counts(p, y)
    assert P == int(y.sum()) and P + N == n
    assert isinstance(u2, int) and 0 <= u2 <= 2 * P * N
    assert abs(u2 / (2 * P * N) - roc_auc_score(y, p)) <= 1e-12


def test_signed_zeros_tie():
    """sklearn ties -0.0 and +0.0; keys taken from the raw bits would not (0.25 here)."""
    p = np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    y = np.array([1, 0, 0, 1], dtype=np.float32)
    assert R.auc_counts(p, y) == (4, 2, 2)
    assert R.auc(p, y) == 0.5 == roc_auc_score(y, p)
    r = R.records(p, np.zeros(4))
    assert len(set(r.tolist())) == 1


def test_order_of_negative_and_large_scores():
    p = np.array([-3.5, -1e-30, 0.0, 1e-30, 0.5, 1.0, 2.0, np.inf, -np.inf], dtype=np.float32)
    r = R.records(p, np.zeros(p.size)) >> np.uint64(1)
    assert np.array_equal(np.argsort(r, kind="stable"), np.argsort(p, kind="stable"))
    y = np.array([0, 1, 0, 1, 0, 1, 1], dtype=np.float32)
    p = p[:7]  # sklearn refuses infinities
    assert abs(R.auc(p, y) - roc_auc_score(y, p)) <= 1e-12


def test_exact_extremes():
    p = np.full(1000, 0.25, dtype=np.float32)
    y = (np.arange(1000) % 3 == 0).astype(np.float32)
    u2, P, N = R.auc_counts(p, y)
    assert u2 == P * N and R.auc(p, y) == 0.5
    p = np.linspace(0.1, 0.9, 1000).astype(np.float32)
    y = np.zeros(1000, dtype=np.float32)
    y[-1] = 1
    assert R.auc(p, y) == 1.0
    y[-1], y[0] = 0, 1
    assert R.auc(p, y) == 0.0


@pytest.mark.parametrize("n", [1, 7, 4096, 100003])
def test_bce_matches_torch_float64(n):
    p, y = _case(max(n, 2), 0, 0.3, seed=n)
    p, y = p[:n], y[:n]
    if n > 4:
        p[2], p[3] = 0.0, 1.0  # the -100 clamp, both ways
        y[2], y[3] = 1.0, 0.0
    pt, yt = torch.from_numpy(p).double(), torch.from_numpy(y).double()
    want = torch.nn.BCELoss(reduction="none")(pt, yt).numpy()
    got = R.bce_terms(p, y)
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
    s = R.bce_sums(p, y)
    assert s["logloss"] == pytest.approx(float(torch.nn.BCELoss()(pt, yt)), rel=1e-12)
    if n > 4:
        assert got[2] == 100.0 and got[3] == 100.0


def test_mean_of_batch_means():
    p, y = _case(8199, 0, 0.3, seed=5)
    sizes = [1, 4095, 4096, 7]
    s = R.bce_sums(p, y, sizes)
    loss = torch.nn.BCELoss()
    pt, yt = torch.from_numpy(p).double(), torch.from_numpy(y).double()
    means, o = [], 0
    for b in sizes:
        means.append(float(loss(pt[o:o + b], yt[o:o + b])))
        o += b
    assert s["batches"] == 4
    assert s["loss"] == pytest.approx(sum(means) / 4, rel=1e-12)
    assert s["loss"] != pytest.approx(s["logloss"], rel=1e-6)  # uneven batches: not the mean
