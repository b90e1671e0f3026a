"""CPU checks of tests/adam_refs.py (the float64 reference and the slack model of the Adam
GPU tests) against torch.optim.Adam: a reference that nothing checks is only a second
implementation."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import adam_refs as A

LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8


def _state(R, K, seed, dtype=np.float64):
    """p ~ 0.05 N, m ~ 1e-4 N, v ~ 1e-8 U: a table in the middle of training, one element
    all zero."""
    rng = np.random.default_rng(seed)
    p = (0.05 * rng.standard_normal((R, K))).astype(dtype)
    m = (1e-4 * rng.standard_normal((R, K))).astype(dtype)
    v = (1e-8 * rng.random((R, K))).astype(dtype)
    p[0, 0] = m[0, 0] = v[0, 0] = 0
    return p, m, v


def _torch_adam(p0, m0, v0, grads, wd, dtype):
    """torch.optim.Adam (single-tensor, coupled L2) from the state (p0, m0, v0, step 0) over
    the dense gradients grads[0..T-1]; the (p, m, v) snapshots after 0..T steps."""
    p = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
    opt = torch.optim.Adam([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, foreach=False)
    opt.state[p] = dict(step=torch.tensor(0.0), exp_avg=torch.tensor(m0, dtype=dtype),
                        exp_avg_sq=torch.tensor(v0, dtype=dtype))
    snap = [(np.array(p0), np.array(m0), np.array(v0))]
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        opt.step()
        st = opt.state[p]
        snap.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(),
                     st["exp_avg_sq"].numpy().copy()))
    return snap


def test_scalars_are_hip_ops():
    from rl_ctr_prediction_amd import hip_ops
    for t in (1, 2, 5, 64, 1000, 8192):
        assert A.adam_scalars64(t, LR, BETAS) == hip_ops.adam_scalars(t, LR, BETAS)


@pytest.mark.parametrize("wd", [0.0, 1e-5])
def test_reference_equals_torch_adam_float64(wd):
    """Seven dense float64 torch steps, the gradient zero except at step 7 on some rows (an
    absent row has a zero gradient). The table handed to the reference has row r taken from
    the snapshot after last[r] steps — rows of mixed staleness — and must come out as the
    snapshot after 6 steps (catch-up), after 7 (catch-up + apply), or untouched."""
    R, K, T = 11, 5, 7
    p0, m0, v0 = _state(R, K, 3)
    rng = np.random.default_rng(4)
    rows = np.array([9, 2, 0, 5, 6])  # the rows step 7 touches, in no order
    grows = 0.01 * rng.standard_normal((rows.size, K))
    grows[2, 0] = 0.0  # row 0's all-zero element keeps a zero gradient
    grads = [np.zeros((R, K)) for _ in range(T)]
    grads[T - 1][rows] = grows
    snap = _torch_adam(p0, m0, v0, grads, wd, torch.float64)
    last = np.array([0, 1, 2, 3, 4, 5, 6, 6, 0, 3, 5])
    mixed = [np.stack([snap[last[r]][i][r] for r in range(R)]) for i in range(3)]

    def close(got, want, what):
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300, err_msg=what)

    out = A.adam_replay64(*mixed, last, T - 1, LR, BETAS, EPS, wd)
    for i, k in enumerate("pmv"):
        close(out[k], snap[T - 1][i], f"catch-up {k}")
    assert (out["last"] == T - 1).all()
    assert out["p"][0, 0] == 0 and out["m"][0, 0] == 0 and out["v"][0, 0] == 0
    assert out["slack_p"][0, 0] == 0 and out["slack_m"][0, 0] == 0 and out["slack_v"][0, 0] == 0
    cur = last == T - 1  # current rows: untouched, no slack
    for i, k in enumerate("pmv"):
        assert (out[k][cur] == mixed[i][cur]).all() and (out["slack_" + k][cur] == 0).all()

    # catch-up + apply on the touched rows only; the others stay exactly as handed in
    out = A.adam_replay64(*mixed, last, T - 1, LR, BETAS, EPS, wd, grads=grows, rows=rows)
    rest = np.setdiff1d(np.arange(R), rows)
    for i, k in enumerate("pmv"):
        close(out[k][rows], snap[T][i][rows], f"apply {k}")
        assert (out[k][rest] == mixed[i][rest]).all(), k
    assert (out["last"][rows] == T).all() and (out["last"][rest] == last[rest]).all()

    # a target in the middle: rows at or past it are untouched, the others reach it
    out = A.adam_replay64(*mixed, last, 3, LR, BETAS, EPS, wd)
    ahead = last >= 3
    for i, k in enumerate("pmv"):
        assert (out[k][ahead] == mixed[i][ahead]).all(), k
        close(out[k][~ahead], snap[3][i][~ahead], f"target 3 {k}")
    assert (out["last"] == np.maximum(last, 3)).all()

    # the dense form (no rows): every row takes step 7, absent rows with a zero gradient
    out = A.adam_replay64(*mixed, last, T - 1, LR, BETAS, EPS, wd, grads=grads[T - 1])
    for i, k in enumerate("pmv"):
        close(out[k], snap[T][i], f"dense apply {k}")


@pytest.mark.parametrize("wd", [0.0, 1e-5])
@pytest.mark.parametrize("T", [1, 7, 70, 300])
def test_torch_float32_lies_inside_the_slack(T, wd):
    """The bound model: torch's own fp32 CPU Adam — T-1 zero-gradient steps, then one with a
    gradient — stays inside the slack around the float64 reference started from the same fp32
    state (as AdamBound.check does with its `desired`)."""
    R, K = 129, 64
    p0, m0, v0 = _state(R, K, 10 + T, np.float32)
    g = A.grad_like(m0, v0, np.random.default_rng(T))  # see there: what the model covers
    assert g[0, 0] == 0.0 and g.dtype == np.float32 and (np.sign(g) == np.sign(m0)).all()
    grads = [np.zeros((R, K), np.float32)] * (T - 1) + [g]
    snap = _torch_adam(p0, m0, v0, grads, wd, torch.float32)
    ref = A.adam_replay64(p0, m0, v0, np.zeros(R, int), T - 1, LR, BETAS, EPS, wd, grads=g)
    for i, k in enumerate("pmv"):
        ok = A.inside(snap[T][i], ref[k], ref["slack_" + k])
        err = np.abs(snap[T][i].astype(np.float64) - ref[k])
        worst = float(np.max(err / np.maximum(ref["slack_" + k], 1e-300)))
        assert ok.all(), (k, T, wd, worst)
    assert snap[T][0][0, 0] == 0 and ref["slack_p"][0, 0] == 0
    if T > 1:  # and the catch-up alone
        ref = A.adam_replay64(p0, m0, v0, np.zeros(R, int), T - 1, LR, BETAS, EPS, wd)
        for i, k in enumerate("pmv"):
            assert A.inside(snap[T - 1][i], ref[k], ref["slack_" + k]).all(), (k, T, wd)
