"""The float64 reference of the Adam kernels (csrc/adam.hip, csrc/adam_common.h and the fused
apply of csrc/sparse_grad.hip), for tests/test_gpu_adam_family.py, numpy only.
tests/test_adam_refs.py checks it on the CPU against torch.optim.Adam, so the GPU tests
compare the kernels with a reference that something else has checked.

The operation: torch.optim.Adam(lr, betas, eps, weight_decay) — coupled L2 — on a table whose
rows are not all current. Row r is current to step last[r]; a step it took no part in has the
gradient g = wd * p (torch's dense Adam with a zero gradient), a function of the row alone, so
the row is brought forward by replaying steps last[r]+1 .. target, and may then take step
target+1 with a given gradient.

Beside every value a slack is accumulated, one term per replayed or applied step: what an
fp32 evaluation of the same recurrences (any operation order, fused or not, hardware sqrt and
reciprocal) may differ by.

* p: 2^-22 |p| + 2^-20 |u| per step, u the step taken — conftest.AdamBound's constants (the
  parameter's store rounding, and the ~6 dependent roundings of the step).
* m: 3 * 2^-24 * e_m per step, with e_m <- max(beta1 e_m + (1 - beta1)|g|, |m|), e_m(0) = |m0|:
  three roundings a step (g, g - m, the fma) against the magnitudes summed, not against m
  itself, because g - m cancels.
* v: 4 * 2^-24 * v per step (the products g*g, w2*(g*g), beta2*v and the sum; a plain fp32
  numpy emulation of the kernel's order reaches 0.72 of this bound at factor 3, hence 4).

These constants are the test's bar; they are not fitted to what the kernels give.
"""
from __future__ import annotations

import numpy as np

U24 = 2.0 ** -24


def adam_scalars64(step: int, lr: float, betas=(0.9, 0.999)) -> tuple[float, float]:
    """step_size and sqrt(bias_correction2) in python doubles, as torch/optim/adam.py and
    hip_ops.adam_scalars compute them (test_adam_refs.py asserts the two are equal)."""
    beta1, beta2 = betas
    return lr / (1 - beta1 ** step), (1 - beta2 ** step) ** 0.5


def _lr_at(tab_lr, t: int) -> float:
    return float(tab_lr) if np.ndim(tab_lr) == 0 else float(np.asarray(tab_lr)[t])


def adam_replay64(p, m, v, last, target, tab_lr, betas, eps, wd, grads=None, rows=None) -> dict:
    """p, m, v [R, ...] (any trailing shape), last [R] int. Replays steps last[r]+1 .. target
    on every row r (of `rows`, an index array, when given) with g = wd * p; rows with
    last[r] >= target are returned untouched. grads (the table's shape; with `rows`, one
    gradient row per entry of rows, in that order): those rows then take step target+1 with
    that gradient, and their last becomes target+1. tab_lr: the learning rate, a scalar or an array indexed by the step.

    Returns float64 p, m, v, the new last, and slack_p / slack_m / slack_v (see the module
    docstring): zero on every element no step touched."""
    p = np.array(p, dtype=np.float64)
    m = np.array(m, dtype=np.float64)
    v = np.array(v, dtype=np.float64)
    last = np.array(last, dtype=np.int64).reshape(-1)
    R = p.shape[0]
    assert m.shape == p.shape and v.shape == p.shape and last.shape == (R,)
    target = int(target)
    b1, b2 = betas
    bshape = (R,) + (1,) * (p.ndim - 1)
    sel = np.zeros(R, dtype=bool)
    if rows is None:
        sel[:] = True
    else:
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        assert np.unique(rows).size == rows.size, "rows must be unique"
        sel[rows] = True
    sp, sm, sv = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    e_m = np.abs(m)

    def step(t, g, mask):
        """One Adam step t on the rows of mask (bool [R]) with gradient g (before decay)."""
        nonlocal p, m, v, sp, sm, sv, e_m
        k = mask.reshape(bshape)
        step_size, bc2_sqrt = adam_scalars64(t, _lr_at(tab_lr, t), betas)
        gd = g + wd * p                                  # grad.add(param, alpha=wd)
        mn = m + (1 - b1) * (gd - m)                     # exp_avg.lerp_(grad, 1 - beta1)
        vn = b2 * v + (1 - b2) * gd * gd                 # mul_(beta2).addcmul_(g, g, 1-beta2)
        u = step_size * mn / (np.sqrt(vn) / bc2_sqrt + eps)
        pn = p - u                                       # addcdiv_(exp_avg, denom, -step_size)
        en = np.maximum(b1 * e_m + (1 - b1) * np.abs(gd), np.abs(mn))
        sp = np.where(k, sp + 2.0 ** -22 * np.abs(pn) + 2.0 ** -20 * np.abs(u), sp)
        sm = np.where(k, sm + 3 * U24 * en, sm)
        sv = np.where(k, sv + 4 * U24 * vn, sv)
        p, m, v, e_m = np.where(k, pn, p), np.where(k, mn, m), np.where(k, vn, v), \
            np.where(k, en, e_m)

    new_last = last.copy()
    stale = sel & (last < target)
    if stale.any():
        zero = np.zeros_like(p)
        for t in range(int(last[stale].min()) + 1, target + 1):
            step(t, zero, stale & (last < t))
        new_last[stale] = target
    if grads is not None:
        g = np.asarray(grads, dtype=np.float64)
        if rows is not None:  # one gradient row per entry of rows, in that order
            assert g.shape == (rows.size,) + p.shape[1:], (g.shape, rows.size, p.shape)
            full = np.zeros_like(p)
            full[rows] = g
            g = full
        assert g.shape == p.shape
        assert (last[sel] <= target).all(), "apply: a row is ahead of the step before"
        step(target + 1, g, sel)
        new_last[sel] = target + 1
    return dict(p=p, m=m, v=v, last=new_last, slack_p=sp, slack_m=sm, slack_v=sv)


def grad_like(m, v, rng) -> np.ndarray:
    """A gradient consistent with the moments it meets: g = sign(m) * sqrt(v) * (0.5 + U),
    as in a table in the middle of training, where m ~ E[g] and v ~ E[g^2] (fp32). Zero where
    m or v is zero.

    Why not any gradient: the slack above is a model of steps whose gradient neither cancels
    m nor dwarfs sqrt(v) — every replayed step (g = wd * p) is one. Under a gradient that
    cancels m down to a small fraction of the magnitudes summed, the step u inherits m's
    absolute rounding error as a large relative one, which the p term (2^-20 |u|) does not
    cover; and where (1 - beta2) g^2 dominates v, the rounding of g + wd * p counts twice in
    v. torch's own fp32 CPU Adam then leaves the slack: measured over 4.2M elements from the
    state of the GPU tests with one applied step of g ~ s * N(0, 1), elements outside / worst
    error : slack were, for p, 2-25 / 9.6 (s = 1e-2), 13-79 / 13.6 (1e-3), 0-4 / 4.6 (1e-4);
    for v, up to 362 / 1.15 (s = 1e-2), 5 / 1.11 (1e-3); for m, 1 / 1.14 (1e-4) — a few per
    million. With grad_like gradients the same runs gave 0 outside and worst ratios 0.33 (p),
    0.87 (m), 0.55 (v). The bar is not widened; the applied gradients of the tests are drawn
    where the bar is a valid statement about a correct fp32 Adam."""
    m, v = np.asarray(m), np.asarray(v)
    g = np.sign(m) * np.sqrt(v.astype(np.float64)) * (0.5 + rng.random(m.shape))
    return g.astype(np.float32)


def inside(got, ref, slack) -> np.ndarray:
    """Elementwise: |got - ref| <= slack (float64)."""
    return np.abs(np.asarray(got, dtype=np.float64) - ref) <= slack
