"""Test-side references of the hybrid TD3 ensemble driver (rl_ctr_prediction_amd.
hybrid_td3_main_per): a numpy restatement of the base driver's ``generate_preds``
(src/all_main/hybrid_td3_main_per.py:56-133), the loader of the recorded reference run
(tests/golden/make_golden_rl.py) and the rule that decides which recorded examples a parity
test may compare discretely (actions, rewards).

The margin rule. The reference's fp32 and fp64 runs differ by their own rounding (`gap`: the
largest element of |fp32 - fp64| of a quantity). A discrete outcome is compared only where the
decision behind it is clear of that rounding by a factor of 100:
  * the action (argmax of the d values):  top-two gap of the fp64 d values > 100 x gap(d values)
  * the model order (sort of the weights): smallest gap between adjacent sorted fp64
    prob_weights > 100 x gap(prob_weights)
  * the reward (y against the models' mean): |y - mean| in fp64 > 100 x max(gap(y), gap(mean)),
    the gaps taken over the examples the first two rules keep.
At most 2 % of the examples of a batch may be left out (MAX_DROPPED).
"""
from __future__ import annotations

from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
MARGIN = 100.0
MAX_DROPPED = 0.02
SEED_MODELS, SEED_AGENT = 11, 0   # torch.manual_seed before the three models / the agent
SCALE = 0.1                       # the seeded models' tables are multiplied by this
K, ACTIONS = 4, 3
TRAIN_BATCH, TEST_BATCH, MEMORY = 256, 64, 1024
FILES = ["g_rl_driver.npz", "g_rl_driver_b.npz", "g_rl_driver_c.npz"]


def load(names=FILES):
    out = {}
    for n in names:
        with np.load(GOLDEN / n, allow_pickle=False) as z:
            out.update({k: z[k] for k in z.files})
    return out


def softmax32(x):
    """torch.softmax of a float32 row: max-shifted exp, then a division by the sum."""
    e = np.exp((x - x.max()).astype(np.float32)).astype(np.float32)
    s = np.float32(0)
    for v in e:
        s = np.float32(s + v)
    return (e / s).astype(np.float32)


def generate_preds_base(preds, actions, prob_weights, labels):
    """(y [B], rewards [B]) of the base driver's generate_preds in float32, example by example.
    preds [B, M] are the models' pCTRs. The reference's three branches are one: the a models of
    the largest weights (a stable descending sort), combined with the softmax of those weights —
    for a == 1 that weight is exactly 1, for a == M the weights themselves are used unsorted.
    Reward 1 where y >= the models' mean on a click and y <= it on a non-click (a tie earns 1);
    an action outside 1..M leaves y = 1 and reward = 1."""
    preds = np.asarray(preds, dtype=np.float32)
    pw = np.asarray(prob_weights, dtype=np.float32)
    act = np.asarray(actions).reshape(-1)
    lab = np.asarray(labels).reshape(-1)
    B, M = preds.shape
    y = np.ones(B, dtype=np.float32)
    r = np.ones(B, dtype=np.float32)
    for b in range(B):
        a = int(act[b])
        if not 1 <= a <= M:
            continue
        if a == M:
            acc = np.float32(0)
            for m in range(M):
                acc = np.float32(acc + np.float32(pw[b, m] * preds[b, m]))
        else:
            order = np.argsort(-pw[b], kind="stable")[:a]
            w = softmax32(pw[b, order])
            acc = np.float32(0)
            for m in range(a):
                acc = np.float32(acc + np.float32(w[m] * preds[b, order[m]]))
        y[b] = acc
        s = np.float32(0)
        for m in range(M):
            s = np.float32(s + preds[b, m])
        mean = np.float32(s / np.float32(M))
        if lab[b] == 1:
            r[b] = 1.0 if acc >= mean else 0.0
        elif lab[b] == 0:
            r[b] = 1.0 if acc <= mean else 0.0
    return y, r


def _gap(a32, a64, rows=None):
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    if rows is not None:
        a32, a64 = a32[rows], a64[rows]
    return float(np.max(np.abs(a32 - a64))) if a64.size else 0.0


def top2_gap(d):
    s = np.sort(np.asarray(d, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


def min_sorted_gap(w):
    s = np.sort(np.asarray(w, dtype=np.float64), axis=1)
    return np.min(np.diff(s, axis=1), axis=1)


def keep_masks(g, tag):
    """(keep_action, keep_y, keep_reward), each [B], of the recorded batch `tag` (its arrays
    g[tag/...] and g[f64/tag/...]): the examples whose action, whose action and model order (so
    whose y is one quantity in both runs), and whose reward may be compared; see the module
    docstring."""
    f = lambda k: g[f"{tag}/{k}"]          # noqa: E731
    d = lambda k: g[f"f64/{tag}/{k}"]      # noqa: E731
    keep_a = top2_gap(d("d_values")) > MARGIN * _gap(f("d_values"), d("d_values"))
    keep_w = min_sorted_gap(d("prob_weights")) > MARGIN * _gap(f("prob_weights"),
                                                              d("prob_weights"))
    keep = keep_a & keep_w
    mean32 = np.asarray(f("preds"), dtype=np.float64).mean(1)
    mean64 = np.asarray(d("preds"), dtype=np.float64).mean(1)
    y32, y64 = f("y").reshape(-1), d("y").reshape(-1)
    gy = max(_gap(y32, y64, keep), _gap(mean32, mean64, keep))
    keep_r = keep & (np.abs(y64.astype(np.float64) - mean64) > MARGIN * gy)
    return keep_a, keep, keep_r
