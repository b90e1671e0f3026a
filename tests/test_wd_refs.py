"""The float64 W&D references (tests/wd_refs.py) against the reference implementation's own run
(tests/golden/g_wd*.npz, make_golden_wd.py). CPU only: no kernel is launched here."""
from __future__ import annotations

import numpy as np
import pytest

import wd_refs as R
from conftest import load_golden


def _params(g, head="init"):
    return {k: g[f"{head}/{k}"].astype(np.float64) for k in R.KEYS}


def test_refs_match_the_reference_run():
    """p0 at the bar of test_opnn_refs.py (rtol 1e-5, atol 1e-7), the loss to rel 1e-5, every
    gradient within rtol 1e-5, atol 1e-6 * max|ref|."""
    g = load_golden("g_wd.npz")
    loss, p, gr, _ = R.grads(_params(g), g["x0"], g["y0"])
    np.testing.assert_allclose(p, g["p0"], rtol=1e-5, atol=1e-7)
    assert loss == pytest.approx(float(g["loss0"]), rel=1e-5)
    for k in R.KEYS:
        ref = g[f"grad0/{k}"]
        np.testing.assert_allclose(gr[k].reshape(ref.shape), ref, rtol=1e-5,
                                   atol=1e-6 * max(np.abs(ref).max(), 1e-12), err_msg=k)


def test_the_wide_part_is_visible_in_the_fixture():
    """The fixture does what it is for: without the linear term, or without the bias, the
    predictions are outside the bar."""
    g = load_golden("g_wd.npz")
    for k in ("linear.weight", "bias"):
        params = _params(g)
        params[k] = np.zeros_like(params[k])
        assert not np.allclose(R.model(params, g["x0"]), g["p0"], rtol=1e-5, atol=1e-7), k


def test_parts_agree_with_the_whole():
    """flat, z_lin and row_sums are what grads composes; the scales dominate their values."""
    rng = np.random.default_rng(5)
    V, F, K, B = 30, 4, 3, 9
    E, lin, bias = rng.normal(size=(V, K)), rng.normal(size=(V, 1)), rng.normal(size=1)
    x = rng.integers(0, V, size=(B, F))
    x[:, 0] = 2
    np.testing.assert_array_equal(R.flat(E, x)[3, K:2 * K], E[x[3, 1]])
    z = R.z_lin(lin, bias, x)
    assert z[4] == pytest.approx(bias[0] + sum(lin[i, 0] for i in x[4]), rel=1e-14)
    assert (np.abs(z) <= R.z_lin_scale(lin, bias, x) * (1 + 1e-12)).all()
    gz, dx = rng.normal(size=B), rng.normal(size=(B, F * K))
    g_emb, g_lin, c_emb, c_lin = R.row_sums(x, V, gz, dx)
    assert g_lin[2] == pytest.approx(gz.sum() + sum(gz[b] for b in range(B)
                                                    for f in range(1, F) if x[b, f] == 2))
    want = sum(dx[b, f * K:(f + 1) * K] for b in range(B) for f in range(F) if x[b, f] == 2)
    np.testing.assert_allclose(g_emb[2], want, rtol=1e-13)
    assert (np.abs(g_emb) <= c_emb * (1 + 1e-12)).all() and (np.abs(g_lin) <= c_lin + 1e-300).all()
    untouched = np.setdiff1d(np.arange(V), x.reshape(-1))
    assert not g_emb[untouched].any() and not g_lin[untouched].any()
