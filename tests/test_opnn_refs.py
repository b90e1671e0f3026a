"""The float64 OPNN references (tests/opnn_refs.py) against the reference implementation's own
run (tests/golden/g_opnn*.npz, make_golden_opnn.py). CPU only: no kernel is launched here."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import opnn_refs as R
from conftest import load_golden


def _params(g):
    return {k: torch.tensor(g[f"init/{k}"]).double().requires_grad_(True) for k in R.KEYS}


@pytest.mark.parametrize("fixture", ["g_opnn.npz", "g_opnn_kernel.npz"])
def test_refs_match_the_reference_run(fixture):
    """p0 at the bar of test_autograd_ipnn_grads_vs_reference (rtol 1e-5, atol 1e-7), every
    gradient within rtol 1e-5, atol 1e-6 * max|ref|; the second fixture has a non-symmetric
    kernel (a row sum taken for the column sum fails there)."""
    g0 = load_golden("g_opnn.npz")
    g = load_golden(fixture)
    K = g0["init/feature_embedding.weight"].shape[1]
    kernel = torch.tensor(g["kernel"]) if "kernel" in g.files else torch.ones(K, K)
    if "kernel" in g.files:
        assert not np.array_equal(g["kernel"], g["kernel"].T)
    x, y = torch.tensor(g0["x0"]), torch.tensor(g0["y0"])
    loss, p, gr = R.grads(_params(g0), x, y, kernel)
    np.testing.assert_allclose(p.numpy(), g["p0"], rtol=1e-5, atol=1e-7)
    assert float(loss) == pytest.approx(float(g["loss0"]), rel=1e-5)
    for k in R.KEYS:
        ref = g[f"grad0/{k}"]
        np.testing.assert_allclose(gr[k].numpy(), ref, rtol=1e-5,
                                   atol=1e-6 * max(np.abs(ref).max(), 1e-12), err_msg=k)


def test_a_row_sum_for_the_column_sum_misses_the_kernel_fixture():
    """The fixture does what it is for: the transposed kernel is outside the bar."""
    g0, g = load_golden("g_opnn.npz"), load_golden("g_opnn_kernel.npz")
    x = torch.tensor(g0["x0"])
    p = R.model({k: v.detach() for k, v in _params(g0).items()}, x, torch.tensor(g["kernel"]).t())
    assert not np.allclose(p.numpy(), g["p0"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("K", [1, 3, 10, 16, 64])
def test_all_ones_kernel_is_k_times_the_square(K):
    """sum_i (s_j * 1) * s_j = K * s_j^2: K equal fp64 terms, so the sum is within K roundings
    (K * 2^-53 relative) of the product."""
    gen = torch.Generator().manual_seed(K)
    V, F, B = 30, 4, 6
    E = torch.randn(V, K, generator=gen, dtype=torch.float64)
    x = torch.randint(0, V, (B, F), generator=gen)
    c = R.cat(E, x, torch.ones(K, K))
    s = R.sum_e(E, x)
    np.testing.assert_array_equal(c[:, :F * K].numpy(), E[x].reshape(B, -1).numpy())
    np.testing.assert_allclose(c[:, F * K:].numpy(), (K * s * s).numpy(), rtol=K * 2.0 ** -52,
                               atol=0)
    # and the scales dominate the values they bound
    ks = torch.full((K,), float(K))
    assert (c.abs() <= R.cat_scale(E, x, ks) * (1 + 1e-12)).all()
    dcat = torch.randn(B, F * K + K, generator=gen, dtype=torch.float64)
    d = R.dslot(E, x, torch.ones(K, K), dcat)
    assert (d.abs() <= R.dslot_scale(E, x, ks, dcat) * (1 + 1e-12)).all()
    want = dcat[:, :F * K].reshape(B, F, K) + (2 * K * s * dcat[:, F * K:]).unsqueeze(1)
    np.testing.assert_allclose(d.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
