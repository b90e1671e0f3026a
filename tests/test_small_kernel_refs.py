"""CPU checks of tests/small_kernel_refs.py (the float64 references of the small-kernel GPU
tests) against torch autograd and the oracle: a reference that nothing checks is only a
second implementation."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import small_kernel_refs as R
from oracle import ctr_oracle as O


@pytest.mark.parametrize("B,H", [(1, 1), (5, 65), (9, 257)])
@pytest.mark.parametrize("mean_div,drop_scale", [(None, 1.0), (4096.0, 1.25)])
def test_head_ref_vs_autograd(B, H, mean_div, drop_scale):
    """relu -> mask * scale -> dot + b + z_fm -> sigmoid -> BCE / mean_div in float64:
    z, p, the per-example loss, gz = dL/dz and dh_pre = dL/d(pre-ReLU activation)."""
    g = torch.Generator().manual_seed(B * 1000 + H)
    a = torch.randn(B, H, generator=g, dtype=torch.float64).requires_grad_(True)
    mask = (torch.rand(B, H, generator=g) < 0.7).double()
    w = (torch.randn(H, generator=g, dtype=torch.float64) * 0.1).requires_grad_(True)
    b = torch.tensor([0.3], dtype=torch.float64)
    z_fm = torch.randn(B, generator=g, dtype=torch.float64)
    y = (torch.rand(B, generator=g) < 0.4).double()
    h = torch.relu(a) * mask * drop_scale
    z = h @ w + b + z_fm
    z.retain_grad()
    p = torch.sigmoid(z)
    le = torch.nn.functional.binary_cross_entropy(p, y, reduction="none")
    md = float(B if mean_div is None else mean_div)
    (le.sum() / md).backward()
    r = R.head_ref(h.detach(), w.detach(), b, z_fm, y, mean_div, drop_scale)
    np.testing.assert_allclose(r["z"], z.detach().numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(r["p"], p.detach().numpy(), rtol=1e-13)
    np.testing.assert_allclose(r["loss"], le.detach().numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(r["gz"], z.grad.numpy(), rtol=1e-11, atol=1e-18)
    np.testing.assert_allclose(r["dh_pre"], a.grad.numpy(), rtol=1e-11, atol=1e-18)
    assert (r["mag"] >= np.abs(r["z"]) * (1 - 1e-12)).all()
    # inference: the same z and p, nothing else
    ri = R.head_ref(h.detach(), w.detach(), b, z_fm)
    assert set(ri) == {"z", "p", "mag"} and (ri["z"] == r["z"]).all() and (ri["p"] == r["p"]).all()


@pytest.mark.parametrize("V,F,K,B", [(50, 2, 1, 5), (40, 3, 5, 7), (60, 5, 48, 9)])
def test_ffm_ref_vs_oracle(V, F, K, B):
    params = {k: v.detach().double() for k, v in O.init_params("FFM", V, F, K, seed=V + K).items()}
    params["bias"] = params["bias"] + 0.25
    g = torch.Generator().manual_seed(F)
    x = torch.randint(0, V, (B, F), generator=g)
    tabs = [params[f"field_feature_embeddings.{t}.weight"] for t in range(F)]
    r = R.ffm_ref(x.numpy(), tabs, params["linear.weight"], params["bias"])
    np.testing.assert_allclose(r["z"], O.ffm_logit(params, x).reshape(-1).numpy(), rtol=1e-12,
                               atol=1e-12)
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-r["z"])),
                               O.forward("FFM", params, x).reshape(-1).numpy(), rtol=1e-12)
    assert (r["mag"] >= np.abs(r["z"]) * (1 - 1e-12)).all()
    # the (key, row gradient) list summed per key is autograd's table gradient of sum(gz * z)
    gz = torch.randn(B, generator=g, dtype=torch.float64)
    leaf = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    (O.ffm_logit(leaf, x).reshape(-1) * gz).sum().backward()
    keys = R.ffm_keys_ref(x.numpy(), V)
    vals = R.ffm_vals_ref(x.numpy(), [t.numpy() for t in tabs], gz.numpy())
    assert keys.shape == (B * F * (F - 1),) and vals.shape == (keys.size, K)
    dense = np.zeros((F * V, K))
    np.add.at(dense, keys, vals)
    for t in range(F):
        np.testing.assert_allclose(dense[t * V:(t + 1) * V],
                                   leaf[f"field_feature_embeddings.{t}.weight"].grad.numpy(),
                                   rtol=1e-12, atol=1e-14, err_msg=f"table {t}")


@pytest.mark.parametrize("B,A", [(1, 1), (40, 3), (1025, 5)])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_pg_ref_vs_oracle(B, A, grad_scale):
    """pg_ref is autograd through oracle.pg_loss; the closed form is derived by hand."""
    rng = np.random.default_rng(B + A)
    logits = rng.standard_normal((B, A)) * 2
    acts = rng.integers(1, A + 1, size=B)
    vt = rng.random(B) + 0.5
    p = R.softmax_ref(logits)
    np.testing.assert_allclose(p, torch.softmax(torch.tensor(logits), 1).numpy(), rtol=1e-13)
    np.testing.assert_allclose(p.sum(1), 1.0, rtol=1e-14)
    loss, dl = R.pg_ref(logits, acts, vt, grad_scale)
    assert loss == pytest.approx(
        float(O.pg_loss(torch.tensor(p), torch.tensor(acts), torch.tensor(vt))), rel=1e-12)
    loss2, dl2 = R.pg_closed_form(logits, acts, vt, grad_scale)
    assert loss == pytest.approx(loss2, rel=1e-12, abs=1e-300)
    np.testing.assert_allclose(dl, dl2, rtol=1e-10, atol=1e-15)
