"""The float64 AFM references (tests/afm_refs.py) against the reference implementation's own
run (tests/golden/g_afm.npz, make_golden_afm.py). CPU only: no kernel is launched here."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import afm_refs as R
from conftest import assert_grad_close, load_golden


@pytest.fixture(scope="module")
def run0():
    g = load_golden("g_afm.npz")
    params = {k: torch.tensor(g[f"init/{k}"]) for k in R.KEYS}
    loss, p, grads, r = R.model_grads(params, torch.tensor(g["x0"]), torch.tensor(g["y0"]))
    return g, params, loss, p, grads, r


def test_fixture_keys_follow_the_reference_state_dict():
    g = load_golden("g_afm.npz")
    assert [k[5:] for k in g.files if k.startswith("init/")] == list(R.KEYS)
    assert g["init/feature_embedding.weight"].shape == (500, 16) and g["x0"].shape == (64, 8)


def test_the_attention_bites(run0):
    """What the fixture is for: weights from ~1e-6 to ~0.4, not 1/28 everywhere."""
    g, params, *_ = run0
    a = R.forward(params["feature_embedding.weight"], torch.tensor(g["x0"]),
                  params["attention_net.weight"], params["attention_net.bias"],
                  params["attention_softmax.weight"], params["attention_softmax.bias"])["a"]
    assert float(a.max()) > 0.3 and float(a.min()) < 1e-3
    np.testing.assert_allclose(a.sum(1).numpy(), 1.0, rtol=1e-12)


def test_refs_match_the_reference_run(run0):
    """p0 within rtol 1e-5 / atol 1e-7, loss0 within 1e-5, every grad0/* within
    assert_grad_close's bar; attention_softmax.bias (zero in exact arithmetic: the softmax is
    shift-invariant; the recorded value is fp32 rounding noise) with cond = sum |ds|."""
    g, params, loss, p, grads, r = run0
    np.testing.assert_allclose(p.numpy(), g["p0"], rtol=1e-5, atol=1e-7)
    assert float(loss) == pytest.approx(float(g["loss0"]), rel=1e-5)
    for k in R.KEYS:
        cond = None
        if k == "attention_softmax.bias":
            cond = np.array([float(r["ds"].abs().sum())])
            assert abs(float(grads[k])) <= 1e-12 * cond[0]
        assert_grad_close(g[f"grad0/{k}"], grads[k].numpy(), cond=cond, err_msg=k)


def test_a_broken_attention_misses_the_fixture(run0):
    """Uniform attention (the path skipped) is far outside the bar on this fixture."""
    g, params, *_ = run0
    flat = dict(params)
    flat["attention_softmax.weight"] = torch.zeros_like(params["attention_softmax.weight"])
    _, p, _, _ = R.model_grads(flat, torch.tensor(g["x0"]), torch.tensor(g["y0"]))
    assert not np.allclose(p.numpy(), g["p0"], rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("shape", [(3, 2, 1, 1), (4, 5, 7, 3), (2, 9, 16, 16)])
def test_backward_formulas_match_autograd(shape):
    """The hand-written backward against torch.autograd in float64, with dropout masks."""
    B, F, K, A = shape
    c = R.case(B, F, K, A)
    m1, m2 = R.masks(B, F, K, 0.2, 11)
    leaves = [t.double().requires_grad_(True) for t in (c.E, c.W1, c.b1, c.w2, c.b2)]
    E, W1, b1, w2, b2 = leaves
    row, col = R.pairs(F)
    e = E[c.x]
    q = e[:, row] * e[:, col]
    s = torch.relu(q @ W1.t() + b1) @ w2 + b2
    pooled = ((torch.softmax(s, 1) * m1).unsqueeze(-1) * q).sum(1) * m2
    gE, gW1, gb1, gw2, gb2 = torch.autograd.grad(pooled, leaves, c.dpooled.double())
    f = R.forward(c.E, c.x, c.W1, c.b1, c.w2, c.b2, m1, m2)
    np.testing.assert_allclose(f["pooled"].numpy(), pooled.detach().numpy(), rtol=1e-12, atol=1e-14)
    r = R.backward(f, c.W1, c.b1, c.w2, c.dpooled)
    dense = torch.zeros_like(E).index_add_(0, c.x.reshape(-1), r["dslot"].reshape(B * F, K))
    for name, ours, ref in (("E", dense, gE), ("dW1", r["dW1"], gW1), ("db1", r["db1"], gb1),
                            ("dw2", r["dw2"], gw2)):
        np.testing.assert_allclose(ours.numpy(), ref.numpy(), rtol=1e-10,
                                   atol=1e-12 * max(float(ref.abs().max()), 1e-30), err_msg=name)
    assert abs(float(r["db2"]) - float(gb2)) <= 1e-12 * float(r["db2_scale"])
    for name in ("dslot", "dW1", "db1", "dw2", "db2"):  # the scales dominate what they bound
        assert bool((r[name].abs() <= r[name + "_scale"] * (1 + 1e-12) + 1e-300).all()), name
    assert bool((f["pooled"].abs() <= f["pooled_scale"] * (1 + 1e-12)).all())


def test_masks_follow_the_gemm_convention():
    import gemm_refs as G
    B, F, K = 5, 4, 3
    P = 6
    m1, m2 = R.masks(B, F, K, 0.2, 99)
    keep = G.dropout_keep(B, P + K, 0.2, 99, 0)
    scale = float(G.drop_scale(0.2))
    np.testing.assert_array_equal(m1.numpy(), keep[:, :P] * scale)
    np.testing.assert_array_equal(m2.numpy(), keep[:, P:] * scale)
    o1, o2 = R.masks(B, F, K, 0.0, 99)
    assert bool((o1 == 1).all()) and bool((o2 == 1).all())
