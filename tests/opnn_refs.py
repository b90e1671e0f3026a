"""float64 references of the OuterPNN (OPNN) path, written from the reference's formulas
(src/models/p_model.py:202-254) with the K x K kernel kept as a matrix — nothing here uses the
``ksum * s^2`` reduction the HIP kernels compute, so the two are independent.

  cat(E, x, kernel)            the MLP input [B, F*K + K]: flat(e) ++ sum_i (s*kernel[i])*s
  cat_scale(E, x, ksum)        the L1 scale of every cat element: |e| for the flat part,
                               |ksum_k| * (sum_f |e_fk|)^2 for the cross term
  dslot(E, x, kernel, dcat)    the gradient of every slot's embedding [B, F, K] (autograd)
  dslot_scale(E, x, ksum, dcat)  |d1| + 2 |ksum_k| (sum_f |e_fk|) |d2|
  model(params, x, kernel)     p = sigmoid(MLP(cat)) with the reference's 300/200/1 MLP, no dropout
  grads(params, x, y, kernel)  (loss, p, {name: grad}) of BCELoss(model, y) by autograd
"""
from __future__ import annotations

import torch

KEYS = ("feature_embedding.weight", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias",
        "mlp.6.weight", "mlp.6.bias")


def cat(E: torch.Tensor, x: torch.Tensor, kernel: torch.Tensor) -> torch.Tensor:
    """p_model.py:244-251, operation by operation, in E's dtype."""
    B, F = x.shape
    e = torch.nn.functional.embedding(x, E)                    # [B, F, K]
    s = torch.sum(e, dim=1).unsqueeze(1)                       # [B, 1, K]
    outer = torch.mul(torch.mul(s, kernel.to(E.dtype)), s)     # [B, K, K]
    cross = torch.sum(outer, dim=1)                            # [B, K]
    return torch.cat([e.reshape(B, -1), cross], dim=1)


def cat_scale(E: torch.Tensor, x: torch.Tensor, ksum: torch.Tensor) -> torch.Tensor:
    B, F = x.shape
    ea = torch.nn.functional.embedding(x, E.double().abs())
    sa = ea.sum(1)
    return torch.cat([ea.reshape(B, -1), ksum.double().abs() * sa * sa], dim=1)


def sum_e(E: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.embedding(x, E).sum(1)


def dslot(E: torch.Tensor, x: torch.Tensor, kernel: torch.Tensor, dcat: torch.Tensor):
    """[B, F, K]: autograd of cat with respect to every slot's own embedding copy."""
    B, F = x.shape
    e = torch.nn.functional.embedding(x, E.double()).requires_grad_(True)
    s = torch.sum(e, dim=1).unsqueeze(1)
    cross = torch.sum(torch.mul(torch.mul(s, kernel.double()), s), dim=1)
    out = torch.cat([e.reshape(B, -1), cross], dim=1)
    out.backward(dcat.double()[:, :out.shape[1]])
    return e.grad


def dslot_scale(E, x, ksum, dcat):
    B, F = x.shape
    K = E.shape[1]
    sa = torch.nn.functional.embedding(x, E.double().abs()).sum(1)           # [B, K]
    d = dcat.double().abs()
    d1 = d[:, :F * K].reshape(B, F, K)
    d2 = d[:, F * K:F * K + K]
    return d1 + (2.0 * ksum.double().abs() * sa * d2).unsqueeze(1)


def mlp(params: dict, h: torch.Tensor) -> torch.Tensor:
    h = torch.relu(h @ params["mlp.0.weight"].t() + params["mlp.0.bias"])
    h = torch.relu(h @ params["mlp.3.weight"].t() + params["mlp.3.bias"])
    return h @ params["mlp.6.weight"].t() + params["mlp.6.bias"]


def model(params: dict, x: torch.Tensor, kernel: torch.Tensor) -> torch.Tensor:
    return torch.sigmoid(mlp(params, cat(params["feature_embedding.weight"], x, kernel)))


def grads(params: dict, x: torch.Tensor, y: torch.Tensor, kernel: torch.Tensor):
    """params: {name: leaf tensor requiring grad}. Returns (loss, p, {name: grad})."""
    p = model(params, x, kernel)
    loss = torch.nn.functional.binary_cross_entropy(p, y.to(p.dtype).view(-1, 1))
    gs = torch.autograd.grad(loss, [params[k] for k in KEYS])
    return loss.detach(), p.detach(), dict(zip(KEYS, gs))
