"""Plain float64 restatements of the small per-step kernels (the DeepFM out head, the FFM
logit and its row gradients, softmax + the REINFORCE loss gradient), for
tests/test_gpu_small_kernels.py. tests/test_small_kernel_refs.py checks each of them on the
CPU against torch autograd / the oracle, so the GPU tests compare the kernels with
references that something else has checked."""
from __future__ import annotations

import numpy as np
import torch

from oracle import ctr_oracle as O


def f64(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


# --------------------------------------------------------------------- DeepFM head ----
def head_ref(h, w, b, z_fm, y=None, mean_div=None, drop_scale=1.0) -> dict:
    """p_model.py:322 + BCELoss(mean) + the gradient into the last hidden layer, float64.
    h [B, H] is the last Linear's input (after ReLU and Dropout: zero where either cut it),
    w [H], b [1], z_fm [B]. Returns z, p, mag (the L1 norm of z's summands) and, with labels,
    loss (per example), gz = dL/dz = (p - y) / mean_div and dh_pre = dL/d(pre-ReLU
    activation) = gz * w * drop_scale where h > 0, else 0."""
    h, w, b, z_fm = f64(h), f64(w).reshape(-1), f64(b).reshape(-1), f64(z_fm).reshape(-1)
    z = z_fm + (h @ w + b[0])
    p = 1.0 / (1.0 + np.exp(-z))
    out = {"z": z, "p": p, "mag": np.abs(h) @ np.abs(w) + abs(b[0]) + np.abs(z_fm)}
    if y is not None:
        y = f64(y).reshape(-1)
        md = float(h.shape[0] if mean_div is None else mean_div)
        out["loss"] = -(y * np.log(p) + (1.0 - y) * np.log1p(-p))
        out["gz"] = (p - y) / md
        out["dh_pre"] = np.where(h > 0, out["gz"][:, None] * w[None, :] * drop_scale, 0.0)
    return out


# ----------------------------------------------------------------------------- FFM ----
def ffm_ref(x, tables, lin, bias) -> dict:
    """p_model.FFM's logit in float64, pair by pair:
    z = bias + sum_f w[x_f] + sum_{i<j} sum_k E_j[x_i, k] * E_i[x_j, k]; mag is the L1 norm
    of the summands."""
    x = np.asarray(x, dtype=np.int64)
    B, F = x.shape
    T = [f64(t) for t in tables]
    lin, bias = f64(lin).reshape(-1), f64(bias).reshape(-1)
    z = bias[0] + lin[x].sum(1)
    mag = abs(bias[0]) + np.abs(lin[x]).sum(1)
    for i in range(F):
        for j in range(i + 1, F):
            prod = T[j][x[:, i]] * T[i][x[:, j]]
            z = z + prod.sum(1)
            mag = mag + np.abs(prod).sum(1)
    return {"z": z, "mag": mag}


def ffm_keys_ref(x, V: int) -> np.ndarray:
    """keys[(b*F + f)*(F-1) + t'] = t*V + x[b, f], t the t'-th field other than f."""
    x = np.asarray(x, dtype=np.int64)
    B, F = x.shape
    keys = np.empty((B, F, F - 1), dtype=np.int64)
    for f in range(F):
        others = [t for t in range(F) if t != f]
        for tp, t in enumerate(others):
            keys[:, f, tp] = t * V + x[:, f]
    return keys.reshape(-1)


def ffm_vals_ref(x, tables, gz) -> np.ndarray:
    """vals[(b*F + f)*(F-1) + t'] = gz[b] * E_f[x[b, t]] (the gradient of row x[b, f] of
    table t from the pair (f, t)), in the dtype of gz / tables (fp32 in: one fp32 multiply,
    fp64 in: the float64 reference)."""
    x = np.asarray(x, dtype=np.int64)
    B, F = x.shape
    K = tables[0].shape[1]
    gz = np.asarray(gz)
    vals = np.empty((B, F, F - 1, K), dtype=gz.dtype)
    for f in range(F):
        others = [t for t in range(F) if t != f]
        for tp, t in enumerate(others):
            vals[:, f, tp] = gz[:, None] * np.asarray(tables[f], dtype=gz.dtype)[x[:, t]]
    return vals.reshape(-1, K)


# ----------------------------------------------------------------------- REINFORCE ----
def softmax_ref(logits) -> np.ndarray:
    z = f64(logits)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def pg_ref(logits, acts, vt, grad_scale=1.0):
    """(loss, dlogits) of PG_model.loss_func by autograd through oracle.pg_loss in float64,
    from the logits: probs = softmax(logits), loss = sum_b(-log probs[b, a_b - 1]) * mean(vt),
    dlogits = grad_scale * d loss / d logits."""
    lg = torch.tensor(f64(logits), dtype=torch.float64, requires_grad=True)
    loss = O.pg_loss(torch.softmax(lg, dim=1), torch.as_tensor(np.asarray(acts)).reshape(-1),
                     torch.tensor(f64(vt)).reshape(-1))
    loss.backward()
    return float(loss.detach()), lg.grad.numpy() * float(grad_scale)


def pg_closed_form(logits, acts, vt, grad_scale=1.0):
    """The same by hand: dlogits[b, j] = grad_scale * mean(vt) * (p[b, j] - [j == a_b - 1])."""
    p = softmax_ref(logits)
    a = np.asarray(acts, dtype=np.int64).reshape(-1) - 1
    c = f64(vt).mean()
    rows = np.arange(p.shape[0])
    loss = -np.log(p[rows, a]).sum() * c
    onehot = np.zeros_like(p)
    onehot[rows, a] = 1.0
    return float(loss), float(grad_scale) * c * (p - onehot)
