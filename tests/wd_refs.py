"""float64 numpy references of the WideAndDeep (W&D) path, written from the reference's formulas
(src/models/p_model.py:103-144); the backward is derived by hand (no autograd), so nothing here
shares code with the HIP kernels or with torch's own backward.

  flat(E, x)                    the MLP input [B, F*K]: E[x] flattened
  z_lin(lin, bias, x)           bias + sum_f lin[x_f], [B]
  z_lin_scale(lin, bias, x)     |bias| + sum_f |lin[x_f]|, the L1 scale of that sum
  row_sums(x, V, gz, dx)        (g_emb [V, K], g_lin [V], cond_emb [V, K], cond_lin [V]): every
                                row's gradient sums over the slots that hold it, dx [B, F*K], and
                                the sums of the contributions' magnitudes (their L1 condition)
  model(params, x)              p = sigmoid(z_lin + MLP(flat)) [B, 1], 300/200/1 MLP, no dropout
  grads(params, x, y)           (loss, p, {name: grad}, {name: L1 condition of the table grads})
                                of BCELoss(model, y), mean over the batch
"""
from __future__ import annotations

import numpy as np

KEYS = ("bias", "linear.weight", "embedding.weight", "mlp.0.weight", "mlp.0.bias",
        "mlp.3.weight", "mlp.3.bias", "mlp.6.weight", "mlp.6.bias")


def _f64(a) -> np.ndarray:
    return np.asarray(a, dtype=np.float64)


def flat(E, x) -> np.ndarray:
    x = np.asarray(x)
    E = np.asarray(E)
    return E[x].reshape(x.shape[0], -1)


def z_lin(lin, bias, x) -> np.ndarray:
    w = _f64(lin).reshape(-1)
    return _f64(bias).reshape(-1)[0] + w[np.asarray(x)].sum(1)


def z_lin_scale(lin, bias, x) -> np.ndarray:
    w = np.abs(_f64(lin).reshape(-1))
    return abs(_f64(bias).reshape(-1)[0]) + w[np.asarray(x)].sum(1)


def row_sums(x, V: int, gz, dx):
    x = np.asarray(x)
    B, F = x.shape
    gz = _f64(gz).reshape(B)
    d = _f64(dx).reshape(B * F, -1)
    K = d.shape[1]
    rows = x.reshape(-1)
    g_emb, c_emb = np.zeros((V, K)), np.zeros((V, K))
    g_lin, c_lin = np.zeros(V), np.zeros(V)
    np.add.at(g_emb, rows, d)
    np.add.at(c_emb, rows, np.abs(d))
    gl = np.repeat(gz, F)
    np.add.at(g_lin, rows, gl)
    np.add.at(c_lin, rows, np.abs(gl))
    return g_emb, g_lin, c_emb, c_lin


def _mlp(params, h):
    a1 = np.maximum(h @ _f64(params["mlp.0.weight"]).T + _f64(params["mlp.0.bias"]), 0.0)
    a2 = np.maximum(a1 @ _f64(params["mlp.3.weight"]).T + _f64(params["mlp.3.bias"]), 0.0)
    out = a2 @ _f64(params["mlp.6.weight"]).T + _f64(params["mlp.6.bias"])
    return a1, a2, out


def model(params, x) -> np.ndarray:
    h = flat(_f64(params["embedding.weight"]), x)
    z = z_lin(params["linear.weight"], params["bias"], x)[:, None] + _mlp(params, h)[2]
    return 1.0 / (1.0 + np.exp(-z))


def grads(params, x, y):
    x = np.asarray(x)
    B = x.shape[0]
    E = _f64(params["embedding.weight"])
    V = E.shape[0]
    y = _f64(y).reshape(B, 1)
    h = flat(E, x)
    a1, a2, out = _mlp(params, h)
    z = z_lin(params["linear.weight"], params["bias"], x)[:, None] + out
    p = 1.0 / (1.0 + np.exp(-z))
    loss = float(np.mean(-(y * np.log(p) + (1.0 - y) * np.log1p(-p))))
    gz = (p - y) / B                                     # dL/dz of the mean BCE after sigmoid
    g = {"bias": gz.sum(0), "mlp.6.weight": gz.T @ a2, "mlp.6.bias": gz.sum(0)}
    d2 = (gz @ _f64(params["mlp.6.weight"])) * (a2 > 0)
    g["mlp.3.weight"], g["mlp.3.bias"] = d2.T @ a1, d2.sum(0)
    d1 = (d2 @ _f64(params["mlp.3.weight"])) * (a1 > 0)
    g["mlp.0.weight"], g["mlp.0.bias"] = d1.T @ h, d1.sum(0)
    dx = d1 @ _f64(params["mlp.0.weight"])
    g_emb, g_lin, c_emb, c_lin = row_sums(x, V, gz, dx)
    g["embedding.weight"], g["linear.weight"] = g_emb, g_lin.reshape(V, 1)
    cond = {"embedding.weight": c_emb, "linear.weight": c_lin.reshape(V, 1)}
    return loss, p, g, cond
