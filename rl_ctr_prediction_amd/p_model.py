"""LR, FM, FFM, WideAndDeep, DeepFM, InnerPNN, OuterPNN, FNN, DCN and AFM with the reference's construction API, on the
HIP kernels.

Drop-in for ``src/models/p_model.py`` (LR 9-26, FM 28-57, FFM 59-100, WideAndDeep 103-144, InnerPNN 146-200, OuterPNN 202-254, DeepFM 256-324,
FNN 326-373, DCN 376-435, AFM 438-486): identical constructor
signatures, submodules created in the same order (so ``torch.manual_seed(s)`` gives the
same initial weights as the reference) and identical state_dict keys, so the RL drivers'
``torch.load('...FMbest.pth')`` / ``load_state_dict`` and ``Feature_Embedding.load_embedding``
work unchanged. ``forward(LongTensor[B,F]) -> FloatTensor[B,1]`` pCTR.

Two execution paths, both entirely on libctr_hip.so kernels for the model math:
  * autograd (drop-in): ``loss.backward()`` produces the reference's DENSE [V,K] embedding
    gradient, so a stock ``torch.optim.Adam`` keeps working;
  * fused training (the hot path): :class:`rl_ctr_prediction_amd.trainer.FusedCTRTrainer`
    runs forward, BCE, backward, the scatter-add and dense Adam without materialising the
    dense gradient.
"""
from __future__ import annotations

import itertools

import numpy as np
import torch
import torch.nn as nn

from . import hip_ops

_seed_counter = itertools.count()


def _dropout_seed() -> int:
    # deterministic under torch.manual_seed, distinct per call site
    return (torch.initial_seed() * 1000003 + next(_seed_counter) * 7919) & (2**63 - 1)


def _rng_dropout_seed() -> int:
    # drawn from torch's generator, like the reference's dropout masks: two forwards after
    # the same torch.manual_seed drop the same elements (FNN, DCN)
    return int(torch.randint(0, 2**62, (1,)).item())


class _FMPart(torch.autograd.Function):
    """(z_fm [B,1], flat embeddings [B,F*K]) = FM part of p_model.py:296-313 (+ the
    gather at 320). Backward = FM gradient + MLP-input gradient, summed per row in slot
    order (deterministic), returned as dense grads like embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, emb, lin, bias, want_emb):
        B, F = x.shape
        r = hip_ops.fm_forward(x, emb, lin, bias, want_sum=True, want_emb=want_emb, want_p=False)
        ctx.save_for_backward(x, emb, r.sum_e)
        ctx.want_emb = want_emb
        flat = r.emb_out if want_emb else emb.new_empty(0)
        return r.z.view(B, 1), flat

    @staticmethod
    def backward(ctx, gz, gflat):
        x, emb, sum_e = ctx.saved_tensors
        B, F = x.shape
        V, K = emb.shape
        if gz is None:
            gz = torch.zeros(B, dtype=torch.float32, device=emb.device)
        gz = gz.reshape(-1).contiguous()
        dx = gflat.contiguous() if (ctx.want_emb and gflat is not None) else None
        plan = hip_ops.SparsePlanBuffers(B * F, emb.device).build(x, V)
        grad_rows, grad_lin = hip_ops.fm_embedding_grad(plan, F, emb, gz, sum_e, dx)
        g_emb, g_lin = hip_ops.rows_to_dense(plan, V, grad_rows, grad_lin)
        g_bias = hip_ops.tensor_sum(gz) if ctx.needs_input_grad[3] else None
        return (None, g_emb if ctx.needs_input_grad[1] else None,
                g_lin if ctx.needs_input_grad[2] else None, g_bias, None)


class _WDPart(torch.autograd.Function):
    """(z_lin [B,1], flat embeddings [B,F*K]) = the wide logit and the MLP input of
    p_model.py:140-142 in one launch (ctr_wd_forward). Backward: a slot's embedding gradient
    is its slice of the MLP-input gradient, its linear gradient its example's gz
    (ctr_wd_embedding_grad), summed per row in slot order (deterministic), returned as dense
    grads like embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, emb, lin, bias):
        B, F = x.shape
        z_lin, flat = hip_ops.wd_forward(x, emb, lin, bias)
        ctx.save_for_backward(x)
        ctx.VK = tuple(emb.shape)
        return z_lin.view(B, 1), flat

    @staticmethod
    def backward(ctx, gz, gflat):
        (x,) = ctx.saved_tensors
        B, F = x.shape
        V, K = ctx.VK
        dev = x.device
        gz = (torch.zeros(B, dtype=torch.float32, device=dev) if gz is None
              else gz.reshape(-1).contiguous())
        dx = (torch.zeros(B, F * K, dtype=torch.float32, device=dev) if gflat is None
              else gflat.contiguous())
        plan = hip_ops.SparsePlanBuffers(B * F, dev).build(x, V)
        grad_rows, grad_lin = hip_ops.wd_embedding_grad(plan, F, K, gz, dx)
        g_emb, g_lin = hip_ops.rows_to_dense(plan, V, grad_rows, grad_lin)
        g_bias = hip_ops.tensor_sum(gz).view(1) if ctx.needs_input_grad[3] else None
        return (None, g_emb if ctx.needs_input_grad[1] else None,
                g_lin if ctx.needs_input_grad[2] else None, g_bias)


class _LRPart(torch.autograd.Function):
    """z [B,1] = bias + sum_f lin[x_f] (p_model.py:23) on ctr_lr_forward. Backward: every
    slot's gradient is gz[b]; summed per row in slot order through the sparse plan
    (deterministic, as _FMPart), returned dense [V,1] like embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, lin, bias):
        ctx.save_for_backward(x)
        ctx.V = lin.shape[0]
        return hip_ops.lr_forward(x, lin, bias, want_p=False)["z"].view(-1, 1)

    @staticmethod
    def backward(ctx, gz):
        (x,) = ctx.saved_tensors
        B, F = x.shape
        gz = gz.reshape(-1).contiguous()
        g_lin = None
        if ctx.needs_input_grad[1]:
            plan = hip_ops.SparsePlanBuffers(B * F, gz.device).build(x, ctx.V)
            slot_g = gz.view(B, 1).expand(B, F).reshape(-1, 1).contiguous()  # dL/dw[x_bf] = gz[b]
            rows, _ = hip_ops.segment_sum_rows(plan, slot_g)
            g_lin, _ = hip_ops.rows_to_dense(plan, ctx.V, rows)
        g_bias = hip_ops.tensor_sum(gz).view(1) if ctx.needs_input_grad[2] else None
        return None, g_lin, g_bias


class _LinearAct(torch.autograd.Function):
    """nn.Linear (+ ReLU + Dropout) on the fp32 MFMA GEMM with fused epilogues."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, drop_p, seed):
        y = hip_ops.linear(x.contiguous(), weight, bias, relu=relu, drop_p=drop_p, seed=seed)
        ctx.save_for_backward(x, weight, y)
        ctx.relu = relu
        ctx.scale = 1.0 / (1.0 - drop_p)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        gy = gy.contiguous()
        if ctx.relu:  # Dropout then ReLU backward: grad where the saved output is > 0
            g = torch.where(y > 0, gy * ctx.scale, torch.zeros_like(gy))
        else:
            g = gy
        dx = hip_ops.gemm(g, weight) if ctx.needs_input_grad[0] else None
        dw = hip_ops.gemm(g, x.contiguous(), trans_a=True) if ctx.needs_input_grad[1] else None
        db = hip_ops.colsum(g) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None, None


class _IPNNPart(torch.autograd.Function):
    """cat = flat(E[x]) ++ pairwise inner products (p_model.py:187-195). Backward: the
    per-slot gradients (ctr_ipnn_backward), summed per row in slot order (deterministic),
    returned dense like embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, emb):
        ctx.save_for_backward(x, emb)
        return hip_ops.ipnn_forward(x, emb)

    @staticmethod
    def backward(ctx, gcat):
        x, emb = ctx.saved_tensors
        B, F = x.shape
        V, K = emb.shape
        dslot = hip_ops.ipnn_backward(x, emb, gcat.contiguous())
        plan = hip_ops.SparsePlanBuffers(B * F, emb.device).build(x, V)
        grad_rows, _ = hip_ops.segment_sum_rows(plan, dslot)
        g_emb, _ = hip_ops.rows_to_dense(plan, V, grad_rows)
        return None, g_emb


class _OPNNPart(torch.autograd.Function):
    """cat = flat(E[x]) ++ ksum * (sum_f e_f)^2 (p_model.py:244-251). Backward: the per-slot
    gradients (ctr_opnn_backward, from the saved field sums: no second gather), summed per row
    in slot order (deterministic), returned dense like embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, emb, ksum):
        B, F = x.shape
        sum_e = torch.empty(B, emb.shape[1], dtype=torch.float32, device=emb.device)
        cat = hip_ops.opnn_forward(x, emb, ksum, sum_e=sum_e)
        # ksum is the model's cache, refreshed in place: the backward needs this call's values
        ctx.save_for_backward(x, sum_e, ksum.clone())
        ctx.V = emb.shape[0]
        return cat

    @staticmethod
    def backward(ctx, gcat):
        x, sum_e, ksum = ctx.saved_tensors
        B, F = x.shape
        dslot = hip_ops.opnn_backward(sum_e, ksum, gcat.contiguous(), F)
        plan = hip_ops.SparsePlanBuffers(B * F, gcat.device).build(x, ctx.V)
        grad_rows, _ = hip_ops.segment_sum_rows(plan, dslot)
        g_emb, _ = hip_ops.rows_to_dense(plan, ctx.V, grad_rows)
        return None, g_emb, None


class _FFMPart(torch.autograd.Function):
    """FFM logit (p_model.py:82-97) on ctr_ffm_forward; backward: every example's table-row
    gradients (ctr_ffm_backward), summed per (table, row) in slot order through a sparse plan
    over the F*V key space, returned dense per table like embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, lin, bias, ptrs, *tables):
        ctx.save_for_backward(x, ptrs, *tables)
        return hip_ops.ffm_forward(x, tables, ptrs, lin, bias)["z"].view(-1, 1)

    @staticmethod
    def backward(ctx, gz):
        x, ptrs, *tables = ctx.saved_tensors
        B, F = x.shape
        V, K = tables[0].shape
        dev = gz.device
        gz = gz.reshape(-1).contiguous()
        keys, vals = hip_ops.ffm_backward(x, tables, ptrs, gz)
        plan = hip_ops.SparsePlanBuffers(keys.numel(), dev).build(keys, F * V)
        rows, _ = hip_ops.segment_sum_rows(plan, vals)
        dense, _ = hip_ops.rows_to_dense(plan, F * V, rows)
        g_tables = [dense[t * V:(t + 1) * V] for t in range(F)]
        plan_x = hip_ops.SparsePlanBuffers(B * F, dev).build(x, V)
        slot_g = gz.view(B, 1).expand(B, F).reshape(-1, 1).contiguous()  # dL/dw[x_bf] = gz[b]
        rows_w, _ = hip_ops.segment_sum_rows(plan_x, slot_g)
        g_lin, _ = hip_ops.rows_to_dense(plan_x, V, rows_w)
        return (None, g_lin, hip_ops.tensor_sum(gz).view(1), None, *g_tables)


class _GatherFlat(torch.autograd.Function):
    """flat(E[x]) [B, F*K] (p_model.py:370, 424: the gather + view of FNN and DCN). Backward:
    the slot gradients summed per row in slot order (deterministic), returned dense like
    embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, emb):
        ctx.save_for_backward(x, emb)
        B, F = x.shape
        return hip_ops.embedding_gather(emb, x).view(B, F * emb.shape[1])

    @staticmethod
    def backward(ctx, gflat):
        x, emb = ctx.saved_tensors
        B, F = x.shape
        V, K = emb.shape
        plan = hip_ops.SparsePlanBuffers(B * F, emb.device).build(x, V)
        grad_rows, _ = hip_ops.segment_sum_rows(plan, gflat.contiguous().view(B * F, K))
        g_emb, _ = hip_ops.rows_to_dense(plan, V, grad_rows)
        return None, g_emb


class _CrossPart(torch.autograd.Function):
    """z_cross [B,1] = <x_L, w_tail> of DCN's cross network (p_model.py:426-429 and the cross
    columns of the final Linear, 431-433) on ctr_dcn_cross_forward; x_L is never written.
    Saves x0 and the per-layer dots s; backward = one ctr_dcn_cross_backward in the rank-1
    form (dL/dx_L = gz * w_tail)."""

    @staticmethod
    def forward(ctx, x0, W, b, w_tail):
        x0 = x0.contiguous()
        r = hip_ops.dcn_cross_forward(x0, W, b, w_tail, want_xl=False)
        ctx.save_for_backward(x0, W, b, w_tail, r["s"])
        return r["z"].view(-1, 1)

    @staticmethod
    def backward(ctx, gz):
        x0, W, b, w_tail, s = ctx.saved_tensors
        r = hip_ops.dcn_cross_backward(x0, W, b, s, gz=gz.reshape(-1).contiguous(), w_tail=w_tail)
        return r["dx0"], r["dW"], r["dbias"], r["dw_tail"]


class _AFMPart(torch.autograd.Function):
    """pooled [B, K] = AFM's attention pooling of the pair products (p_model.py:473-482) on
    ctr_afm_forward; keeps the softmax [B, P] alone. Backward = one ctr_afm_backward (the
    attention parameters' gradients and the per-slot embedding gradients), the slots summed
    per row in slot order (deterministic), returned dense like embedding_dense_backward."""

    @staticmethod
    def forward(ctx, x, emb, W1, b1, w2, b2, drop_p, seed):
        pooled, attn = hip_ops.afm_forward(x, emb, W1, b1, w2.reshape(-1), b2, drop_p, seed)
        ctx.save_for_backward(x, emb, W1, b1, w2, b2, attn)
        ctx.drop = (drop_p, seed)
        return pooled

    @staticmethod
    def backward(ctx, gpooled):
        x, emb, W1, b1, w2, b2, attn = ctx.saved_tensors
        B, F = x.shape
        V, K = emb.shape
        r = hip_ops.afm_backward(x, emb, W1, b1, w2.reshape(-1), b2, attn, gpooled.contiguous(),
                                 *ctx.drop)
        plan = hip_ops.SparsePlanBuffers(B * F, emb.device).build(x, V)
        grad_rows, _ = hip_ops.segment_sum_rows(plan, r["dslot"])
        g_emb, _ = hip_ops.rows_to_dense(plan, V, grad_rows)
        return None, g_emb, r["dW1"], r["db1"], r["dw2"].view_as(w2), r["db2"], None, None


def _fm_part(x, emb, lin, bias, want_emb):
    return _FMPart.apply(x, emb, lin, bias, want_emb)


def mlp_forward(mlp: nn.Sequential, h: torch.Tensor, training: bool,
                seed_fn=_dropout_seed) -> torch.Tensor:
    """Run an nn.Sequential of [Linear, ReLU, Dropout]* + Linear on fused HIP GEMMs; seed_fn
    gives each dropout layer's seed."""
    mods = list(mlp)
    i = 0
    while i < len(mods):
        lin = mods[i]
        if not isinstance(lin, nn.Linear):
            raise TypeError(f"unsupported MLP layer {type(lin).__name__}")
        j = i + 1
        relu = j < len(mods) and isinstance(mods[j], nn.ReLU)
        j += int(relu)
        drop = 0.0
        if relu and j < len(mods) and isinstance(mods[j], nn.Dropout):
            drop = float(mods[j].p) if training else 0.0
            j += 1
        h = _LinearAct.apply(h, lin.weight, lin.bias, relu, drop, seed_fn())
        i = j
    return h


class LR(nn.Module):
    """p_model.py:9-26. z = bias + sum_f w[x_f]; p = sigmoid(z)."""

    def __init__(self, feature_nums, output_dim=1):
        super().__init__()
        if output_dim != 1:
            raise NotImplementedError("LR: output_dim must be 1 (the reference's only use)")
        self.linear = nn.Embedding(feature_nums, output_dim)
        self.bias = nn.Parameter(torch.zeros((output_dim,)))

    def forward(self, x):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return torch.sigmoid(_LRPart.apply(x, self.linear.weight, self.bias))
        r = hip_ops.lr_forward(x, self.linear.weight.detach(), self.bias.detach())
        return r["p"].view(-1, 1)


class FM(nn.Module):
    """p_model.py:28-57. z = bias + sum_f w[x_f] + 0.5 * sum_k((sum_f e)^2 - sum_f e^2)."""

    def __init__(self, feature_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)  # the driver's --latent_dims arrives as str
        if output_dim != 1:
            raise NotImplementedError("FM: output_dim must be 1 (the reference's only use)")
        self.linear = nn.Embedding(feature_nums, output_dim)
        self.bias = nn.Parameter(torch.zeros((output_dim,)))
        self.feature_embedding = nn.Embedding(feature_nums, latent_dims)

    def forward(self, x):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            z, _ = _fm_part(x, self.feature_embedding.weight, self.linear.weight, self.bias, False)
            return torch.sigmoid(z)
        r = hip_ops.fm_forward(x, self.feature_embedding.weight.detach(),
                               self.linear.weight.detach(), self.bias.detach(), want_sum=False)
        return r.p.view(-1, 1)


class WideAndDeep(nn.Module):
    """p_model.py:103-144: z = (bias + sum_f w[x_f]) + MLP [F*K -> 300 -> 200 -> 1] (ReLU,
    Dropout 0.2) over the flat embeddings — DeepFM without the second-order term. The table
    is ``embedding`` (not ``feature_embedding``), as in the reference."""

    def __init__(self, feature_nums, field_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)
        if output_dim != 1:
            raise NotImplementedError("WideAndDeep: output_dim must be 1 (the reference's only "
                                      "use)")
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.latent_dims = latent_dims
        self.linear = nn.Embedding(self.feature_nums, output_dim)
        self.bias = nn.Parameter(torch.zeros((output_dim,)))
        self.embedding = nn.Embedding(self.feature_nums, self.latent_dims)
        deep_input_dims = self.field_nums * self.latent_dims
        layers = []
        for neuron_num in (300, 200):
            layers.append(nn.Linear(deep_input_dims, neuron_num))
            layers.append(nn.ReLU())
            layers.append(nn.Dropout(p=0.2))
            deep_input_dims = neuron_num
        layers.append(nn.Linear(deep_input_dims, 1))
        self.mlp = nn.Sequential(*layers)

    def forward(self, x):
        E, w, b = self.embedding.weight, self.linear.weight, self.bias
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            z_lin, flat = _WDPart.apply(x, E, w, b)
            out = mlp_forward(self.mlp, flat, self.training)
            return torch.sigmoid(z_lin + out)
        with torch.no_grad():
            z_lin, h = hip_ops.wd_forward(x, E.detach(), w.detach(), b.detach())
            m = self.mlp
            p0 = m[2].p if self.training else 0.0
            p1 = m[5].p if self.training else 0.0
            h = hip_ops.linear(h, m[0].weight, m[0].bias, relu=True, drop_p=p0,
                               seed=_dropout_seed())
            h = hip_ops.linear(h, m[3].weight, m[3].bias, relu=True, drop_p=p1,
                               seed=_dropout_seed())
            head = hip_ops.deepfm_head(h, m[6].weight, m[6].bias, z_lin)
            return head["p"].view(-1, 1)


class DeepFM(nn.Module):
    """p_model.py:256-324: FM part + MLP [F*K -> 300 -> 200 -> 1] (ReLU, Dropout 0.2)."""

    def __init__(self, feature_nums, field_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.latent_dims = latent_dims
        self.linear = nn.Embedding(self.feature_nums, output_dim)
        self.bias = nn.Parameter(torch.zeros((output_dim,)))
        self.feature_embedding = nn.Embedding(self.feature_nums, self.latent_dims)
        deep_input_dims = self.field_nums * self.latent_dims
        layers = []
        for neuron_num in (300, 200):
            layers.append(nn.Linear(deep_input_dims, neuron_num))
            layers.append(nn.ReLU())
            layers.append(nn.Dropout(p=0.2))
            deep_input_dims = neuron_num
        layers.append(nn.Linear(deep_input_dims, 1))
        self.mlp = nn.Sequential(*layers)

    def forward(self, x):
        E, w, b = self.feature_embedding.weight, self.linear.weight, self.bias
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            z_fm, flat = _fm_part(x, E, w, b, True)
            out = mlp_forward(self.mlp, flat, self.training)
            return torch.sigmoid(z_fm + out)
        with torch.no_grad():
            r = hip_ops.fm_forward(x, E.detach(), w.detach(), b.detach(), want_sum=False,
                                   want_emb=True, want_p=False)
            h = r.emb_out
            m = self.mlp
            p0 = m[2].p if self.training else 0.0
            p1 = m[5].p if self.training else 0.0
            h = hip_ops.linear(h, m[0].weight, m[0].bias, relu=True, drop_p=p0,
                               seed=_dropout_seed())
            h = hip_ops.linear(h, m[3].weight, m[3].bias, relu=True, drop_p=p1,
                               seed=_dropout_seed())
            head = hip_ops.deepfm_head(h, m[6].weight, m[6].bias, r.z)
            return head["p"].view(-1, 1)


class InnerPNN(nn.Module):
    """p_model.py:146-200: MLP [F*K + F(F-1)/2 -> 300 -> 200 -> 1] (ReLU, Dropout 0.2) over
    the flat embeddings and their pairwise inner products; no linear term, no bias."""

    def __init__(self, feature_nums, field_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.latent_dims = latent_dims
        self.feature_embedding = nn.Embedding(self.feature_nums, self.latent_dims)
        deep_input_dims = self.field_nums * self.latent_dims + self.field_nums * (self.field_nums - 1) // 2
        layers = []
        for neuron_num in (300, 200):
            layers.append(nn.Linear(deep_input_dims, neuron_num))
            layers.append(nn.ReLU())
            layers.append(nn.Dropout(p=0.2))
            deep_input_dims = neuron_num
        layers.append(nn.Linear(deep_input_dims, 1))
        self.mlp = nn.Sequential(*layers)
        # the reference's pair lists (p_model.py:179-182), kept for API parity
        self.row, self.col = [], []
        for i in range(self.field_nums - 1):
            for j in range(i + 1, self.field_nums):
                self.row.append(i), self.col.append(j)

    def forward(self, x):
        E = self.feature_embedding.weight
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            cat = _IPNNPart.apply(x, E)
            return torch.sigmoid(mlp_forward(self.mlp, cat, self.training))
        with torch.no_grad():
            h = hip_ops.ipnn_forward(x, E.detach())
            m = self.mlp
            p0 = m[2].p if self.training else 0.0
            p1 = m[5].p if self.training else 0.0
            h = hip_ops.linear(h, m[0].weight, m[0].bias, relu=True, drop_p=p0,
                               seed=_dropout_seed())
            h = hip_ops.linear(h, m[3].weight, m[3].bias, relu=True, drop_p=p1,
                               seed=_dropout_seed())
            zero = torch.zeros(h.shape[0], dtype=torch.float32, device=h.device)
            head = hip_ops.deepfm_head(h, m[6].weight, m[6].bias, zero)
            return head["p"].view(-1, 1)


class OuterPNN(nn.Module):
    """p_model.py:202-254: MLP [F*K + K -> 300 -> 200 -> 1] (ReLU, Dropout 0.2) over the flat
    embeddings and the kernel-weighted outer-product term of their field sum s,
    sum_i (s_j * kernel[i,j]) * s_j = kernel.sum(0)[j] * s_j^2; no linear term, no bias.
    ``kernel`` (ones, as in the reference, where it is a plain attribute) is a non-persistent
    buffer: absent from state_dict, it follows ``.to()``; it is not trained."""

    def __init__(self, feature_nums, field_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)
        if output_dim != 1:
            raise NotImplementedError("OuterPNN: output_dim must be 1 (the reference's only use)")
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.latent_dims = latent_dims
        self.feature_embedding = nn.Embedding(self.feature_nums, self.latent_dims)
        deep_input_dims = self.latent_dims + self.field_nums * self.latent_dims
        layers = []
        for neuron_num in (300, 200):
            layers.append(nn.Linear(deep_input_dims, neuron_num))
            layers.append(nn.ReLU())
            layers.append(nn.Dropout(p=0.2))
            deep_input_dims = neuron_num
        layers.append(nn.Linear(deep_input_dims, 1))
        self.mlp = nn.Sequential(*layers)
        self.register_buffer("kernel", torch.ones((self.latent_dims, self.latent_dims)),
                             persistent=False)
        # kernel.sum(0), what the kernels read: one buffer, refreshed in place (ksum())
        self.register_buffer("_ksum", torch.zeros(self.latent_dims), persistent=False)
        self._ksum_key = None

    def ksum(self) -> torch.Tensor:
        """The cached column sums of ``kernel``, refreshed in place when the kernel was
        replaced or written (its data pointer or version counter moved). Nothing is read
        back to the host. Writes through ``kernel.data`` bypass the counter: assign or
        ``copy_`` instead."""
        kern = self.kernel
        if kern.requires_grad:
            raise NotImplementedError("OuterPNN: the kernel is a constant (as in the reference); "
                                      "a kernel that requires grad is not supported")
        K = self.latent_dims
        if tuple(kern.shape) != (K, K):
            raise ValueError(f"OuterPNN: kernel must be [{K}, {K}], got {tuple(kern.shape)}")
        # the tensor itself is held too: a freed kernel's address can be handed out again
        key = (kern.data_ptr(), kern._version, self._ksum.data_ptr())
        src = self._ksum_key
        if src is None or src[0] is not kern or src[1] != key:
            self._ksum.copy_(kern.detach().sum(0), non_blocking=True)
            self._ksum_key = (kern, key)
        return self._ksum

    def forward(self, x):
        E = self.feature_embedding.weight
        ksum = self.ksum()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            cat = _OPNNPart.apply(x, E, ksum)
            return torch.sigmoid(mlp_forward(self.mlp, cat, self.training))
        with torch.no_grad():
            h = hip_ops.opnn_forward(x, E.detach(), ksum)
            m = self.mlp
            p0 = m[2].p if self.training else 0.0
            p1 = m[5].p if self.training else 0.0
            h = hip_ops.linear(h, m[0].weight, m[0].bias, relu=True, drop_p=p0,
                               seed=_dropout_seed())
            h = hip_ops.linear(h, m[3].weight, m[3].bias, relu=True, drop_p=p1,
                               seed=_dropout_seed())
            zero = torch.zeros(h.shape[0], dtype=torch.float32, device=h.device)
            head = hip_ops.deepfm_head(h, m[6].weight, m[6].bias, zero)
            return head["p"].view(-1, 1)


class AFM(nn.Module):
    """p_model.py:438-486, the attentional factorisation machine: the pair products
    e_i * e_j (i < j) go through attention_net (K -> K, ReLU) and attention_softmax (K -> 1), a
    softmax over the pairs weighs them, and z = bias + sum_f w[x_f] + fc(pooled). Submodules
    are created in the reference's order, so a seed gives its initial weights and its
    state_dict keys. The pooling and its backward are one HIP kernel each (ctr_afm_*): no
    [B, P, K] tensor is formed.

    ``drop_p`` (0.2, the reference's constant) drives both dropouts: on the attention weights
    and on the pooled vector, with one seed per forward drawn from torch's generator.
    Deliberate difference: the reference calls ``F.dropout(x, p=0.2)``, whose ``training``
    flag defaults to True, so it keeps dropping in ``eval()`` and its test predictions are
    random; here ``eval()`` applies neither dropout."""

    def __init__(self, feature_nums, field_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)
        if output_dim != 1:
            raise NotImplementedError("AFM: output_dim must be 1 (the reference's only use)")
        if field_nums < 2:
            raise NotImplementedError("AFM: field_nums must be at least 2 (there is no pair to "
                                      "attend over otherwise)")
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.latent_dims = latent_dims
        self.feature_embedding = nn.Embedding(self.feature_nums, self.latent_dims)
        # the reference's pair lists (p_model.py:451-454), kept for API parity
        self.row, self.col = [], []
        for i in range(self.field_nums - 1):
            for j in range(i + 1, self.field_nums):
                self.row.append(i), self.col.append(j)
        attention_factor = self.latent_dims
        self.attention_net = nn.Linear(self.latent_dims, attention_factor)
        self.attention_softmax = nn.Linear(attention_factor, 1)
        self.fc = nn.Linear(self.latent_dims, output_dim)
        self.linear = nn.Embedding(self.feature_nums, output_dim)
        self.bias = nn.Parameter(torch.zeros((output_dim,)))
        self.drop_p = 0.2

    def forward(self, x):
        E = self.feature_embedding.weight
        an, asm = self.attention_net, self.attention_softmax
        drop = float(self.drop_p) if self.training else 0.0
        seed = _rng_dropout_seed() if drop > 0.0 else 0
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            pooled = _AFMPart.apply(x, E, an.weight, an.bias, asm.weight, asm.bias, drop, seed)
            z = _LRPart.apply(x, self.linear.weight, self.bias) + _LinearAct.apply(
                pooled, self.fc.weight, self.fc.bias, False, 0.0, 0)
            return torch.sigmoid(z)
        with torch.no_grad():
            pooled, _ = hip_ops.afm_forward(x, E.detach(), an.weight.detach(), an.bias.detach(),
                                            asm.weight.detach().reshape(-1), asm.bias.detach(),
                                            drop, seed, want_attn=False)
            z_lr = hip_ops.lr_forward(x, self.linear.weight.detach(), self.bias.detach(),
                                      want_p=False)["z"]
            head = hip_ops.deepfm_head(pooled, self.fc.weight.detach(), self.fc.bias.detach(), z_lr)
            return head["p"].view(-1, 1)


class FFM(nn.Module):
    """p_model.py:59-100: z = bias + sum_f w[x_f] + sum_{i<j} <E_j[x_i], E_i[x_j]>, one
    nn.Embedding(V, K) per field (same construction order and state_dict keys)."""

    def __init__(self, feature_nums, field_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)
        if output_dim != 1:
            raise NotImplementedError("FFM: output_dim must be 1 (the reference's only use)")
        self.field_nums = field_nums
        self.linear = nn.Embedding(feature_nums, output_dim)
        self.bias = nn.Parameter(torch.zeros((output_dim,)))
        self.field_feature_embeddings = nn.ModuleList([
            nn.Embedding(feature_nums, latent_dims) for _ in range(field_nums)])
        self._ptrs = hip_ops.FFMTables()

    def forward(self, x):
        tabs = [e.weight for e in self.field_feature_embeddings]
        ptrs = self._ptrs.get(tabs)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return torch.sigmoid(_FFMPart.apply(x, self.linear.weight, self.bias, ptrs, *tabs))
        with torch.no_grad():
            z = hip_ops.ffm_forward(x, [t.detach() for t in tabs], ptrs,
                                    self.linear.weight.detach(), self.bias.detach())["z"]
            return torch.sigmoid(z).view(-1, 1)


class FNN(nn.Module):
    """p_model.py:326-373: MLP [F*K -> 300 -> 200 -> 1] (ReLU, Dropout 0.2) over the flat
    embeddings (DeepFM's deep half alone); load_embedding takes the FM-pretrained table."""

    def __init__(self, feature_nums, field_nums, latent_dims):
        super().__init__()
        latent_dims = int(latent_dims)
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.latent_dims = latent_dims
        self.feature_embedding = nn.Embedding(self.feature_nums, self.latent_dims)
        deep_input_dims = self.field_nums * self.latent_dims
        layers = []
        for neuron_num in (300, 200):
            layers.append(nn.Linear(deep_input_dims, neuron_num))
            layers.append(nn.ReLU())
            layers.append(nn.Dropout(p=0.2))
            deep_input_dims = neuron_num
        layers.append(nn.Linear(deep_input_dims, 1))
        self.mlp = nn.Sequential(*layers)

    def load_embedding(self, pretrain_params):
        self.feature_embedding.weight.data.copy_(
            torch.from_numpy(np.array(pretrain_params["feature_embedding.weight"].cpu())))

    def forward(self, x):
        E = self.feature_embedding.weight
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            flat = _GatherFlat.apply(x, E)
            seed_fn = _rng_dropout_seed if self.training else _dropout_seed
            return torch.sigmoid(mlp_forward(self.mlp, flat, self.training, seed_fn))
        with torch.no_grad():
            B, F = x.shape
            h = hip_ops.embedding_gather(E.detach(), x).view(B, F * E.shape[1])
            m = self.mlp
            p0 = m[2].p if self.training else 0.0
            p1 = m[5].p if self.training else 0.0
            seed_fn = _rng_dropout_seed if self.training else _dropout_seed
            h = hip_ops.linear(h, m[0].weight, m[0].bias, relu=True, drop_p=p0,
                               seed=seed_fn())
            h = hip_ops.linear(h, m[3].weight, m[3].bias, relu=True, drop_p=p1,
                               seed=seed_fn())
            zero = torch.zeros(h.shape[0], dtype=torch.float32, device=h.device)
            head = hip_ops.deepfm_head(h, m[6].weight, m[6].bias, zero)
            return head["p"].view(-1, 1)


class DCN(nn.Module):
    """p_model.py:376-435: a 5-layer cross network x_{i+1} = x0 * <x_i, w_i> + b_i + x_i beside
    the deep network DN [F*K -> 300 -> 200] (ReLU, Dropout 0.2), both over the flat embeddings;
    p = sigmoid(linear(cat[x_5, dn])). The final Linear is split at column F*K: the cross
    kernel emits <x_5, w[:F*K]> itself, so neither x_5 nor the concatenation is materialised."""

    def __init__(self, feature_nums, field_nums, latent_dims, output_dim=1):
        super().__init__()
        latent_dims = int(latent_dims)
        if output_dim != 1:
            raise NotImplementedError("DCN: output_dim must be 1 (the reference's only use)")
        self.feature_nums = feature_nums
        self.field_nums = field_nums
        self.latent_dims = latent_dims
        self.feature_embedding = nn.Embedding(self.feature_nums, self.latent_dims)
        deep_input_dims = self.field_nums * self.latent_dims
        deep_net_layers = []
        neural_nums = [300, 200]
        self.num_neural_layers = 5
        for neural_num in neural_nums:
            deep_net_layers.append(nn.Linear(deep_input_dims, neural_num))
            deep_net_layers.append(nn.ReLU())
            deep_net_layers.append(nn.Dropout(p=0.2))
            deep_input_dims = neural_num
        self.DN = nn.Sequential(*deep_net_layers)
        cross_input_dims = self.field_nums * self.latent_dims
        self.cross_net_w = nn.ModuleList([
            nn.Linear(cross_input_dims, output_dim, bias=False)
            for _ in range(self.num_neural_layers)])
        self.cross_net_b = nn.ParameterList([
            nn.Parameter(torch.zeros((cross_input_dims,)))
            for _ in range(self.num_neural_layers)])
        self.linear = nn.Linear(neural_nums[-1] + cross_input_dims, output_dim)

    def _cross_params(self):
        W = torch.cat([lin.weight for lin in self.cross_net_w], dim=0)  # [L, D]
        b = torch.stack(list(self.cross_net_b), dim=0)
        return W, b

    def forward(self, x):
        E = self.feature_embedding.weight
        D = self.field_nums * self.latent_dims
        lw = self.linear.weight  # [1, D + 200]: cross columns, then deep columns
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            flat = _GatherFlat.apply(x, E)
            W, b = self._cross_params()
            z_cross = _CrossPart.apply(flat, W, b, lw[0, :D].contiguous())
            seed_fn = _rng_dropout_seed if self.training else _dropout_seed
            dn = mlp_forward(self.DN, flat, self.training, seed_fn)
            z_deep = _LinearAct.apply(dn, lw[:, D:].clone(), self.linear.bias, False, 0.0, 0)
            return torch.sigmoid(z_cross + z_deep)
        with torch.no_grad():
            B, F = x.shape
            flat = hip_ops.embedding_gather(E.detach(), x).view(B, D)
            W, b = self._cross_params()
            z_cross = hip_ops.dcn_cross_forward(flat, W, b, lw[0, :D].contiguous(),
                                                want_xl=False)["z"]
            m = self.DN
            p0 = m[2].p if self.training else 0.0
            p1 = m[5].p if self.training else 0.0
            seed_fn = _rng_dropout_seed if self.training else _dropout_seed
            h = hip_ops.linear(flat, m[0].weight, m[0].bias, relu=True, drop_p=p0,
                               seed=seed_fn())
            h = hip_ops.linear(h, m[3].weight, m[3].bias, relu=True, drop_p=p1,
                               seed=seed_fn())
            head = hip_ops.deepfm_head(h, lw[:, D:].clone(), self.linear.bias, z_cross)
            return head["p"].view(-1, 1)
