"""The fused AFM training step: the reference's per-batch body
(all_main/pretrain_main.py:72-79: ``y = model(x); loss = BCELoss(y, labels);
model.zero_grad(); loss.backward(); optimizer.step()``) for AFM (p_model.py:438-486) with
torch.optim.Adam(lr, weight_decay) — dense Adam semantics (every row of both tables moves
every step), computed deferred-exact like FusedCTRTrainer's default mode.

``feature_embedding.weight`` [V, K] and ``linear.weight`` [V, 1] are the (E, w) pair of one
deferred-Adam table, so one sparse plan over the batch's ids serves both; the seven dense
parameters (bias, the attention network, the attention softmax, fc) are re-pointed into one
flat buffer with a flat gradient and flat moments (step_trainer.pack_dense).

  plan over x                      the batch's unique rows
  deferred catch-up of those rows  (they replay the g = wd*p steps they missed)
  afm_forward(step_dev)            pooled [B, K], attn [B, P]; dropout seeded by the step
  afm_head                         z, p, per-example loss, dL/dz, dL/dpooled
  afm_backward(step_dev)           per-slot gradients dslot [B*F, K]; dW1, db1, dw2, db2
                                   straight into the flat gradient
  scatter                          a slot's embedding gradient is its row of dslot, its linear
                                   gradient its example's dL/dz: Wide&Deep's scatter, with the
                                   Adam apply fused where FusedCTRTrainer fuses it
  colsum_multi                     fc.weight grad = sum_b gz[b] pooled[b, :], fc.bias grad
  fm_step_tail                     batch loss, bias grad, dense Adam over the flat buffer,
                                   step counters, loss_sum

No dense [V, .] gradient is materialised (AutogradTrainer densifies two and runs
torch.optim.Adam over every row of both tables, every batch). The step bookkeeping, the
optimiser interface and the capture / replay of the step as a HIP graph are StepTrainer's
(step_trainer.py): one graph per batch shape and dropout rate; the dropout masks follow the
device step counter (ctr_afm_forward_step), so a replay draws the masks of its own step.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn

from . import hip_ops
from .distributed import world
from .p_model import AFM
from .step_trainer import StepTrainer, pack_dense

AFM_DENSE = ("bias", "attention_net.weight", "attention_net.bias", "attention_softmax.weight",
             "attention_softmax.bias", "fc.weight", "fc.bias")


@dataclass
class _AFMBufs:
    B: int
    plan: hip_ops.SparsePlanBuffers    # over x (V rows of both tables)
    pooled: torch.Tensor               # [B, K]
    attn: torch.Tensor                 # [B, P]
    head: dict                         # z, p, loss_elem, gz [B], dpooled [B, K]
    bwd: dict                          # dslot [B*F, K] and the four sums' flat-gradient views
    grad_rows: torch.Tensor            # [B*F, K] per-row sums (scratch; kept with keep_grads)
    grad_lin: torch.Tensor             # [B*F]
    loss: torch.Tensor                 # [1]


class FusedAFMTrainer(StepTrainer):
    """Fused forward + BCE + backward + dense Adam for AFM.

    Args mirror ``torch.optim.Adam(model.parameters(), lr, betas, eps, weight_decay)``; the
    interface (step / flush / reset_optimizer / optimizer_state_dict / check_errors), the
    step bookkeeping and the graph replay are StepTrainer's. optimizer_mode "deferred"
    (default) or "dense": identical results, bitwise."""

    NAME = "FusedAFMTrainer"
    MIN_BATCH = 1

    def __init__(self, model: nn.Module, lr: float = 1e-3, weight_decay: float = 0.0,
                 betas=(0.9, 0.999), eps: float = 1e-8, seed: int | None = None,
                 optimizer_mode: str = "deferred"):
        if not isinstance(model, AFM):
            raise TypeError("FusedAFMTrainer drives AFM")
        E = model.feature_embedding.weight
        if E.device.type == "cuda" and world()[1] > 1:  # a host model: refused as such below
            raise RuntimeError("FusedAFMTrainer runs in one process (no sharded or replicated "
                               "AFM step)")
        if optimizer_mode not in ("deferred", "dense"):
            raise ValueError(f"optimizer_mode must be 'deferred' or 'dense', not {optimizer_mode!r}")
        self.kind = "AFM"
        self.optimizer_mode = optimizer_mode
        self.V, self.K = E.shape
        self.F = int(model.field_nums)
        super().__init__(model, E.device, self.K, lr, weight_decay, betas, eps, seed,
                         deferred=optimizer_mode == "deferred")
        dev = self.device
        # the dense parameters in one flat buffer
        self.dense_names = AFM_DENSE
        self.flat, self.flat_grad, self.offsets, self.views, self.grad_views = pack_dense(
            dict(model.named_parameters()), AFM_DENSE, dev)
        self.m_flat = torch.zeros_like(self.flat)
        self.v_flat = torch.zeros_like(self.flat)
        # the two tables: one deferred (E, m_E, v_E, w, m_w, v_w, last) table
        self.E_tab = E.data
        self.w_tab = model.linear.weight.data
        self.m_E = torch.zeros_like(self.E_tab)
        self.v_E = torch.zeros_like(self.E_tab)
        self.m_w = torch.zeros(self.V, dtype=torch.float32, device=dev)
        self.v_w = torch.zeros_like(self.m_w)
        self.last = torch.zeros(self.V, dtype=torch.int32, device=dev)
        self.rowmap = torch.full((self.V,), -1, dtype=torch.int32, device=dev)  # dense mode

    # ----------------------------------------------------------------- optimiser -----
    def _table_args(self):
        return (self.E_tab, self.m_E, self.v_E, self.w_tab, self.m_w, self.v_w, self.last)

    def _tables(self):
        return (self._table_args(),)

    def _moments(self) -> dict:
        return {"feature_embedding.weight": (self.m_E, self.v_E),
                "linear.weight": (self.m_w.view(-1, 1), self.v_w.view(-1, 1)),
                **self._flat_moments()}

    # --------------------------------------------------------------------- buffers ---
    def _buffers(self, B: int, F: int) -> _AFMBufs:
        # one buffer set per batch shape, never freed: captured HIP graphs hold their addresses
        b = self._bufsets.get((B, F))
        if b is None:
            dev, K = self.device, self.K
            S, P = B * F, F * (F - 1) // 2
            e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
            gv = self.grad_views
            b = _AFMBufs(B=B, plan=hip_ops.SparsePlanBuffers(S, dev), pooled=e(B, K),
                         attn=e(B, P),
                         head=dict(z=e(B), p=e(B), loss_elem=e(B), gz=e(B), dpooled=e(B, K)),
                         bwd=dict(dslot=e(max(S, 1), K), dW1=gv["attention_net.weight"],
                                  db1=gv["attention_net.bias"],
                                  dw2=gv["attention_softmax.weight"].view(-1),
                                  db2=gv["attention_softmax.bias"]),
                         grad_rows=e(max(S, 1), K), grad_lin=e(max(S, 1)), loss=e(1))
            self._bufsets[(B, F)] = b
        self._bufs = b
        return b

    # ------------------------------------------------------------------------ step ----
    def _drop_p(self) -> float:
        return float(self.model.drop_p) if self.model.training else 0.0

    def _graph_key(self) -> tuple:
        return (self._drop_p(),)  # the dropout rate is a launch argument

    def _launch(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Enqueue one step; step-dependent values (the Adam step, the dropout seed) come
        from the device step counter, so the launch sequence can be captured."""
        B, F = x.shape
        K = self.K
        b = self._buffers(B, F)
        y = self._float_labels(y)
        m, vw, gv = self.model, self.views, self.grad_views
        E, w = m.feature_embedding.weight.data, m.linear.weight.data
        W1, b1 = vw["attention_net.weight"], vw["attention_net.bias"]
        w2, b2 = vw["attention_softmax.weight"].view(-1), vw["attention_softmax.bias"]
        table = self._table_args()
        hint = self.step_count + 1
        opt = dict(betas=self.betas, eps=self.eps, weight_decay=self.weight_decay)
        drop = self._drop_p()
        # the batch's rows, caught up before the forward reads them
        b.plan.build(x, self.V, err_flag=self.err)
        if self.deferred:
            hip_ops.adam_deferred_rows(*table, b.plan, hint, self.step_table, **opt,
                                       step_dev=self.step_done)
        # forward, head, backward: the dropout masks of the step in flight (completed steps)
        hip_ops.afm_forward(x, E, W1, b1, w2, b2, drop, self.seed, out=b.pooled, attn=b.attn,
                            err_flag=self.err, step_dev=self.step_done)
        head = hip_ops.afm_head(x, w, vw["bias"], b.pooled, vw["fc.weight"], vw["fc.bias"], y,
                                mean_div=B, out=b.head, err_flag=self.err)
        gz = head["gz"]
        hip_ops.afm_backward(x, E, W1, b1, w2, b2, b.attn, head["dpooled"], drop, self.seed,
                             out=b.bwd, err_flag=self.err, step_dev=self.step_done)
        # scatter: Wide&Deep's contract with dX = dslot viewed [B, F*K]
        dx = b.bwd["dslot"]
        fused = (self.deferred and self._vec_ok and self.fuse_apply
                 and K >= self.fuse_apply_min_k)
        if fused:
            hip_ops.wd_embedding_grad_adam(b.plan, F, gz, dx, table, step_dev=self.step_cur,
                                           step_table=self.step_table, step=hint, **opt,
                                           grad_rows=b.grad_rows, grad_lin=b.grad_lin,
                                           keep_sums=self.keep_grads)
        elif self.deferred:
            hip_ops.wd_embedding_grad(b.plan, F, K, gz, dx, None, grad_rows=b.grad_rows,
                                      grad_lin=b.grad_lin)
            hip_ops.adam_deferred_rows(*table, b.plan, hint, self.step_table, **opt,
                                       grad_rows=b.grad_rows, grad_lin=b.grad_lin,
                                       step_dev=self.step_cur)
        else:  # one streaming pass over all V rows (rowmap-gated gradients)
            hip_ops.wd_embedding_grad(b.plan, F, K, gz, dx, self.rowmap, grad_rows=b.grad_rows,
                                      grad_lin=b.grad_lin)
            hip_ops.adam_embedding(*table[:6], self.rowmap, b.grad_rows, b.grad_lin, hint,
                                   self.lr, **opt, step_dev=self.step_cur, table=self.step_table)
        # fc: dW = gz^T pooled, db = sum gz
        hip_ops.colsum_multi([(b.pooled, gz, gv["fc.weight"].view(-1)),
                              (gz.view(B, 1), None, gv["fc.bias"].view(1))])
        # batch loss, bias gradient, the flat dense Adam, the step counters, loss_sum
        hip_ops.fm_step_tail(head["loss_elem"], gz, 1.0 / B, b.loss, gv["bias"].view(1),
                             self.flat, self.flat_grad, self.m_flat, self.v_flat,
                             self.step_table, hint, self.step_ctr, **opt,
                             loss_sum=self.loss_sum)
        return b.loss
