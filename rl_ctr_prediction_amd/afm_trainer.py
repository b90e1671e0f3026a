"""The fused AFM training step: the reference's per-batch body
(all_main/pretrain_main.py:72-79: ``y = model(x); loss = BCELoss(y, labels);
model.zero_grad(); loss.backward(); optimizer.step()``) for AFM (p_model.py:438-486) with
torch.optim.Adam(lr, weight_decay) — dense Adam semantics (every row of both tables moves
every step), computed deferred-exact like FusedCTRTrainer's default mode.

``feature_embedding.weight`` [V, K] and ``linear.weight`` [V, 1] are the (E, w) pair of one
deferred-Adam table, so one sparse plan over the batch's ids serves both; the seven dense
parameters (bias, the attention network, the attention softmax, fc) are re-pointed into one
flat buffer with a flat gradient and flat moments, as FusedCTRTrainer does with the MLP.

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
torch.optim.Adam over every row of both tables, every batch). Steps are captured into HIP
graphs and replayed, one graph per batch shape; the dropout masks follow the device step
counter (ctr_afm_forward_step), so a replay draws the masks of its own step.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import torch
import torch.nn as nn

from . import hip_ops
from .distributed import world
from .p_model import AFM
from .trainer import flush_hooks, graph_capture, live_pool

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


class FusedAFMTrainer:
    """Fused forward + BCE + backward + dense Adam for AFM.

    Args mirror ``torch.optim.Adam(model.parameters(), lr, betas, eps, weight_decay)``; the
    interface is FusedCTRTrainer's (step / flush / reset_optimizer / optimizer_state_dict /
    check_errors). optimizer_mode "deferred" (default) or "dense": identical results, bitwise."""

    def __init__(self, model: nn.Module, lr: float = 1e-3, weight_decay: float = 0.0,
                 betas=(0.9, 0.999), eps: float = 1e-8, seed: int | None = None,
                 optimizer_mode: str = "deferred"):
        if not isinstance(model, AFM):
            raise TypeError("FusedAFMTrainer drives AFM")
        E = model.feature_embedding.weight
        self.model = model
        self.kind = "AFM"
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), betas, eps
        self.device = E.device
        if self.device.type != "cuda":
            raise RuntimeError("FusedAFMTrainer needs the model on a ROCm device")
        if world()[1] > 1:
            raise RuntimeError("FusedAFMTrainer runs in one process (no sharded or replicated "
                               "AFM step)")
        if optimizer_mode not in ("deferred", "dense"):
            raise ValueError(f"optimizer_mode must be 'deferred' or 'dense', not {optimizer_mode!r}")
        self.optimizer_mode = optimizer_mode
        self.deferred = optimizer_mode == "deferred"
        self.V, self.K = E.shape
        self.F = int(model.field_nums)
        dev = self.device
        # the dense parameters in one flat buffer (16-B aligned views, as FusedCTRTrainer)
        named = dict(model.named_parameters())
        self.dense_names = AFM_DENSE
        self.offsets, total = {}, 0
        for n in self.dense_names:
            self.offsets[n] = total
            total += (named[n].numel() + 3) // 4 * 4
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros_like(self.flat)
        self.views, self.grad_views = {}, {}
        for n in self.dense_names:
            p, off = named[n], self.offsets[n]
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view_as(p)
            self.views[n] = p.data
            self.grad_views[n] = self.flat_grad[off:off + k].view_as(p)
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
        # FusedCTRTrainer's fuse rule: the scatter applies Adam where the row sums complete
        self._vec_ok = self.K % 4 == 0 and 64 % (self.K // 4 or 1) == 0 and self.K <= 256
        self.fuse_apply = os.environ.get("CTR_FUSE_APPLY", "1") != "0"
        self.fuse_apply_min_k = int(os.environ.get("CTR_FUSE_APPLY_MIN_K", "16"))
        self.keep_grads = False  # fused apply: keep every row's sum in grad_rows / grad_lin
        self.step_ctr = torch.tensor([0, 1], dtype=torch.int32, device=dev)
        self.step_done, self.step_cur = self.step_ctr[0:1], self.step_ctr[1:2]
        self.step_table = hip_ops.AdamStepTable(self.lr, self.betas, dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=dev)
        # own scratch and capture stream (hip_ops.Workspace: no captured graph shares
        # scratch with another object's launches)
        self._scratch = hip_ops.Workspace()
        self._capture_stream = torch.cuda.Stream(device=dev)
        self.step_count = 0
        self._dirty = False
        if self.deferred:  # nothing may read a table with rows still owed steps
            flush_hooks(model, self)
        self._bufs: _AFMBufs | None = None
        self._bufsets: dict = {}
        self.seed = int(torch.initial_seed() if seed is None else seed) & (2**63 - 1)
        self.use_graphs = True
        self.max_graphs = 8
        self._graphs: dict = {}
        # every batch is copied into the fixed input buffers of its shape (ids, labels), so
        # one captured graph per shape serves a stream of fresh batches
        self._inputs: dict = {}
        self.captures = 0
        # bounded staleness, as FusedCTRTrainer.flush_every
        self.flush_every = int(os.environ.get("CTR_FLUSH_EVERY", "32"))
        self._flushed_at = 0
        self._graph_pool = torch.cuda.graph_pool_handle()
        self._graph_tab_version = self.step_table.version
        self.timing = None  # FusedCTRTrainer's bench hook: not instrumented here

    def __del__(self):
        try:  # a captured graph must not be destroyed while it still runs
            if getattr(self, "_graphs", None):
                torch.cuda.synchronize(self.device)
        except Exception:  # interpreter shutdown
            pass

    # ----------------------------------------------------------------- optimiser -----
    def _table_args(self):
        return (self.E_tab, self.m_E, self.v_E, self.w_tab, self.m_w, self.v_w, self.last)

    def _drain_tail(self) -> None:
        """No work is ever pending across steps here (flush_hooks' load_state_dict hook)."""

    def flush(self) -> None:
        """Bring every row of both tables up to the last completed step (deferred mode)."""
        self._flushed_at = self.step_count
        if self.deferred and self._dirty and self.step_count > 0:
            hip_ops.adam_deferred_flush(*self._table_args(), self.step_count, self.step_table,
                                        self.betas, self.eps, self.weight_decay)
        self._dirty = False

    def reset_optimizer(self, lr: float | None = None) -> None:
        """A re-created torch.optim.Adam (all_main/pretrain_main.py:153), optionally at a new
        learning rate; captured graphs stay valid (the step table is rewritten in place)."""
        self.flush()
        if lr is not None:
            self.lr = float(lr)
            self.step_table.set_lr(self.lr)
        for t in (self.m_flat, self.v_flat, self.m_E, self.v_E, self.m_w, self.v_w, self.last):
            t.zero_()
        self.step_ctr.copy_(torch.tensor([0, 1], dtype=torch.int32))
        self.step_count = 0
        self._flushed_at = 0

    def optimizer_state_dict(self) -> dict:
        """torch.optim.Adam-compatible state_dict: parameter i is the i-th entry of
        model.named_parameters()."""
        self.flush()
        moments = {"feature_embedding.weight": (self.m_E, self.v_E),
                   "linear.weight": (self.m_w.view(-1, 1), self.v_w.view(-1, 1))}
        for n in self.dense_names:
            k, off = self.views[n].numel(), self.offsets[n]
            moments[n] = (self.m_flat[off:off + k].view_as(self.views[n]),
                          self.v_flat[off:off + k].view_as(self.views[n]))
        named = [n for n, _ in self.model.named_parameters()]
        state = {i: {"step": torch.tensor(float(self.step_count)),
                     "exp_avg": moments[n][0].clone(), "exp_avg_sq": moments[n][1].clone()}
                 for i, n in enumerate(named)}
        return {"state": state if self.step_count else {},
                "param_groups": [{"lr": self.lr, "betas": self.betas, "eps": self.eps,
                                  "weight_decay": self.weight_decay, "amsgrad": False,
                                  "params": list(range(len(named)))}]}

    def check_errors(self) -> None:
        """Raise IndexError if any kernel saw a feature id outside [0, V). Syncs."""
        hip_ops.check_index_error(self.err)

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
    def step(self, x: torch.Tensor, y: torch.Tensor, return_loss: bool = True):
        """One training step on batch (x [B,F] int64/int32, y [B] 0/1); returns the mean
        BCE as a fresh 1-element device tensor (no host sync), or None with
        return_loss=False. Every step adds its loss to ``loss_sum`` (float64, on the device;
        read_loss_sum / reset_loss_sum, as FusedCTRTrainer)."""
        with self._scratch.scope():
            loss = self._step(x, y)
            return loss.clone() if return_loss else None

    def reset_loss_sum(self) -> None:
        self.loss_sum.zero_()

    def read_loss_sum(self) -> float:
        return float(self.loss_sum.item())

    def _drop_p(self) -> float:
        return float(self.model.drop_p) if self.model.training else 0.0

    def _step(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        B, F = x.shape
        if F != self.F:
            raise ValueError(f"FusedAFMTrainer: batch has {F} fields, model {self.F}")
        if B < 1:
            raise ValueError("FusedAFMTrainer: empty batch")
        if (self.deferred and self.flush_every > 0
                and self.step_count - self._flushed_at >= self.flush_every):
            self.flush()
        if self.use_graphs:
            return self._graph_step(x, y)
        self.step_table.ensure(self.step_count + 1)
        loss = self._launch(x, y)
        self._after_step()
        return loss

    def _after_step(self) -> None:
        self.step_count += 1
        if self.deferred:
            self._dirty = True

    def _graph_step(self, x, y):
        if self.step_table.capacity < self.step_count + 2:
            self.step_table.ensure(max(self.step_count + 2, 2 * self.step_table.capacity))
        if self._graph_tab_version != self.step_table.version:
            torch.cuda.synchronize(self.device)  # none may still run when destroyed
            self._graphs.clear()  # they hold the old table's address
            self._graph_tab_version = self.step_table.version
        B, F = x.shape
        shape = (B, F, x.dtype)
        inp = self._inputs.get(shape)
        if inp is None:
            inp = self._inputs[shape] = (torch.empty(B, F, dtype=x.dtype, device=self.device),
                                         torch.empty(B, dtype=torch.float32, device=self.device))
        xs, ys = inp
        xs.copy_(x, non_blocking=True)
        ys.copy_(y.reshape(-1), non_blocking=True)
        key = (shape, self._drop_p())  # the dropout rate is a launch argument
        hit = self._graphs.get(key)
        if hit is None:
            loss = self._launch(xs, ys)  # the real step; also sizes every buffer
            self._after_step()
            if len(self._graphs) < self.max_graphs:
                g = torch.cuda.CUDAGraph()
                with graph_capture(g, pool=live_pool(self), stream=self._capture_stream):
                    self._launch(xs, ys)  # captured, not executed
                self._graphs[key] = (g, self._bufs)
                self.captures += 1
            return loss
        g, self._bufs = hit
        g.replay()
        self._after_step()
        return self._bufs.loss

    def _launch(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Enqueue one step; step-dependent values (the Adam step, the dropout seed) come
        from the device step counter, so the launch sequence can be captured."""
        B, F = x.shape
        K = self.K
        b = self._buffers(B, F)
        y = y.reshape(-1)
        if y.dtype != torch.float32:
            y = y.float()
        y = y.contiguous()
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
