"""What every graph-captured training step shares: ``StepTrainer``, the base of
FusedCTRTrainer (trainer.py), ShardedCTRTrainer (sharded.py), FusedFFMTrainer (ffm_trainer.py)
and FusedAFMTrainer (afm_trainer.py).

A subclass supplies its model's tables and launch sequence; the base owns, once,
  - the optimiser state around them: the device step counters, the per-step Adam scalars
    (hip_ops.AdamStepTable), flush / reset_optimizer / optimizer_state_dict over the subclass's
    ``_tables()`` and ``_moments()``, the bounded staleness of deferred Adam;
  - the lifetime rules of captured step graphs: an own graph pool, scratch and capture stream,
    graphs dropped when the step table moves (``_sync_step_table``), and "run the step once
    for real, capture it once, replay it after" (``_replay_or_capture``);
  - the single-process default step on fixed input buffers (step / _step / _graph_step), which
    the two small trainers inherit whole and FusedCTRTrainer replaces by its slot ring.

pack_dense / split_dense are the flat dense-parameter buffer and its inverse; graph_capture,
live_pool and flush_hooks are the helpers PolicyGradient (pg_model.py) shares with the trainers.
"""
from __future__ import annotations

import contextlib
import gc
import os
import weakref

import torch
import torch.nn as nn

from . import hip_ops


@contextlib.contextmanager
def graph_capture(g, **kw):
    """torch.cuda.graph with Python's cyclic GC paused: a collection during the capture
    could destroy another trainer's captured graphs (HIP calls that are illegal while a
    stream captures -> abort)."""
    gc.collect()  # dead cycles holding captured graphs die here, outside any capture
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, **kw):
            yield
    finally:
        if was:
            gc.enable()


def live_pool(owner):
    """The graph memory pool handle of `owner` (a trainer / PolicyGradient) for its next
    capture: torch frees a shared pool once every graph captured into it is gone, and a
    capture into the freed pool's handle trips an allocator assert (and leaves the RNG in
    capture state), so an owner whose step graphs were all dropped starts a new pool."""
    if not owner._graphs:
        owner._graph_pool = torch.cuda.graph_pool_handle()
    return owner._graph_pool


def flush_hooks(model: nn.Module, trainer) -> None:
    """forward / state_dict / load_state_dict pre-hooks that flush the trainer's deferred rows,
    holding the trainer weakly (no model <-> trainer cycle: a dropped trainer is freed at once).
    Before a load too: the loaded values must land on rows that owe no step (a later flush
    would replay the old values' missed steps on them) and after a pending weight-gradient
    tail."""
    ref = weakref.ref(trainer)

    def flush(*_):
        t = ref()
        if t is not None:
            t.flush()
    model.register_forward_pre_hook(flush)
    model.register_state_dict_pre_hook(flush)
    model._register_load_state_dict_pre_hook(flush)


def pack_dense(named_params: dict, names, device, grad_tail: int = 0):
    """Re-point the parameters `names` of `named_params` into one flat float32 buffer (same
    Parameter objects, same values, same state_dict) and return (flat, flat_grad, offsets,
    views, grad_views). Offsets are multiples of 4 floats: the GEMMs read the weights through
    the float4 / LDS-DMA path only when a row start is 16-B aligned. flat_grad has flat's
    length, with `grad_tail` more floats of storage behind it (the row-sharded step
    all-reduces the batch loss there, in the gradient's own collective)."""
    offsets, total = {}, 0
    for n in names:
        offsets[n] = total
        total += (named_params[n].numel() + 3) // 4 * 4
    flat = torch.zeros(total, dtype=torch.float32, device=device)
    flat_grad = torch.zeros(total + grad_tail, dtype=torch.float32, device=device)[:total]
    views, grad_views = {}, {}
    for n in names:
        p, off = named_params[n], offsets[n]
        k = p.numel()
        flat[off:off + k].copy_(p.data.reshape(-1))
        p.data = flat[off:off + k].view_as(p)
        views[n] = p.data
        grad_views[n] = flat_grad[off:off + k].view_as(p)
    return flat, flat_grad, offsets, views, grad_views


def split_dense(flat: torch.Tensor, names, offsets: dict, views: dict) -> dict:
    """pack_dense's inverse on any buffer of flat's layout (the parameters, a moment):
    {name: its view, shaped like the parameter}."""
    return {n: flat[offsets[n]:offsets[n] + views[n].numel()].view_as(views[n]) for n in names}


class StepTrainer:
    """The shared part of the fused trainers. A subclass's ``__init__`` checks its model,
    calls this one, then builds its tables; it defines

      _tables()    the deferred-Adam tables, each (E, m_E, v_E, w, m_w, v_w, last)
      _moments()   {parameter name: (exp_avg, exp_avg_sq)} for every model parameter
      _buffers(B, F), _launch(x, y)    the per-shape buffers (``.loss`` [1]) and the launches
                                       of one step, capturable: no host state changes

    and may override _graph_key (what besides the batch shape is a launch argument),
    _new_capture_stream, _drain_tail and the step methods themselves."""

    NAME = "StepTrainer"      # the class name the messages carry (subclasses of it too)
    MAX_GRAPHS = 8
    MIN_BATCH = 0
    _SYNC_BEFORE_DEL = ("_graphs",)  # attributes that hold captured graphs

    def __init__(self, model: nn.Module, device, K: int, lr, weight_decay, betas, eps, seed,
                 deferred: bool = True):
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), betas, eps
        self.device = device
        if device.type != "cuda":
            raise RuntimeError(f"{self.NAME} needs the model on a ROCm device")
        # "deferred": deferred-exact dense Adam (csrc/adam.hip), flushed before anything reads
        # a table; otherwise one streaming pass over every row, every step
        self.deferred = deferred
        # device step counters: [0] completed steps, [1] the step in flight (ctr_step_begin/end)
        # initialised to {0, 1}: ctr_step_end advances both, so no step-begin launch is needed
        self.step_ctr = torch.tensor([0, 1], dtype=torch.int32, device=device)
        self.step_done, self.step_cur = self.step_ctr[0:1], self.step_ctr[1:2]
        self.step_table = hip_ops.AdamStepTable(self.lr, self.betas, device)
        self.err = torch.zeros(1, dtype=torch.int32, device=device)
        # every step's mean loss added in float64 by its last launch (the driver's epoch sum)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=device)
        self.step_count = 0
        self._dirty = False
        if deferred:  # nothing may read a table with rows still owed steps
            flush_hooks(model, self)
        # bounded staleness of deferred Adam: every `flush_every` steps all rows are brought
        # to the current step (one tiled flush pass), so a row a batch touches has missed at
        # most that many steps and the in-step catch-up replays stay short under a stream
        # of fresh batches (0: only at forward / state_dict / epoch end)
        self.flush_every = int(os.environ.get("CTR_FLUSH_EVERY", "32"))
        self._flushed_at = 0
        # fused scatter + Adam apply where the row sums complete: the vector kernels' K rule,
        # the switch and the smallest K it is used at (A/B: CTR_FUSE_APPLY, CTR_FUSE_APPLY_MIN_K);
        # keep_grads keeps every row's gradient sum in the step's buffers (tests read them)
        self._vec_ok = K % 4 == 0 and 64 % (K // 4 or 1) == 0 and K <= 256
        self.fuse_apply = os.environ.get("CTR_FUSE_APPLY", "1") != "0"
        self.fuse_apply_min_k = int(os.environ.get("CTR_FUSE_APPLY_MIN_K", "16"))
        self.keep_grads = False
        self.seed = int(torch.initial_seed() if seed is None else seed) & (2**63 - 1)
        # scratch and a capture stream owned by this trainer alone: its captured graphs
        # reference no buffer that another object's launches use (hip_ops.Workspace)
        self._scratch = hip_ops.Workspace()
        self._capture_stream = self._new_capture_stream()
        # one buffer set per batch shape, never freed: captured HIP graphs hold their
        # addresses (a ragged last batch must not invalidate the full-batch graphs)
        self._bufs = None
        self._bufsets: dict = {}
        # the default step: every batch is copied into the fixed input buffers of its shape
        # (ids, labels), so one captured graph per shape serves a stream of fresh batches
        self._inputs: dict = {}
        self.use_graphs = True
        self.max_graphs = self.MAX_GRAPHS
        self._graphs: dict = {}    # key -> (graph, the buffer set it was captured with)
        self.captures = 0          # step graphs captured (tests: bounded, batch-independent)
        self._graph_pool = torch.cuda.graph_pool_handle()
        self._graph_tab_version = self.step_table.version
        # bench hook: {"adam": [], "gather": [], ...} -> [(start, end, work)] HIP events
        # recorded on the launch stream around those kernels; only the keys present in the
        # dict are instrumented (each event is a queue packet: keep the timed region lean)
        self.timing: dict | None = None

    def __del__(self):
        # a captured graph must not be destroyed while it still runs (replays on a plan stream
        # are not ordered before anything the caller synchronises with)
        try:
            if any(getattr(self, a, None) for a in self._SYNC_BEFORE_DEL):
                torch.cuda.synchronize(self.device)
        except Exception:  # interpreter shutdown
            pass

    def _new_capture_stream(self):
        return torch.cuda.Stream(device=self.device)

    def _mark(self, key):
        if self.timing is None or key not in self.timing:
            return None
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def _span(self, key, start, work=None):
        if start is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.timing[key].append((start, ev, work))

    # ----------------------------------------------------------------- optimiser -----
    def _tables(self):
        raise NotImplementedError

    def _moments(self) -> dict:
        raise NotImplementedError

    def _dense_moments(self) -> tuple:
        """The moments of the parameters outside the tables."""
        return (self.m_flat, self.v_flat)

    def _flat_moments(self) -> dict:
        """_moments() of the parameters packed by pack_dense (m_flat, v_flat)."""
        m, v = (split_dense(f, self.dense_names, self.offsets, self.views)
                for f in (self.m_flat, self.v_flat))
        return {n: (m[n], v[n]) for n in self.dense_names}

    def _drain_tail(self) -> None:
        """Apply work a step left pending (flush() starts with it): none here;
        FusedCTRTrainer's pipelined weight-gradient tail."""

    def flush(self) -> None:
        """Apply whatever the last step left pending and bring every row of every table up to
        the last completed step (deferred mode): every parameter and moment is then the
        reference's after that step."""
        self._drain_tail()
        self._flush_table()

    def _flush_table(self) -> None:
        """The tables' rows up to the last completed step (deferred mode)."""
        self._flushed_at = self.step_count
        if self.deferred and self._dirty and self.step_count > 0:
            t = self._mark("flush")
            for tab in self._tables():
                hip_ops.adam_deferred_flush(*tab, self.step_count, self.step_table, self.betas,
                                            self.eps, self.weight_decay)
            self._span("flush", t)
        self._dirty = False

    def _flush_due(self) -> bool:
        """True when `flush_every` steps have passed since the last flush."""
        return (self.deferred and self.flush_every > 0
                and self.step_count - self._flushed_at >= self.flush_every)

    def _bound_staleness(self) -> None:
        """Flush once `flush_every` steps have passed since the last flush: no row is then
        more than that many steps behind when a batch reads it."""
        if self._flush_due():
            self._flush_table()  # the tables only: a pending tail stays pending

    def reset_optimizer(self, lr: float | None = None) -> None:
        """What ``torch.optim.Adam(...)`` re-created every epoch does
        (all_main/pretrain_main.py:153): fresh moments, step 0 — with `lr`, at a new
        learning rate (main/pretrain_main.py:180-181: ``learning_rate += 1e-4`` then a new
        Adam): the per-step scalars are rewritten in place (captured graphs stay valid)."""
        self.flush()
        if lr is not None:
            self.lr = float(lr)
            self.step_table.set_lr(self.lr)
        for tab in self._tables():
            for t in tab[1:3] + tab[4:]:  # m_E, v_E, m_w, v_w (None: no linear part), last
                if t is not None:
                    t.zero_()
        for t in self._dense_moments():
            t.zero_()
        self.step_ctr.copy_(torch.tensor([0, 1], dtype=torch.int32))
        self.step_count = 0
        self._flushed_at = 0

    def optimizer_state_dict(self) -> dict:
        """torch.optim.Adam-compatible state_dict: parameter i is the i-th entry of
        model.named_parameters() (a root module's own parameters come before its
        submodules')."""
        self.flush()
        moments = self._moments()
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

    def reset_loss_sum(self) -> None:
        """Zero the device loss accumulator (on the current stream, in step order)."""
        self.loss_sum.zero_()

    def read_loss_sum(self) -> float:
        """The sum of every step's mean loss since reset_loss_sum(), accumulated on the
        device in float64 in step order: bitwise the reference's per-step
        ``total_loss += loss.item()`` (all_main/pretrain_main.py:79). Syncs once."""
        return float(self.loss_sum.item())

    # ---------------------------------------------------------------- step graphs ----
    def _sync_step_table(self) -> None:
        """Before a graph step: room in the step table for this step and the next, and no
        graph that holds a moved table's address (it would read freed memory)."""
        tab = self.step_table
        if tab.capacity < self.step_count + 2:
            tab.ensure(max(self.step_count + 2, 2 * tab.capacity))
        if self._graph_tab_version != tab.version:
            torch.cuda.synchronize(self.device)  # none may still run when destroyed
            self._graphs.clear()  # they hold the old table's address
            self._graph_tab_version = tab.version

    def _replay_or_capture(self, key, launch, on_hit=None, **capture_kw):
        """The step of graph key `key`: replayed if captured; else `launch()` runs it for
        real (which also sizes every buffer) and, while the cache has room, is captured — not
        executed — for the steps after. on_hit(bufs): called with the graph's buffer set
        before a replay. launch is only called on a miss. Returns the step's loss buffer."""
        hit = self._graphs.get(key)
        if hit is None:
            loss = launch()
            self._after_step()
            if len(self._graphs) < self.max_graphs:
                g = torch.cuda.CUDAGraph()
                with graph_capture(g, pool=live_pool(self), stream=self._capture_stream,
                                   **capture_kw):
                    launch()
                self._graphs[key] = (g, self._bufs)
                self.captures += 1
            return loss
        g, self._bufs = hit  # the buffer set the graph was captured with
        if on_hit is not None:
            on_hit(self._bufs)
        g.replay()
        self._after_step()
        return self._bufs.loss

    def _after_step(self) -> None:
        """Host mirrors of what a step did on the device."""
        self.step_count += 1
        if self.deferred:
            self._dirty = True

    # ----------------------------------------------------- the default step ----------
    def step(self, x: torch.Tensor, y: torch.Tensor, return_loss: bool = True):
        """One training step on batch (x [B,F] int64/int32, y [B] 0/1); returns the mean
        BCE as a fresh 1-element device tensor (no host sync), or None with
        return_loss=False. Every step adds its loss to ``loss_sum`` (float64, on the device;
        read_loss_sum / reset_loss_sum). The first step of a batch shape runs eagerly and is
        captured; later ones replay its HIP graph."""
        with self._scratch.scope():  # this trainer's own scratch (hip_ops.Workspace)
            loss = self._step(x, y)
            return loss.clone() if return_loss else None

    def _step(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        B, F = x.shape
        if F != self.F:
            raise ValueError(f"{self.NAME}: batch has {F} fields, model {self.F}")
        if B < self.MIN_BATCH:
            raise ValueError(f"{self.NAME}: empty batch")
        self._bound_staleness()
        if self.use_graphs:
            return self._graph_step(x, y)
        self.step_table.ensure(self.step_count + 1)
        loss = self._launch(x, y)
        self._after_step()
        return loss

    def _graph_key(self) -> tuple:
        """The launch arguments, besides the batch shape, that a captured step holds."""
        return ()

    def _graph_step(self, x, y):
        self._sync_step_table()
        B, F = x.shape
        shape = (B, F, x.dtype)
        inp = self._inputs.get(shape)
        if inp is None:
            inp = self._inputs[shape] = (torch.empty(B, F, dtype=x.dtype, device=self.device),
                                         torch.empty(B, dtype=torch.float32, device=self.device))
        xs, ys = inp
        xs.copy_(x, non_blocking=True)
        ys.copy_(y.reshape(-1), non_blocking=True)
        return self._replay_or_capture((shape,) + self._graph_key(),
                                       lambda: self._launch(xs, ys))

    @staticmethod
    def _float_labels(y: torch.Tensor) -> torch.Tensor:
        """The labels as the kernels read them: flat, float32, contiguous."""
        y = y.reshape(-1)
        if y.dtype != torch.float32:
            y = y.float()
        return y.contiguous()
