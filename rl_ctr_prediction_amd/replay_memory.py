"""Prioritized experience replay of the hybrid TD3 agent, resident on the MI355X.

``Memory`` has the attribute names, defaults and method signatures of the reference's
``Hybrid_TD3_model_PER.Memory`` (src/models/Hybrid_TD3_model_PER.py:22-109), so it replaces
that class without another change to ``Hybrid_TD3_Model``. The reference samples on the host:
every ``stochastic_sample`` copies the whole priority column to numpy, runs
``np.random.choice(p=P, replace=False)`` and copies the indices back; ``greedy_sample`` sorts
the column. Here ``prioritys_`` and ``memory`` are device tensors that the kernels of
csrc/per.hip write in place, and add, both samplers and ``batch_update`` enqueue launches on
the current stream without a device-to-host copy or a host wait.

``stochastic_sample`` draws the same distribution (sequential weighted draws without
replacement, by the Gumbel top-k form), not numpy's random stream: the seed comes from
torch's CPU generator, so ``torch.manual_seed`` fixes the draw, or from ``seed=``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hip_ops

__all__ = ["Memory"]


def _rng_sample_seed() -> int:
    # torch's CPU generator, like p_model._rng_dropout_seed: two samples after the same
    # torch.manual_seed pick the same indices
    return int(torch.randint(0, 2**62, (1,)).item())


class Memory(object):
    def __init__(self, memory_size, transition_lens, device):
        memory_size, transition_lens = int(memory_size), int(transition_lens)
        if memory_size < 1 or transition_lens < 1:
            raise ValueError("Memory: memory_size and transition_lens must be positive")
        self.device = device
        self.transition_lens = transition_lens
        self.epsilon = 1e-3
        self.alpha = 0.6
        self.beta = 0.4
        self.beta_increment_per_sampling = 1e-5
        self.abs_err_upper = 1

        self.memory_size = memory_size
        self.memory_counter = 0

        self.prioritys_ = torch.zeros(size=[memory_size, 1], dtype=torch.float32, device=device)
        self.memory = torch.zeros(size=[memory_size, transition_lens], dtype=torch.float32,
                                  device=device)

    def get_priority(self, td_error):
        return torch.pow(torch.abs(td_error) + self.epsilon, self.alpha)

    # ------------------------------------------------------------------ host checks ---
    def _check_td(self, td, n, who):
        if not isinstance(td, torch.Tensor) or td.dtype != torch.float32 or \
                tuple(td.shape) not in ((n, 1), (n,)):
            raise ValueError(f"{who}: td errors must be float32 [{n}, 1]")
        return td.contiguous()

    def _check_k(self, k, who):
        k = int(k)
        filled = min(self.memory_counter, self.memory_size)
        if k < 1 or k > filled:
            raise ValueError(f"{who}: batch_size {k} outside [1, {filled}] (the filled slots)")
        if k > hip_ops.PER_MAX_K:
            raise ValueError(f"{who}: batch_size {k} > {hip_ops.PER_MAX_K}")
        return k, filled

    # ------------------------------------------------------------------------ ops -----
    def add(self, td_error, transitions):
        if not isinstance(transitions, torch.Tensor) or transitions.dim() != 2 or \
                transitions.shape[1] != self.transition_lens or transitions.dtype != torch.float32:
            raise ValueError(f"add: transitions must be float32 [n, {self.transition_lens}]")
        n = transitions.shape[0]
        if n > self.memory_size:
            raise ValueError(f"add: {n} transitions do not fit a memory of {self.memory_size}")
        td = self._check_td(td_error, n, "add")
        if n and transitions.stride(1) != 1:
            transitions = transitions.contiguous()
        hip_ops.per_add(self.memory, self.prioritys_, self.memory_counter % self.memory_size,
                        transitions, td, self.epsilon, self.alpha)
        self.memory_counter += n

    def add_step(self, features, c_actions, d_values, d_actions, rewards):
        """add(ones, cat([features.float(), c_actions, d_values, d_actions.float(), rewards], 1))
        — the driver's store of one batch — as one launch, bitwise the same memory and
        priorities. features [n, F] and d_actions [n, 1] are int32 / int64; c_actions, d_values
        [n, A] and rewards [n, 1] may be row-strided views."""
        n = features.shape[0] if isinstance(features, torch.Tensor) and features.dim() == 2 else -1
        if n < 0:
            raise ValueError("add_step: features must be an integer [n, F] tensor")
        if n > self.memory_size:
            raise ValueError(f"add_step: {n} transitions do not fit a memory of {self.memory_size}")
        hip_ops.per_store_step(self.memory, self.prioritys_,
                               self.memory_counter % self.memory_size, features, c_actions,
                               d_values, d_actions, rewards, self.epsilon, self.alpha)
        self.memory_counter += n

    def _sample(self, batch_size, mode, seed, who):
        k, filled = self._check_k(batch_size, who)
        if mode == hip_ops.PER_STOCHASTIC and seed is None:
            seed = _rng_sample_seed()
        # the reference rounds beta through a FloatTensor (lines 78, 93)
        beta = float(np.float32(min(1.0, self.beta + self.beta_increment_per_sampling)))
        out = hip_ops.per_sample(self.memory, self.prioritys_, filled, k, mode,
                                 int(seed or 0) & (2**64 - 1), beta)
        self.beta = beta
        return out["idx"], out["batch"], out["isw"]

    def stochastic_sample(self, batch_size, seed=None):
        return self._sample(batch_size, hip_ops.PER_STOCHASTIC, seed, "stochastic_sample")

    def greedy_sample(self, batch_size):
        return self._sample(batch_size, hip_ops.PER_GREEDY, None, "greedy_sample")

    def batch_update(self, choose_idx, td_errors):
        if not isinstance(choose_idx, torch.Tensor) or choose_idx.dtype != torch.int64:
            raise ValueError("batch_update: choose_idx must be an int64 tensor")
        idx = choose_idx.reshape(-1).contiguous()
        td = self._check_td(td_errors, idx.numel(), "batch_update")
        hip_ops.per_update(self.prioritys_, idx, td, self.epsilon, self.alpha)
