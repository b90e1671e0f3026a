"""Capture the prioritized-replay golden record from the reference's Memory (survey container
only), like make_golden_dcn.py.

Imports jqsl2012/RL_CTR_Prediction from /root/reference (read-only, never copied) and runs
src/models/Hybrid_TD3_model_PER.Memory on CPU. The fixture is data: every input, the state
after every operation and the greedy samples.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_per.py

  g_per.npz
    attrs/*                      the constructor's attributes (Memory(1000, 7, 'cpu'))
    a/ops, b/ops                 the operation names of the two scripts, in order
    {a,b}/{i}/td, trans          inputs of add i;  {i}/idx, td of batch_update i;  {i}/k of greedy i
    {a,b}/{i}/memory, prio, counter, beta     the state after operation i
    {a,b}/{i}/idx, batch, isw    what greedy_sample i returned
  script a, Memory(1000, 7): add 300 x4 (the fourth wraps: slots 900..999, 0..199),
    greedy_sample(64), batch_update of those 64, add 300, greedy_sample(64)
  script b, Memory(450, 7): add 150, add 300 (ends exactly at N: the reference's wrap branch)

|td| comes from a shuffled grid, never twice the same value: torch.sort breaks ties
arbitrarily and powf on the device differs from torch's CPU pow in the last bits, so at every
greedy call any two of the top 65 priorities must differ by >= 1e-4 relative (ten times the
1e-5 comparison bar); the generator asserts it (a seeded randn stream gives gaps of 8e-6).
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path(os.environ.get("CTR_REFERENCE", "/root/reference"))
T = 7
TOP, MIN_GAP = 65, 1e-4


def _import_reference():
    if not REF.exists():
        raise SystemExit(f"{REF} not found: goldens are generated in the survey container only")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    import src.models.Hybrid_TD3_model_PER as M  # noqa: E402
    return M


def _np(t):
    return t.detach().cpu().numpy().copy()


class Recorder:
    def __init__(self, mem, tag, out, grid, g):
        self.mem, self.tag, self.out, self.grid, self.g = mem, tag, out, grid, g
        self.ops = []
        self.used = 0

    def _td(self, n):
        """n unused grid magnitudes with random signs, [n, 1] fp32."""
        mag = self.grid[self.used:self.used + n]
        assert len(mag) == n, "grid exhausted"
        self.used += n
        sign = torch.randint(0, 2, (n,), generator=self.g).float() * 2 - 1
        return (torch.from_numpy(mag) * sign).reshape(n, 1)

    def _state(self, i):
        o, m = self.out, self.mem
        o[f"{self.tag}/{i}/memory"] = _np(m.memory)
        o[f"{self.tag}/{i}/prio"] = _np(m.prioritys_)
        o[f"{self.tag}/{i}/counter"] = np.int64(m.memory_counter)
        o[f"{self.tag}/{i}/beta"] = np.float64(m.beta)

    def add(self, n):
        i = len(self.ops)
        td, tr = self._td(n), torch.randn(n, T, generator=self.g)
        self.out[f"{self.tag}/{i}/td"], self.out[f"{self.tag}/{i}/trans"] = _np(td), _np(tr)
        self.mem.add(td, tr)
        self.ops.append("add")
        self._state(i)

    def greedy(self, k):
        i = len(self.ops)
        p = np.sort(_np(self.mem.prioritys_).reshape(-1).astype(np.float64))[::-1][:TOP]
        gap = np.min((p[:-1] - p[1:]) / p[:-1])
        assert k < TOP and gap >= MIN_GAP, f"greedy {i}: top-{TOP} priority gap {gap:.3g}"
        idx, batch, isw = self.mem.greedy_sample(k)
        o = self.out
        o[f"{self.tag}/{i}/k"] = np.int64(k)
        o[f"{self.tag}/{i}/idx"], o[f"{self.tag}/{i}/batch"] = _np(idx), _np(batch)
        o[f"{self.tag}/{i}/isw"] = _np(isw)
        self.ops.append("greedy")
        self._state(i)
        print(f"{self.tag}/{i} greedy: min relative gap among the top {TOP} = {gap:.3g}")
        return idx

    def update(self, idx):
        i = len(self.ops)
        td = self._td(len(idx))
        self.out[f"{self.tag}/{i}/idx"], self.out[f"{self.tag}/{i}/td"] = _np(idx), _np(td)
        self.mem.batch_update(idx, td)
        self.ops.append("update")
        self._state(i)

    def finish(self):
        self.out[f"{self.tag}/ops"] = np.array(self.ops)


def main():
    M = _import_reference()
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(11)
    # 2600 distinct |td| in [0.1, 3]: neighbours differ by 1.1e-3, >= 3.7e-4 relative, which
    # the 0.6 power turns into >= 2.2e-4 relative between any two priorities
    grid = np.linspace(0.1, 3.0, 2600).astype(np.float32)
    grid = grid[torch.randperm(len(grid), generator=g).numpy()]
    out = {}
    mem = M.Memory(1000, T, "cpu")
    for name in ("epsilon", "alpha", "beta", "beta_increment_per_sampling", "abs_err_upper",
                 "memory_size", "memory_counter", "transition_lens"):
        out[f"attrs/{name}"] = np.float64(getattr(mem, name))
    out["attrs/prio_shape"] = np.array(mem.prioritys_.shape)
    out["attrs/memory_shape"] = np.array(mem.memory.shape)
    a = Recorder(mem, "a", out, grid, g)
    for _ in range(4):
        a.add(300)
    idx = a.greedy(64)
    a.update(idx)
    a.add(300)
    a.greedy(64)
    a.finish()
    b = Recorder(M.Memory(450, T, "cpu"), "b", out, grid[a.used:], g)
    b.add(150)
    b.add(300)
    b.finish()
    assert b.mem.memory_counter == 450
    np.savez_compressed(HERE / "g_per.npz", **out)
    print(f"wrote g_per.npz ({(HERE / 'g_per.npz').stat().st_size} bytes)")


if __name__ == "__main__":
    main()
