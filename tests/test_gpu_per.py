"""GPU tests of the prioritized replay memory (csrc/per.hip, replay_memory.Memory): parity
with the reference's recorded script (tests/golden/g_per.npz), exact selection against
numpy's stable sort of the kernel's own keys, determinism, the sampling distribution, add /
update edge cases and the absence of host synchronisation."""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

RTOL = 1e-5  # the project's prediction bar


def _mem(dev, N, T):
    from rl_ctr_prediction_amd.replay_memory import Memory
    return Memory(N, T, dev)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ reference parity ----
def _check_state(m, g, tag, i):
    assert m.memory.cpu().numpy().tobytes() == g[f"{tag}/{i}/memory"].tobytes(), (tag, i)
    np.testing.assert_allclose(m.prioritys_.cpu().numpy(), g[f"{tag}/{i}/prio"], rtol=RTOL,
                               atol=0, err_msg=f"{tag}/{i} prioritys_")
    assert m.memory_counter == int(g[f"{tag}/{i}/counter"]), (tag, i)
    assert np.float32(m.beta) == np.float32(g[f"{tag}/{i}/beta"]), (tag, i)
    assert m.beta == float(g[f"{tag}/{i}/beta"]), (tag, i)


@pytest.mark.parametrize("tag,N", [("a", 1000), ("b", 450)])
def test_recorded_script_matches_the_reference(cuda, tag, N):
    g = load_golden("g_per.npz")
    m = _mem(cuda, N, 7)
    assert m.prioritys_.shape == (N, 1) and m.memory.shape == (N, 7)
    assert m.prioritys_.device.type == "cuda" and m.memory.device.type == "cuda"
    ops = [str(o) for o in g[f"{tag}/ops"]]
    assert ops.count("add") >= 2 and (tag == "b" or ops.count("greedy") == 2)
    for i, op in enumerate(ops):
        if op == "add":
            m.add(_t(g[f"{tag}/{i}/td"], cuda), _t(g[f"{tag}/{i}/trans"], cuda))
        elif op == "update":
            m.batch_update(_t(g[f"{tag}/{i}/idx"], cuda), _t(g[f"{tag}/{i}/td"], cuda))
        else:
            idx, batch, isw = m.greedy_sample(int(g[f"{tag}/{i}/k"]))
            assert idx.dtype == torch.int64 and isw.shape == (len(idx), 1)
            np.testing.assert_array_equal(idx.cpu().numpy(), g[f"{tag}/{i}/idx"])
            assert batch.cpu().numpy().tobytes() == g[f"{tag}/{i}/batch"].tobytes()
            np.testing.assert_allclose(isw.cpu().numpy(), g[f"{tag}/{i}/isw"], rtol=RTOL, atol=0)
        _check_state(m, g, tag, i)


# ------------------------------------------------------------------ exact selection -----
def _select_and_check(dev, memory, prio, n_valid, k, mode, seed, beta=0.4):
    from rl_ctr_prediction_amd import hip_ops
    keys = hip_ops.per_keys(prio, n_valid, mode, seed).cpu().numpy()
    out = hip_ops.per_sample(memory, prio, n_valid, k, mode, seed, beta)
    idx = out["idx"].cpu().numpy()
    # descending key, ties in ascending index: numpy's stable sort of the negated keys
    want = np.argsort(-keys, kind="stable")[:k]
    np.testing.assert_array_equal(idx, want)
    assert len(np.unique(idx)) == k and idx.min() >= 0 and idx.max() < n_valid
    assert torch.equal(out["batch"], memory[out["idx"]])
    p = prio.cpu().numpy().reshape(-1).astype(np.float64)
    min_p = p[:n_valid].min()
    assert float(out["min_p"].item()) == min_p
    isw = (p[idx] / min_p) ** (-float(np.float32(beta)))
    np.testing.assert_allclose(out["isw"].cpu().numpy().reshape(-1), isw, rtol=RTOL, atol=0)
    return idx


SHAPES = [(1, 1, 1), (5, 3, 5), (1000, 7, 64), (70001, 27, 257), ((1 << 20) + 3, 32, 4096),
          (300000, 5, 8192)]


@pytest.mark.parametrize("mode", [0, 1], ids=["stochastic", "greedy"])
@pytest.mark.parametrize("N,T,k", SHAPES)
def test_selection_is_exact(cuda, N, T, k, mode):
    rng = np.random.default_rng(N)
    memory = torch.randn(N, T, device=cuda)
    rep = rng.random(N) < 0.5
    # N = 70001: a priority column that is not 16-byte aligned (the scalar loads)
    buf = torch.empty(N + 1, device=cuda)
    for R in (0.8, 2.0):  # the repeated value inside the range, and above it (ties at the cut)
        p = (rng.random(N, dtype=np.float32) * np.float32(0.9) + np.float32(0.1))
        p[rep] = R
        prio = buf[1:] if N == 70001 else buf[:N]
        prio.copy_(_t(p, cuda))
        _select_and_check(cuda, memory, prio, N, k, mode, seed=12345 + N)
        # a partly filled memory: the slots at and above n_valid hold the largest priorities
        n_valid = max(k, N - N // 3)
        if n_valid < N:
            prio[n_valid:] = 100.0
            idx = _select_and_check(cuda, memory, prio, n_valid, k, mode, seed=7)
            assert idx.max() < n_valid


@pytest.mark.parametrize("N,k", [(5000, 300), (300000, 8192)])
def test_equal_priorities_come_back_in_slot_order(cuda, N, k):
    from rl_ctr_prediction_amd import hip_ops
    memory = torch.randn(N, 4, device=cuda)
    prio = torch.full((N, 1), 1.0, device=cuda)
    out = hip_ops.per_sample(memory, prio, N, k, hip_ops.PER_GREEDY, 0, 0.4)
    assert torch.equal(out["idx"], torch.arange(k, device=cuda))
    assert torch.equal(out["batch"], memory[:k])
    assert torch.equal(out["isw"], torch.ones(k, 1, device=cuda))


# --------------------------------------------------------------------- determinism ------
def _filled(dev, N, T, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    m = _mem(dev, N, T)
    m.add(torch.randn(n, 1, generator=g).to(dev), torch.randn(n, T, generator=g).to(dev))
    return m


def test_same_seed_same_bits(cuda):
    m = _filled(cuda, 70001, 27, 60000)
    a = m.stochastic_sample(257, seed=5)
    beta = m.beta
    m.beta = 0.4
    b = m.stochastic_sample(257, seed=5)
    assert m.beta == beta
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    c = m.stochastic_sample(257, seed=6)
    assert not torch.equal(a[0], c[0])
    assert len(torch.unique(c[0])) == 257 and int(c[0].max()) < 60000


def test_torch_manual_seed_controls_the_default_seed(cuda):
    m = _filled(cuda, 5000, 5, 3000)
    torch.manual_seed(3)
    a = m.stochastic_sample(64)[0]
    b = m.stochastic_sample(64)[0]
    torch.manual_seed(3)
    c = m.stochastic_sample(64)[0]
    assert torch.equal(a, c) and not torch.equal(a, b)


# -------------------------------------------------------------------- distribution ------
def test_stochastic_sample_draws_the_sequential_distribution(cuda):
    """N = 6, k = 3, 4000 draws. Every element's inclusion frequency, and its frequency of
    being drawn first, lies within the binomial 5 sigma band 5 * sqrt(q (1 - q) / 4000) of the
    exact probability of sequential weighted sampling without replacement (the 120 ordered
    triples enumerated below)."""
    from rl_ctr_prediction_amd import hip_ops
    draws, N, k = 4000, 6, 3
    m = _mem(cuda, N, 1)
    td = torch.tensor([[2.0], [0.5], [0.1], [0.1], [0.02], [0.0]], device=cuda)
    m.add(td, torch.arange(N, dtype=torch.float32, device=cuda).reshape(N, 1))
    p = m.prioritys_.cpu().numpy().reshape(-1).astype(np.float64)
    np.testing.assert_allclose(p, (np.abs(td.cpu().numpy().reshape(-1)) + 1e-3) ** 0.6, rtol=RTOL)
    S = p.sum()
    incl, first = np.zeros(N), p / S
    for i, j, l in itertools.permutations(range(N), 3):
        pr = p[i] / S * p[j] / (S - p[i]) * p[l] / (S - p[i] - p[j])
        for e in (i, j, l):
            incl[e] += pr
    assert abs(incl.sum() - k) < 1e-9
    got = [hip_ops.per_sample(m.memory, m.prioritys_, N, k, hip_ops.PER_STOCHASTIC, s, 0.4)["idx"]
           for s in range(draws)]
    idx = torch.stack(got).cpu().numpy()
    assert (np.sort(idx, axis=1)[:, 1:] != np.sort(idx, axis=1)[:, :-1]).all()
    f_incl = np.array([(idx == e).any(axis=1).mean() for e in range(N)])
    f_first = np.array([(idx[:, 0] == e).mean() for e in range(N)])
    print("inclusion", f_incl, "exact", incl)
    print("first", f_first, "exact", first)
    for f, q, name in ((f_incl, incl, "inclusion"), (f_first, first, "first")):
        band = 5.0 * np.sqrt(q * (1.0 - q) / draws)
        assert (np.abs(f - q) <= band).all(), (name, f, q, band)


def test_stochastic_keys_are_finite_for_positive_priorities(cuda):
    from rl_ctr_prediction_amd import hip_ops
    N = (1 << 20) + 3
    rng = np.random.default_rng(1)
    p = np.exp(rng.uniform(np.log(1e-37), np.log(1e38), N)).astype(np.float32)
    p[::1001] = 0.0
    p[5::1001] = -1.0
    p[7::1001] = np.inf
    p[9::1001] = np.nan
    prio = _t(p, cuda)
    keys = hip_ops.per_keys(prio, N, hip_ops.PER_STOCHASTIC, 99)
    ok = torch.isfinite(prio) & (prio > 0)
    assert int(ok.sum()) > N // 2
    assert bool(torch.isfinite(keys[ok]).all())
    assert bool((keys[~ok] == float("-inf")).all())
    gk = hip_ops.per_keys(prio, N, hip_ops.PER_GREEDY, 0)
    assert torch.equal(gk[ok], prio[ok]) and bool((gk[~ok] == float("-inf")).all())


# ------------------------------------------------------------------ add and update ------
def _prio_of(td):
    return (np.abs(np.asarray(td, dtype=np.float64)) + 1e-3) ** 0.6


@pytest.mark.parametrize("T", [7, 8])
def test_add_wraps_and_keeps_the_larger_priority(cuda, T):
    N = 10
    g = torch.Generator().manual_seed(T)
    m = _mem(cuda, N, T)
    m.add(torch.zeros(0, 1, device=cuda), torch.zeros(0, T, device=cuda))  # n = 0
    assert m.memory_counter == 0 and not m.memory.any() and not m.prioritys_.any()
    tr0, td0 = torch.randn(N, T, generator=g), torch.rand(N, 1, generator=g) + 1.0
    m.add(td0.to(cuda), tr0.to(cuda))  # n = N: ends exactly at N
    assert m.memory_counter == N and torch.equal(m.memory.cpu(), tr0)
    np.testing.assert_allclose(m.prioritys_.cpu().numpy(), _prio_of(td0), rtol=RTOL)
    tr1 = torch.randn(7, T, generator=g)
    m.add(torch.full((7, 1), 3.0, device=cuda), tr1.to(cuda))  # slots 0..6
    tr2, td2 = torch.randn(6, T, generator=g), torch.full((6, 1), 0.01)
    td2[4] = 5.0
    m.add(td2.to(cuda), tr2.to(cuda))  # a wrap: slots 7, 8, 9, 0, 1, 2
    assert m.memory_counter == N + 13
    want = tr0.clone()
    want[:7] = tr1
    want[7:] = tr2[:3]
    want[:3] = tr2[3:]
    assert torch.equal(m.memory.cpu(), want)  # rows are overwritten ...
    p = _prio_of(td0).reshape(-1)
    p[:7] = _prio_of(3.0)
    p[1] = _prio_of(5.0)  # ... priorities only grow: the smaller td changed none of them
    np.testing.assert_allclose(m.prioritys_.cpu().numpy().reshape(-1), p, rtol=RTOL)
    m.add(torch.full((10, 1), 0.5, device=cuda)[:7], tr1.to(cuda))  # ends exactly at N again
    assert m.memory_counter == 2 * N + 10 and torch.equal(m.memory.cpu()[3:], tr1)


@pytest.mark.parametrize("T", [5, 8])
def test_add_reads_strided_rows_only(cuda, T):
    m = _mem(cuda, 9, T)
    wide = torch.full((4, T + 4), -7.0, device=cuda)
    rows = torch.randn(4, T, device=cuda)
    wide[:, :T] = rows
    m.memory_counter = 7
    m.add(torch.ones(4, 1, device=cuda), wide[:, :T])  # ldt = T + 4
    assert torch.equal(m.memory[7:], rows[:2]) and torch.equal(m.memory[:2], rows[2:])
    assert not m.memory[2:7].any() and not m.prioritys_[2:7].any()
    assert bool((wide[:, T:] == -7.0).all())


def test_batch_update_writes_only_the_named_rows(cuda):
    m = _filled(cuda, 1000, 3, 1000)
    before = m.prioritys_.clone()
    idx = torch.tensor([999, 0, 17, 500], device=cuda)
    td = torch.tensor([[0.0], [-2.0], [0.25], [9.0]], device=cuda)
    m.batch_update(idx, td)
    after = m.prioritys_.cpu().numpy().reshape(-1)
    np.testing.assert_allclose(after[idx.cpu().numpy()], _prio_of(td.cpu().numpy()).reshape(-1),
                               rtol=RTOL)
    keep = np.ones(1000, dtype=bool)
    keep[idx.cpu().numpy()] = False
    assert np.array_equal(after[keep], before.cpu().numpy().reshape(-1)[keep])


# --------------------------------------------------------------------- no host sync -----
def test_no_host_synchronisation(cuda):
    m = _filled(cuda, 20000, 8, 15000)
    td, tr = torch.rand(256, 1, device=cuda), torch.randn(256, 8, device=cuda)

    def loop():
        m.add(td, tr)
        idx, _, _ = m.stochastic_sample(128)
        m.batch_update(idx, td[:128])
        idx, _, isw = m.greedy_sample(128)
        m.batch_update(idx, isw)

    loop()  # warm-up: code objects, the scratch buffer, the allocator's blocks
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loop()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert m.memory_counter == 15000 + 512
