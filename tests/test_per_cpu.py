"""CPU checks of the prioritized replay memory: constructor parity with the reference's
recorded attributes (tests/golden/g_per.npz, make_golden_per.py), the host-side validation of
the ctr_per_* entry points and of the Memory class. No kernel is launched here."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from conftest import load_golden


@pytest.fixture(scope="module")
def built_lib():
    from rl_ctr_prediction_amd.build_lib import LIB, build
    try:
        build()
    except RuntimeError as e:  # no hipcc in this environment
        pytest.skip(str(e))
    return LIB


def test_constructor_attributes_match_the_reference():
    import rl_ctr_prediction_amd as pkg
    from rl_ctr_prediction_amd.replay_memory import Memory
    assert pkg.PrioritizedMemory is Memory
    g = load_golden("g_per.npz")
    m = Memory(1000, 7, "cpu")
    for name in ("epsilon", "alpha", "beta", "beta_increment_per_sampling", "abs_err_upper",
                 "memory_size", "memory_counter", "transition_lens"):
        assert float(getattr(m, name)) == float(g[f"attrs/{name}"]), name
    assert m.device == "cpu"
    for t, key in ((m.prioritys_, "attrs/prio_shape"), (m.memory, "attrs/memory_shape")):
        assert tuple(t.shape) == tuple(g[key]) and t.dtype == torch.float32
        assert not t.any()
    td = torch.tensor([[-2.0], [0.0], [0.5]])
    want = (np.abs(td.numpy()) + np.float32(1e-3)) ** np.float32(0.6)
    np.testing.assert_allclose(m.get_priority(td).numpy(), want, rtol=1e-6)


FAKE = 1 << 20  # a non-null, 16-byte aligned address; never dereferenced: validation comes first


def _sample(lib, N=100, T=4, n_valid=50, k=8, mode=0, memory=FAKE, prio=FAKE, idx=FAKE,
            batch=FAKE, isw=FAKE, ws=FAKE, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.ctr_per_workspace_bytes(100, 8)
    return lib.ctr_per_sample(N, T, n_valid, k, mode, 1, 0.4, memory, prio, idx, batch, isw,
                              None, ws, ws_bytes, None)


def test_host_validation_errors_without_gpu(built_lib):
    """Argument checks run before any HIP call: bad input raises, never launches."""
    from rl_ctr_prediction_amd._lib import CtrHipError, lib
    need = lib.ctr_per_workspace_bytes(100, 8)
    assert need > 0
    # a function of (N, k) alone, and nothing for an N or k out of range
    assert lib.ctr_per_workspace_bytes(4096000, 8192) > 0
    assert lib.ctr_per_workspace_bytes(0, 8) == 0
    assert lib.ctr_per_workspace_bytes(100, 0) == 0
    assert lib.ctr_per_workspace_bytes(100000, 8193) == 0

    with pytest.raises(CtrHipError, match="null memory"):
        _sample(lib, prio=None)
    with pytest.raises(CtrHipError, match="null memory"):
        _sample(lib, idx=None)
    with pytest.raises(CtrHipError, match="N=0"):
        _sample(lib, N=0, n_valid=0)
    with pytest.raises(CtrHipError, match="T=0"):
        _sample(lib, T=0)
    with pytest.raises(CtrHipError, match="k=0"):
        _sample(lib, k=0)
    with pytest.raises(CtrHipError, match="k=51"):
        _sample(lib, k=51)  # > n_valid
    with pytest.raises(CtrHipError, match="k=8193"):
        _sample(lib, N=10000, n_valid=10000, k=8193)
    with pytest.raises(CtrHipError, match="n_valid=101"):
        _sample(lib, n_valid=101)
    with pytest.raises(CtrHipError, match="mode 2"):
        _sample(lib, mode=2)
    with pytest.raises(CtrHipError, match="workspace"):
        _sample(lib, ws_bytes=need - 1)
    with pytest.raises(CtrHipError, match="workspace"):
        _sample(lib, ws=None)

    def add(N=100, T=4, start=0, n=8, tr=FAKE, ldt=4, td=FAKE, memory=FAKE, prio=FAKE):
        return lib.ctr_per_add(N, T, start, n, tr, ldt, td, 1e-3, 0.6, memory, prio, None)

    with pytest.raises(CtrHipError, match="n=101"):
        add(n=101)
    with pytest.raises(CtrHipError, match="N=-1"):
        add(N=-1)
    with pytest.raises(CtrHipError, match="T=0"):
        add(T=0)
    with pytest.raises(CtrHipError, match="start=100"):
        add(start=100)
    with pytest.raises(CtrHipError, match="null memory"):
        add(memory=None)
    with pytest.raises(CtrHipError, match="null transitions"):
        add(td=None)
    with pytest.raises(CtrHipError, match="ldt 3"):
        add(ldt=3)
    assert add(n=0, tr=None, td=None) == 0  # a no-op: nothing to read

    with pytest.raises(CtrHipError, match="N=0"):
        lib.ctr_per_update(0, 4, FAKE, FAKE, 1e-3, 0.6, FAKE, None)
    with pytest.raises(CtrHipError, match="null prio"):
        lib.ctr_per_update(100, 4, FAKE, FAKE, 1e-3, 0.6, None, None)
    with pytest.raises(CtrHipError, match="null idx"):
        lib.ctr_per_update(100, 4, None, FAKE, 1e-3, 0.6, FAKE, None)
    with pytest.raises(CtrHipError, match="negative"):
        lib.ctr_per_update(100, -1, FAKE, FAKE, 1e-3, 0.6, FAKE, None)

    with pytest.raises(CtrHipError, match="mode 7"):
        lib.ctr_per_keys(10, FAKE, 7, 0, FAKE, None)
    with pytest.raises(CtrHipError, match="null prio"):
        lib.ctr_per_keys(10, FAKE, 0, 0, None, None)
    with pytest.raises(CtrHipError, match="n_valid=-1"):
        lib.ctr_per_keys(-1, FAKE, 0, 0, FAKE, None)


def test_cpu_tensors_are_refused(built_lib):
    from rl_ctr_prediction_amd import hip_ops
    from rl_ctr_prediction_amd.replay_memory import Memory
    mem, prio = torch.zeros(10, 3), torch.ones(10, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.per_add(mem, prio, 0, torch.zeros(2, 3), torch.ones(2, 1), 1e-3, 0.6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.per_update(prio, torch.zeros(2, dtype=torch.int64), torch.ones(2, 1), 1e-3, 0.6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.per_keys(prio, 10, hip_ops.PER_GREEDY, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.per_sample(mem, prio, 10, 2, hip_ops.PER_STOCHASTIC, 0, 0.4)
    m = Memory(10, 3, "cpu")  # the class never computes on the host either
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.add(torch.ones(2, 1), torch.zeros(2, 3))
    assert m.memory_counter == 0


def test_class_value_errors_come_from_host_state():
    from rl_ctr_prediction_amd.replay_memory import Memory
    m = Memory(10000, 3, "cpu")
    with pytest.raises(ValueError, match="do not fit"):
        Memory(4, 3, "cpu").add(torch.ones(5, 1), torch.zeros(5, 3))
    with pytest.raises(ValueError, match="transitions must be float32"):
        m.add(torch.ones(2, 1), torch.zeros(2, 4))
    with pytest.raises(ValueError, match="transitions must be float32"):
        m.add(torch.ones(2, 1), torch.zeros(2, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="td errors"):
        m.add(torch.ones(3, 1), torch.zeros(2, 3))
    with pytest.raises(ValueError, match="td errors"):
        m.add(torch.ones(2, 1, dtype=torch.float64), torch.zeros(2, 3))
    for fn in (m.stochastic_sample, m.greedy_sample):
        with pytest.raises(ValueError, match="filled slots"):
            fn(1)  # empty memory
    m.memory_counter = 5
    with pytest.raises(ValueError, match="filled slots"):
        m.stochastic_sample(6)
    with pytest.raises(ValueError, match="filled slots"):
        m.greedy_sample(0)
    m.memory_counter = 25000  # wrapped: 10000 filled slots
    for fn in (m.stochastic_sample, m.greedy_sample):
        with pytest.raises(ValueError, match="> 8192"):
            fn(8193)
        with pytest.raises(ValueError, match="filled slots"):
            fn(10001)
    with pytest.raises(ValueError, match="int64"):
        m.batch_update(torch.zeros(2, dtype=torch.int32), torch.ones(2, 1))
    with pytest.raises(ValueError, match="td errors"):
        m.batch_update(torch.zeros(2, dtype=torch.int64), torch.ones(3, 1))
    assert m.beta == 0.4  # a refused sample does not advance beta
