"""CPU checks of the hybrid TD3 ensemble driver's parts: LR's construction, its place in the
pretraining drivers, the host validation of the three new entry points (no kernel is launched)
and the numpy restatement of the base driver's generate_preds against the reference's record."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import rl_driver_ref as R
from conftest import load_golden


@pytest.fixture(scope="module")
def built_lib():
    from rl_ctr_prediction_amd.build_lib import LIB, build
    try:
        build()
    except RuntimeError as e:  # no hipcc in this environment
        pytest.skip(str(e))
    return LIB


def test_lr_seeded_construction_is_bitwise():
    from rl_ctr_prediction_amd import LR
    g = load_golden("g_lr.npz")
    torch.manual_seed(0)
    m = LR(1508)
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]], "keys / order differ from the reference"
    assert set(sd) == {"linear.weight", "bias"}
    for k, v in sd.items():
        want = g[f"seeded_init/{k}"]
        a = v.detach().numpy()
        assert a.shape == want.shape and a.dtype == want.dtype and a.tobytes() == want.tobytes(), k
    m.load_state_dict({k: torch.from_numpy(np.array(g[f"init/{k}"])) for k in sd}, strict=True)
    with pytest.raises(NotImplementedError, match="output_dim"):
        LR(10, output_dim=2)


def test_get_model_builds_lr_for_the_autograd_trainer():
    from rl_ctr_prediction_amd import LR
    from rl_ctr_prediction_amd import pretrain_main as PM
    from rl_ctr_prediction_amd.main import pretrain_main as PM_days
    from rl_ctr_prediction_amd import pretrain_main_2 as PM2
    m = PM.get_model("LR", 50, 4, 8)
    assert isinstance(m, LR) and m.linear.weight.shape == (50, 1)
    tr = PM.make_trainer("LR", m, 1e-3, 1e-5)
    assert isinstance(tr, PM.AutogradTrainer)
    assert PM_days.get_model is PM.get_model and PM_days.make_trainer is PM.make_trainer
    assert PM2.get_model is PM.get_model
    with pytest.raises(NotImplementedError, match="only LR is built"):
        PM.get_model("W&D", 10, 2, 4)


def test_host_validation_of_the_new_entry_points(built_lib):
    """Argument checks run before any HIP call: fake pointers are never dereferenced."""
    from rl_ctr_prediction_amd._lib import CtrHipError, lib
    P = 4096  # a fake, non-null pointer
    # ctr_lr_forward(idx, idx_type, B, F, V, lin, bias, z, p, labels, mean_div, loss, gz, err, s)
    with pytest.raises(CtrHipError, match="null"):
        lib.ctr_lr_forward(None, 1, 4, 8, 100, P, P, P, P, None, 1.0, None, None, None, None)
    with pytest.raises(CtrHipError, match="null"):
        lib.ctr_lr_forward(P, 1, 4, 8, 100, None, P, P, P, None, 1.0, None, None, None, None)
    with pytest.raises(CtrHipError, match="bad sizes"):
        lib.ctr_lr_forward(P, 1, 4, 65, 100, P, P, P, P, None, 1.0, None, None, None, None)
    with pytest.raises(CtrHipError, match="bad sizes"):
        lib.ctr_lr_forward(P, 1, 4, 0, 100, P, P, P, P, None, 1.0, None, None, None, None)
    with pytest.raises(CtrHipError, match="bad sizes"):
        lib.ctr_lr_forward(P, 1, 4, 8, 2 ** 31, P, P, P, P, None, 1.0, None, None, None, None)
    with pytest.raises(CtrHipError, match="idx_type"):
        lib.ctr_lr_forward(P, 7, 4, 8, 100, P, P, P, P, None, 1.0, None, None, None, None)
    with pytest.raises(CtrHipError, match="mean_div"):
        lib.ctr_lr_forward(P, 1, 4, 8, 100, P, P, P, P, P, 0.0, P, P, None, None)
    assert lib.ctr_lr_forward(P, 1, 0, 8, 100, P, P, None, None, None, 1.0, None, None, None,
                              None) == 0  # B == 0: nothing to do

    # ctr_ensemble_preds_ex(preds, B, M, ld, actions, at, pw, ca, labels, lt, y, r, rc, rank,
    #                       flags, stream)
    def ens(M=3, ld=3, preds=P, pw=P, rc=None, rank=None, flags=1, B=4, at=1):
        return lib.ctr_ensemble_preds_ex(preds, B, M, ld, P, at, pw, None, P, 1, P, P, rc, rank,
                                         flags, None)
    with pytest.raises(CtrHipError, match="M <= 32"):
        ens(M=33, ld=33)
    with pytest.raises(CtrHipError, match="ld_preds"):
        ens(M=3, ld=2)
    with pytest.raises(CtrHipError, match="null"):
        ens(preds=None)
    with pytest.raises(CtrHipError, match="null"):
        ens(pw=None)
    with pytest.raises(CtrHipError, match="null"):
        ens(rc=P, rank=None)  # the returned c_actions need the rank scratch
    with pytest.raises(CtrHipError, match="flags"):
        ens(flags=2)
    with pytest.raises(CtrHipError, match="action_type"):
        ens(at=5)
    assert ens(B=0) == 0
    # the old entry point still needs its c_actions and return_c_actions
    with pytest.raises(CtrHipError, match="null"):
        lib.ctr_ensemble_preds(P, 4, 3, 3, P, 1, P, None, P, 1, P, P, P, P, None)
    with pytest.raises(CtrHipError, match="M <= 32"):
        lib.ctr_ensemble_preds(None, 4, 33, 33, None, 1, None, None, None, 1, None, None, None,
                               None, None)

    # ctr_per_store_step(N, T, start, n, F, A, idx, it, c, ldc, d, ldd, act, at, r, ldr, eps,
    #                    alpha, memory, prio, stream)
    def store(N=64, T=14, start=0, n=8, F=6, A=3, idx=P, c=P, ldc=3, d=P, ldd=3, act=P, r=P,
              ldr=1, memory=P, prio=P, it=1, at=1):
        return lib.ctr_per_store_step(N, T, start, n, F, A, idx, it, c, ldc, d, ldd, act, at, r,
                                      ldr, 1e-3, 0.6, memory, prio, None)
    with pytest.raises(CtrHipError, match=r"F \+ 2A \+ 2"):
        store(T=15)
    with pytest.raises(CtrHipError, match=r"F \+ 2A \+ 2"):
        store(F=0, T=8)
    with pytest.raises(CtrHipError, match="n=65"):
        store(n=65)
    with pytest.raises(CtrHipError, match="start"):
        store(start=64)
    with pytest.raises(CtrHipError, match="null memory"):
        store(memory=None)
    with pytest.raises(CtrHipError, match="null idx"):
        store(idx=None)
    with pytest.raises(CtrHipError, match="null idx"):
        store(r=None)
    with pytest.raises(CtrHipError, match="row strides"):
        store(ldc=2)
    with pytest.raises(CtrHipError, match="row strides"):
        store(ldr=0)
    with pytest.raises(CtrHipError, match="idx_type"):
        store(it=3)
    with pytest.raises(CtrHipError, match="N="):
        store(N=0)
    assert store(n=0, idx=None, c=None, d=None, act=None, r=None) == 0  # a no-op


def test_cpu_tensors_are_refused(built_lib):
    from rl_ctr_prediction_amd import LR, PrioritizedMemory, hip_ops
    x = torch.zeros(4, 6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.lr_forward(x, torch.zeros(10, 1), torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LR(10)(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.ensemble_preds_ex(torch.zeros(4, 3), torch.ones(4, 1, dtype=torch.int64),
                                  torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64))
    mem = PrioritizedMemory(64, 14, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mem.add_step(x, torch.zeros(4, 3), torch.zeros(4, 3), torch.ones(4, 1, dtype=torch.int64),
                     torch.zeros(4, 1))
    assert mem.memory_counter == 0


@pytest.mark.parametrize("case", range(3))
def test_numpy_generate_preds_reproduces_the_reference(case):
    """rl_driver_ref.generate_preds_base against the reference's own outputs: the rewards
    exactly, the built ties included; y exactly for a == 1 and to 1e-6 relative elsewhere (the
    bar of the v10 oracle's test: torch's exp and the order of its short sums)."""
    g = load_golden("g_ensemble_base.npz")
    k = lambda n: g[f"c{case}_{n}"]  # noqa: E731
    y, r = R.generate_preds_base(k("preds"), k("actions"), k("pw"), k("labels"))
    want_y, want_r = k("y").ravel(), k("r").ravel()
    np.testing.assert_array_equal(r, want_r)
    M = k("preds").shape[1]
    a = k("actions").ravel()
    if M > 1:  # a == 1: the one model's prediction itself (a one-element softmax is exactly 1)
        np.testing.assert_array_equal(y[a == 1], want_y[a == 1])
    np.testing.assert_allclose(y, want_y, rtol=1e-6, atol=0)
    ties = int(k("ties"))
    assert ties >= min(4 * M, len(a)) and set(a.tolist()) == set(range(1, M + 1))
    mean = k("preds").astype(np.float32).mean(1)
    tied = np.flatnonzero(want_y == mean)
    assert len(tied) >= (len(a) if M == 1 else 1), "the record holds no exact tie"
    lab = k("labels").ravel()
    assert (want_r[tied][np.isin(lab[tied], (0, 1))] == 1).all()  # a tie earns 1
