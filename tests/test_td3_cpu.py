"""The hybrid TD3 agent without a GPU: seeded construction against the reference's record, the
plain-torch mirror (td3_ref) against the reference's eight recorded learns, host validation of
every new entry point, and the package exports."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest
import torch

import td3_ref
from conftest import GOLDEN

BIG = ["g_td3_f32_a.npz", "g_td3_f32_b.npz"]
load_td3, check_packed = td3_ref.load_golden, td3_ref.check_packed


@pytest.fixture(scope="module")
def gold():
    return load_td3(["g_td3.npz"] + BIG)


@pytest.fixture(scope="module")
def built_lib():
    from rl_ctr_prediction_amd.build_lib import LIB, _hipcc, build
    try:
        _hipcc()
    except RuntimeError as e:  # no HIP toolchain in this environment
        pytest.skip(str(e))
    build()  # a source that no longer compiles fails these tests, it does not skip them
    return LIB


def _bytes_equal(a, d, what):
    assert a.dtype == d.dtype and a.shape == d.shape, what
    assert a.tobytes() == d.tobytes(), f"{what}: bytes differ"


def test_seeded_construction_matches_the_reference(gold):
    from rl_ctr_prediction_amd.hybrid_td3_model_per import Critic, Hybrid_TD3_Model, hybrid_actors
    V, F, K, A, B, MEM, _ = (int(v) for v in gold["shapes"])
    D = F * (F - 1) // 2 + F * K
    torch.manual_seed(0)
    agent = Hybrid_TD3_Model(V, field_nums=F, latent_dims=K, action_nums=A, memory_size=MEM,
                             batch_size=B, device="cpu")
    assert agent.input_dims == D and agent.policy_freq == 4 and agent.learn_iter == 0
    assert agent.memory.transition_lens == F + 2 * A + 2
    for name, n_keys in (("Hybrid_Actor", 30), ("Critic", 51)):
        sd = getattr(agent, name).state_dict()
        assert list(sd) == list(gold[f"keys/{name}"]) and len(sd) == n_keys
        assert check_packed(gold, f"seeded_init/{name}", sd.items(), _bytes_equal, 1e-12) == n_keys
        tgt = getattr(agent, name + "_").state_dict()
        assert all(torch.equal(sd[k], tgt[k]) for k in sd) and list(tgt) == list(sd)
    for net in (agent.Hybrid_Actor_, agent.Critic_):
        assert net.training  # the targets are never put into eval mode
    # the modules alone, in the reference's RNG order (actor first, then the critic)
    torch.manual_seed(0)
    actor = hybrid_actors(D, A)
    critic = Critic(D, A, A)
    check_packed(gold, "seeded_init/Hybrid_Actor", actor.state_dict().items(), _bytes_equal, 1e-12)
    check_packed(gold, "seeded_init/Critic", critic.state_dict().items(), _bytes_equal, 1e-12)
    assert actor.std.shape == (1, A) and actor.mean.device.type == "cpu"  # no .cuda() inside
    assert isinstance(agent.optimizer_a, __import__("rl_ctr_prediction_amd").DenseAdam)
    assert isinstance(agent.memory, __import__("rl_ctr_prediction_amd").PrioritizedMemory)


def test_torch_mirror_replays_the_reference_record(gold):
    """td3_ref in fp32 on this CPU, fed the recorded samples and noise, against the reference's
    eight recorded learns: the same torch ops, possibly on another CPU.

    One thread, as the generator ran: the gradient of the critic's bn_input.bias (and of every
    Linear bias in front of a BatchNorm) is zero in exact arithmetic, so what Adam sees there is
    the GEMMs' rounding noise, which it turns into steps of up to lr whatever its size. Those
    parameters follow the record only while the sums run in the recorded order."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        _replay(gold)
    finally:
        torch.set_num_threads(threads)


# state entries moved by Adam steps on rounding-noise gradients: the biases in front of a
# BatchNorm, bn_input.bias, and the running means of the BatchNorms those biases feed
NOISE_DRIVEN = re.compile(r"/(mlp(_[12])?\.[036]\.bias|bn_input\.bias"
                          r"|mlp(_[12])?\.[147]\.running_mean)$")


def _replay(gold):
    V, F, K, A, B, MEM, CALLS = (int(v) for v in gold["shapes"])
    D = F * (F - 1) // 2 + F * K
    torch.manual_seed(0)
    ref = td3_ref.RefTD3(D, F, A, batch_size=B)
    check_packed(gold, "seeded_init/Hybrid_Actor", ref.Hybrid_Actor.state_dict().items(),
                 _bytes_equal, 1e-12)
    check_packed(gold, "seeded_init/Critic", ref.Critic.state_dict().items(), _bytes_equal, 1e-12)
    emb = torch.from_numpy(gold["emb"])

    def close(a, d, what):
        if NOISE_DRIVEN.search(what):
            what += " (follows the record only in the recorded summation order: see the docstring)"
        np.testing.assert_allclose(a, d, rtol=1e-5, atol=1e-6, err_msg=what)

    prio = np.zeros((MEM, 1), np.float32)
    prio[:] = td3_ref.priority(torch.ones(1)).item()  # 80 stores of td = 1 fill the ring
    for i in range(CALLS):
        t = f"c{i}"
        sample = tuple(torch.from_numpy(gold[f"{t}/{k}"]) for k in ("idx", "batch", "isw"))
        noise = (torch.from_numpy(gold[f"{t}/n_c"]), torch.from_numpy(gold[f"{t}/n_d"]))
        o = ref.learn(lambda ids: td3_ref.embed_state(emb, ids), sample=sample, noise=noise)
        for k in ("q1", "q2", "q1_t", "q2_t", "q_target", "td"):
            close(o[k].numpy(), gold[f"{t}/{k}"], f"{t}/{k}")
        close(float(o["loss"]), gold[f"{t}/loss"], f"{t}/loss")
        check_packed(gold, f"{t}/gc", o["gc"].items(), close)
        assert ("ga" in o) == ((i + 1) % 4 == 0)
        if "ga" in o:
            check_packed(gold, f"{t}/ga", o["ga"].items(), close)
        for n, net in ref.nets().items():
            check_packed(gold, f"{t}/{n}", net.state_dict().items(), close)
        prio[gold[f"{t}/idx"]] = td3_ref.priority(o["td"]).numpy()
        close(prio, gold[f"{t}/prio"], f"{t}/prio")
    s5 = td3_ref.embed_state(emb, torch.from_numpy(gold["states5"]))
    noise = (torch.from_numpy(gold["act/n_c"]), torch.from_numpy(gold["act/n_d"]))
    c, sm, d, ix = ref.choose_action(s5, noise)
    close(c.numpy(), gold["act/c_actions"], "act/c")
    close(sm.numpy(), gold["act/c_softmax"], "act/softmax")
    close(d.numpy(), gold["act/d_actions"], "act/d")
    assert np.array_equal(ix.numpy(), gold["act/d_index"])
    ix, sm = ref.choose_best_action(s5)
    assert np.array_equal(ix.numpy(), gold["best/d_index"])
    close(sm.numpy(), gold["best/c_softmax"], "best/softmax")


def test_fixture_files_stay_under_the_size_limit():
    files = sorted(GOLDEN.glob("g_td3*.npz"))
    assert len(files) == 7
    assert all(f.stat().st_size < (1 << 20) for f in files)


FAKE = 1 << 20  # a non-null, 16-byte aligned address; never dereferenced: validation comes first


def test_host_validation_errors_without_gpu(built_lib):
    from rl_ctr_prediction_amd._lib import CtrHipError, lib

    def bn_fwd(B=4, N=8, x=FAKE, ldx=8, gamma=FAKE, rm=FAKE, rv=FAKE, training=1, y=FAKE, ldy=8):
        lib.ctr_bn_forward(B, N, x, ldx, gamma, FAKE, rm, rv, 1e-5, 0.1, training, 0, y, ldy,
                           FAKE, FAKE, FAKE, FAKE, None)

    def bn_bwd(B=4, N=8, dy=FAKE, lddy=8, y=FAKE, relu=1, dgamma=FAKE, dx=FAKE, ldd=8):
        lib.ctr_bn_backward(B, N, dy, lddy, y, 8, relu, FAKE, 8, FAKE, FAKE, FAKE, FAKE, FAKE,
                            dgamma, FAKE, dx, ldd, None)

    with pytest.raises(CtrHipError, match="null x"):
        bn_fwd(x=None)
    with pytest.raises(CtrHipError, match="null x"):
        bn_fwd(gamma=None)
    with pytest.raises(CtrHipError, match="B >= 2"):
        bn_fwd(B=1)
    with pytest.raises(CtrHipError, match="N=0"):
        bn_fwd(N=0)
    with pytest.raises(CtrHipError, match="row stride"):
        bn_fwd(ldx=7)
    with pytest.raises(CtrHipError, match="row stride"):
        bn_fwd(ldy=7)
    with pytest.raises(CtrHipError, match="together"):
        bn_fwd(rv=None)
    with pytest.raises(CtrHipError, match="eval mode"):
        bn_fwd(training=0, rm=None, rv=None)
    with pytest.raises(CtrHipError, match="outside"):
        bn_fwd(B=1 << 31)
    with pytest.raises(CtrHipError, match="null dy"):
        bn_bwd(dy=None)
    with pytest.raises(CtrHipError, match="null dy"):
        bn_bwd(dgamma=None)
    with pytest.raises(CtrHipError, match="null y"):
        bn_bwd(y=None)
    with pytest.raises(CtrHipError, match="B >= 2"):
        bn_bwd(B=1)
    with pytest.raises(CtrHipError, match="N=-1"):
        bn_bwd(N=-1)
    with pytest.raises(CtrHipError, match="row stride"):
        bn_bwd(lddy=4)
    with pytest.raises(CtrHipError, match="row stride"):
        bn_bwd(ldd=4)

    with pytest.raises(CtrHipError, match="null out"):
        lib.ctr_td3_noise(8, 1, 0, None, None)
    with pytest.raises(CtrHipError, match="outside"):
        lib.ctr_td3_noise(-1, 1, 0, FAKE, None)

    def act(B=4, A=3, pre_c=FAKE, ldp=3, mode=0, n_c=None, c=FAKE):
        lib.ctr_td3_act(B, A, pre_c, FAKE, ldp, mode, n_c, None, 7, 0.1, c, FAKE, FAKE, FAKE, None)

    with pytest.raises(CtrHipError, match="A=65"):
        act(A=65, ldp=65)
    with pytest.raises(CtrHipError, match="A=0"):
        act(A=0)
    with pytest.raises(CtrHipError, match="null pre_c"):
        act(pre_c=None)
    with pytest.raises(CtrHipError, match="null pre_c"):
        act(c=None)
    with pytest.raises(CtrHipError, match="ldp"):
        act(ldp=2)
    with pytest.raises(CtrHipError, match="noise_mode 3"):
        act(mode=3)
    with pytest.raises(CtrHipError, match="null noise_c"):
        act(mode=1, n_c=FAKE)  # noise_d missing
    with pytest.raises(CtrHipError, match="B=0"):
        act(B=0)

    def smooth(B=4, A=3, mc=FAKE, ldm=3, mode=2, out_c=FAKE, ldo=10):
        lib.ctr_td3_smooth(B, A, mc, FAKE, ldm, 1, mode, None, None, 7, out_c, FAKE, ldo, None)

    with pytest.raises(CtrHipError, match="A=65"):
        smooth(A=65, ldm=65, ldo=65)
    with pytest.raises(CtrHipError, match="null mean_c"):
        smooth(mc=None)
    with pytest.raises(CtrHipError, match="null mean_c"):
        smooth(out_c=None)
    with pytest.raises(CtrHipError, match="row stride"):
        smooth(ldo=2)
    with pytest.raises(CtrHipError, match="row stride"):
        smooth(ldm=2)
    with pytest.raises(CtrHipError, match="noise_mode 0"):
        smooth(mode=0)
    with pytest.raises(CtrHipError, match="null noise_c"):
        smooth(mode=1)

    def closs(B=4, q1=FAKE, ldr=1, loss=FAKE):
        lib.ctr_td3_critic_loss(B, q1, FAKE, FAKE, FAKE, FAKE, ldr, FAKE, 1.0, FAKE, FAKE, loss,
                                FAKE, FAKE, None)

    with pytest.raises(CtrHipError, match="null q1"):
        closs(q1=None)
    with pytest.raises(CtrHipError, match="null q_target"):
        closs(loss=None)
    with pytest.raises(CtrHipError, match="B=0"):
        closs(B=0)
    with pytest.raises(CtrHipError, match="ldr"):
        closs(ldr=0)

    with pytest.raises(CtrHipError, match="count=0"):
        lib.ctr_soft_update_multi(0, FAKE, 10, 0.005, None)
    with pytest.raises(CtrHipError, match="count=4097"):
        lib.ctr_soft_update_multi(4097, FAKE, 10, 0.005, None)
    with pytest.raises(CtrHipError, match="null table"):
        lib.ctr_soft_update_multi(3, None, 10, 0.005, None)
    with pytest.raises(CtrHipError, match="max_numel=0"):
        lib.ctr_soft_update_multi(3, FAKE, 0, 0.005, None)
    with pytest.raises(CtrHipError, match="tau"):
        lib.ctr_soft_update_multi(3, FAKE, 10, 1.5, None)


def test_struct_forms_validate_like_the_flat_entry_points(built_lib):
    from rl_ctr_prediction_amd._lib import OP_ARGS, CtrHipError, lib
    for op in ("bn_forward", "bn_backward", "td3_noise", "td3_act", "td3_smooth",
               "td3_critic_loss", "soft_update_multi"):
        with pytest.raises(CtrHipError, match="null argument struct"):
            getattr(lib, f"ctr_op_{op}")(None, None)
    a = OP_ARGS["bn_forward"](B=1, N=8, x=FAKE, ldx=8, gamma=FAKE, beta=FAKE, running_mean=FAKE,
                              running_var=FAKE, eps=1e-5, momentum=0.1, training=1, relu=0, y=FAKE,
                              ldy=8)
    with pytest.raises(CtrHipError, match="B >= 2"):
        lib.ctr_op_bn_forward(C.byref(a), None)
    b = OP_ARGS["td3_act"](B=4, A=65, pre_c=FAKE, pre_d=FAKE, ldp=65, c_actions=FAKE, d_actions=FAKE)
    with pytest.raises(CtrHipError, match="A=65"):
        lib.ctr_op_td3_act(C.byref(b), None)
    c = OP_ARGS["soft_update_multi"](count=5000, table=FAKE, max_numel=4, tau=0.5)
    with pytest.raises(CtrHipError, match="count=5000"):
        lib.ctr_op_soft_update_multi(C.byref(c), None)


def test_struct_mirrors_match_header(tmp_path):
    import shutil
    import subprocess
    from conftest import ROOT
    from rl_ctr_prediction_amd import _lib as L
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    structs = {"ctr_bn_forward_args": "BnForwardArgs", "ctr_bn_backward_args": "BnBackwardArgs",
               "ctr_td3_noise_args": "Td3NoiseArgs", "ctr_td3_act_args": "Td3ActArgs",
               "ctr_td3_smooth_args": "Td3SmoothArgs",
               "ctr_td3_critic_loss_args": "Td3CriticLossArgs",
               "ctr_soft_update_multi_args": "SoftUpdateMultiArgs",
               "ctr_soft_update_entry": "SoftUpdateEntry"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "ctr_hip.h"', "int main(void) {"]
    for cname, pyname in structs.items():
        lines.append(f'  printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in getattr(L, pyname)._fields_:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}
    for cname, pyname in structs.items():
        st = getattr(L, pyname)
        assert got[(cname, "size")] == C.sizeof(st), cname
        for f, _ in st._fields_:
            assert got[(cname, f)] == getattr(st, f).offset, (cname, f)


def test_cpu_tensors_are_refused(built_lib):
    from rl_ctr_prediction_amd import hip_ops
    from rl_ctr_prediction_amd.hybrid_td3_model_per import Critic, hybrid_actors
    x, v = torch.zeros(4, 8), torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.bn_forward(x, v, v, v, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.bn_backward(x, x, v, v, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.td3_noise(8, 1, out=torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.td3_act(torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.td3_smooth(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 3),
                           torch.zeros(4, 3), seed=1)
    q = torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.td3_critic_loss(q, q, q, q, q, q, 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_ops.SoftUpdateTable([torch.zeros(4)], [torch.zeros(4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hybrid_actors(8, 3).evaluate(torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Critic(8, 3, 3).evaluate(torch.zeros(4, 8), torch.zeros(4, 3), torch.zeros(4, 3))


def test_new_names_are_exported():
    import rl_ctr_prediction_amd as pkg
    from rl_ctr_prediction_amd import hip_ops, hybrid_td3_model_per as M
    for n in ("Hybrid_TD3_Model", "Critic", "hybrid_actors"):
        assert n in pkg.__all__ and getattr(pkg, n) is getattr(M, n)
    assert M.Memory is pkg.PrioritizedMemory
    for n in ("bn_forward", "bn_backward", "td3_noise", "td3_act", "td3_smooth",
              "td3_critic_loss", "soft_update_multi", "SoftUpdateTable"):
        assert n in hip_ops.__all__ and hasattr(hip_ops, n)
