"""The hybrid TD3 agent on the GPU: the kernels of csrc/td3.hip against fp64 evaluations of the
formulas (td3_ref), and the agent against td3_ref (teacher-forced, one learn at a time) and
against the reference's recorded run (free-running, tests/golden/g_td3*.npz).

Bars. Kernels and the teacher-forced agent: the project's kernel bar, 1e-5 relative + 1e-6 x
max|expected| (conftest.assert_grad_close); a bias gradient that is zero in exact arithmetic
(see td3_ref.RefTD3) is judged against its summands, the same function's `cond` form.
Free-running: the reference's own fp32-versus-fp64 distance for that quantity and call, from the
fixture, times 10, and never less than the kernel bar. Measured figures: DESIGN.md section 6e.
Every test prints what it measured before it asserts."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import td3_ref
from conftest import assert_grad_close, grad_bound

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1


def _np(t):
    if not torch.is_tensor(t):
        return np.asarray(t, dtype=np.float64)
    return t.detach().double().cpu().numpy()


def close(actual, desired, what, cond=None):
    assert_grad_close(_np(actual) if torch.is_tensor(actual) else actual,
                      _np(desired) if torch.is_tensor(desired) else desired,
                      cond=None if cond is None else _np(cond), err_msg=what)


def strided(dev, B, N, ld, offset, fill=None, gen=None, scale=1.0):
    """A [B, N] view with row stride ld that starts `offset` floats into its buffer (offset 1:
    4 bytes off a 16-byte boundary), and the buffer."""
    buf = torch.full((B * ld + offset + 3,), 777.0 if fill is None else fill, device=dev)
    v = buf[offset:offset + B * ld].view(B, ld)[:, :N]
    if gen is not None:
        v.copy_(torch.randn(B, N, device=dev, generator=gen) * scale)
    return v, buf


# ------------------------------------------------------------------ BatchNorm1d ------
LAYOUTS = {"dense": (0, 0), "padded": (7, 0), "padded4": (8, 0), "offset": (0, 1),
           "padded_offset": (5, 1)}


@pytest.mark.parametrize("B", [2, 3, 64, 65, 257])
@pytest.mark.parametrize("N", [1, 3, 64, 65, 200, 401])
def test_bn_forward_backward(cuda, B, N):
    from rl_ctr_prediction_amd import hip_ops
    g = torch.Generator(device=cuda).manual_seed(1000 * B + N)
    gamma = torch.randn(N, device=cuda, generator=g)
    beta = torch.randn(N, device=cuda, generator=g)
    rm0 = torch.randn(N, device=cuda, generator=g)
    rv0 = torch.rand(N, device=cuda, generator=g) + 0.5
    for li, (lname, (pad, off)) in enumerate(LAYOUTS.items()):
        ld = N + pad
        x, _ = strided(cuda, B, N, ld, off, gen=g, scale=2.0)
        x += 0.5
        x[:, 0] = 3.25                       # a constant column: var 0, invstd eps^-1/2
        if N > 1:                            # mean 100, std 0.1: one-pass variance loses it
            x[:, 1] = 100.0 + 0.1 * torch.randn(B, device=cuda, generator=g)
        dy, _ = strided(cuda, B, N, ld, off, gen=g)
        relu, want_dx = bool(li & 1), li != 2
        xd = x.double().requires_grad_(True)
        gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        ref = td3_ref.bn_ref(xd, gd, bd, rm0.double(), rv0.double(), EPS, MOM, True, relu)
        ref["y"].backward(dy.double())
        y, ybuf = strided(cuda, B, N, ld, off)
        rm, rv = rm0.clone(), rv0.clone()
        r = hip_ops.bn_forward(x, gamma, beta, rm, rv, eps=EPS, momentum=MOM, training=True,
                               relu=relu, out=y)
        what = f"B={B} N={N} {lname} relu={relu}"
        close(y, ref["y"], what + " y")
        close(r["mean"], ref["mean"], what + " mean")
        close(r["invstd"], ref["invstd"], what + " invstd")
        close(rm, ref["rm"], what + " running_mean")
        close(rv, ref["rv"], what + " running_var")
        assert abs(float(r["invstd"][0]) - EPS ** -0.5) <= 1e-5 * EPS ** -0.5
        mask = torch.ones_like(ybuf, dtype=torch.bool)
        mask[off:off + B * ld].view(B, ld)[:, :N] = False
        assert bool((ybuf[mask] == 777.0).all()), what + ": wrote outside y"
        dx, dxbuf = strided(cuda, B, N, ld, off)
        b = hip_ops.bn_backward(dy, x, r["mean"], r["invstd"], gamma, y=y, relu=relu,
                                mean_lo=r["mean_lo"], invstd_lo=r["invstd_lo"], want_dx=want_dx,
                                dx=dx if want_dx else None)
        close(b["dgamma"], gd.grad, what + " dgamma")
        close(b["dbeta"], bd.grad, what + " dbeta")
        if want_dx:
            close(b["dx"], xd.grad, what + " dx")
        else:
            assert b["dx"] is None
        assert bool((dxbuf[mask] == 777.0).all()) and (want_dx or bool((dxbuf == 777.0).all()))
        # the same bits again
        y2, _ = strided(cuda, B, N, ld, off)
        rm2, rv2 = rm0.clone(), rv0.clone()
        r2 = hip_ops.bn_forward(x, gamma, beta, rm2, rv2, eps=EPS, momentum=MOM, training=True,
                                relu=relu, out=y2)
        b2 = hip_ops.bn_backward(dy, x, r["mean"], r["invstd"], gamma, y=y, relu=relu,
                                 mean_lo=r["mean_lo"], invstd_lo=r["invstd_lo"], want_dx=want_dx)
        assert torch.equal(y2, y) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
        assert torch.equal(r2["invstd"], r["invstd"]) and torch.equal(b2["dgamma"], b["dgamma"])
        assert torch.equal(b2["dbeta"], b["dbeta"])
        if want_dx:
            assert torch.equal(b2["dx"], b["dx"])
        # a second call moves the running statistics again
        x2 = x * 0.5 - 1.0
        ref2 = td3_ref.bn_ref(x2.double(), gamma.double(), beta.double(), ref["rm"].detach(),
                              ref["rv"].detach(), EPS, MOM, True, relu)
        hip_ops.bn_forward(x2.contiguous(), gamma, beta, rm, rv, eps=EPS, momentum=MOM,
                           training=True, relu=relu, save=False)
        close(rm, ref2["rm"], what + " running_mean, 2nd call")
        close(rv, ref2["rv"], what + " running_var, 2nd call")


@pytest.mark.parametrize("N", [1, 3, 64, 65])
def test_bn_eval_mode_rows(cuda, N):
    from rl_ctr_prediction_amd import hip_ops
    g = torch.Generator(device=cuda).manual_seed(N)
    gamma, beta = torch.randn(N, device=cuda, generator=g), torch.randn(N, device=cuda, generator=g)
    rm = torch.randn(N, device=cuda, generator=g)
    rv = torch.rand(N, device=cuda, generator=g) + 0.1
    for B in (1, 5):
        for relu in (False, True):
            x = torch.randn(B, N, device=cuda, generator=g)
            rm1, rv1 = rm.clone(), rv.clone()
            y = hip_ops.bn_forward(x, gamma, beta, rm1, rv1, eps=EPS, training=False, relu=relu)
            ref = td3_ref.bn_ref(x.double(), gamma.double(), beta.double(), rm.double(),
                                 rv.double(), EPS, MOM, False, relu)
            close(y["y"], ref["y"], f"eval B={B} N={N} relu={relu}")
            assert y["mean"] is None and torch.equal(rm1, rm) and torch.equal(rv1, rv)


def test_bn_training_refuses_one_row(cuda):
    from rl_ctr_prediction_amd import hip_ops
    from rl_ctr_prediction_amd._lib import CtrHipError
    v = torch.ones(4, device=cuda)
    with pytest.raises(CtrHipError, match="B >= 2"):
        hip_ops.bn_forward(torch.zeros(1, 4, device=cuda), v, v, v.clone(), v.clone())


# ---------------------------------------------------------------- elementwise --------
BS, AS = [1, 2, 63, 64, 65, 256], [1, 2, 3, 64]


@pytest.mark.parametrize("A", AS)
def test_act_smooth_critic_loss(cuda, A):
    from rl_ctr_prediction_amd import hip_ops
    g = torch.Generator(device=cuda).manual_seed(77 + A)
    for B in BS:
        pre_c = torch.randn(B, A, device=cuda, generator=g) * 1.5
        pre_d = torch.randn(B, A, device=cuda, generator=g) * 1.5
        cm, dm = torch.tanh(pre_c.double()), torch.tanh(pre_d.double())
        what = f"B={B} A={A}"
        # sigma * noise of 0.8 std: the +-1 clamp is active on many elements
        noise = tuple(torch.randn(B, A, device=cuda, generator=g) * 8 for _ in range(2))
        r = hip_ops.td3_act(pre_c, pre_d, noise=noise, sigma=0.1)
        rc, rsm, rd, rix = td3_ref.act_ref(cm, dm, tuple(n.double() for n in noise), 0.1)
        if B * A >= 64:
            assert bool((rc.abs() == 1).any()) and bool((rc.abs() < 1).any()), "clamp not active"
        close(r["c_actions"], rc, what + " c_actions")
        close(r["c_softmax"], rsm, what + " softmax")
        close(r["d_actions"], rd, what + " d_actions")
        # the index is the first maximum of the kernel's own d_actions ...
        own = r["d_actions"].cpu().numpy().argmax(1) + 1
        assert np.array_equal(r["d_index"].cpu().numpy().reshape(-1), own), what
        # ... and the reference's wherever the reference has no (near) tie
        if A > 1:
            top = torch.topk(rd, 2, dim=1).values
            clear = ((top[:, 0] - top[:, 1]) > 1e-4).cpu().numpy()
            assert np.array_equal(r["d_index"].cpu().numpy()[clear], rix.cpu().numpy()[clear]), what
        # no noise: tanh only (evaluate), softmax and index of the means (choose_best_action)
        r0 = hip_ops.td3_act(pre_c, pre_d)
        e = td3_ref.act_ref(cm, dm)
        close(r0["c_actions"], e[0], what + " tanh c")
        close(r0["c_softmax"], e[1], what + " softmax of means")
        close(r0["d_actions"], e[2], what + " tanh d")
        if A > 1:
            top = torch.topk(e[2], 2, dim=1).values
            clear = ((top[:, 0] - top[:, 1]) > 1e-4).cpu().numpy()
            assert np.array_equal(r0["d_index"].cpu().numpy()[clear], e[3].cpu().numpy()[clear])
        else:
            assert bool((r0["d_index"] == 1).all()) and bool((r0["c_softmax"] == 1).all())

        # smoothing into two column blocks of a wider matrix; 0.2 * noise of 0.6 std hits +-0.5
        sn = tuple(torch.randn(B, A, device=cuda, generator=g) * 3 for _ in range(2))
        D = 5
        buf = torch.full((B, D + 2 * A + 2), 777.0, device=cuda)
        hip_ops.td3_smooth(pre_c, pre_d, buf[:, D:D + A], buf[:, D + A:D + 2 * A], noise=sn,
                           apply_tanh=True)
        sc, sd = td3_ref.smooth_ref(cm, dm, tuple(n.double() for n in sn))
        if B * A >= 64:
            inner = torch.clamp(sn[0].double() * 0.2, -0.5, 0.5)
            assert bool((inner.abs() == 0.5).any()) and bool((sc.abs() == 1).any())
        close(buf[:, D:D + A], sc, what + " smooth c")
        close(buf[:, D + A:D + 2 * A], sd, what + " smooth d")
        assert bool((buf[:, :D] == 777.0).all()) and bool((buf[:, D + 2 * A:] == 777.0).all())
        out2 = torch.empty(2, B, A, device=cuda)  # means given after the tanh
        hip_ops.td3_smooth(r0["c_actions"], r0["d_actions"], out2[0], out2[1], noise=sn)
        close(out2[0], sc, what + " smooth c (means)")

        # seed mode consumes exactly what td3_noise returns
        seed = 1234567 + B
        n_c = hip_ops.td3_noise(B * A, seed, 0, device=cuda).view(B, A)
        n_d = hip_ops.td3_noise(B * A, seed, B * A, device=cuda).view(B, A)
        rs, rp = hip_ops.td3_act(pre_c, pre_d, seed=seed), hip_ops.td3_act(pre_c, pre_d,
                                                                           noise=(n_c, n_d))
        for k in ("c_actions", "c_softmax", "d_actions", "d_index"):
            assert torch.equal(rs[k], rp[k]), f"{what} act seed vs pointer: {k}"
        o_s, o_p = torch.empty(2, B, A, device=cuda), torch.empty(2, B, A, device=cuda)
        hip_ops.td3_smooth(pre_c, pre_d, o_s[0], o_s[1], seed=seed, apply_tanh=True)
        hip_ops.td3_smooth(pre_c, pre_d, o_p[0], o_p[1], noise=(n_c, n_d), apply_tanh=True)
        assert torch.equal(o_s, o_p), what + " smooth seed vs pointer"

        # critic loss (r: a strided column, as in the sampled batch)
        q = [torch.randn(B, 1, device=cuda, generator=g) for _ in range(4)]
        batch = torch.randn(B, 7, device=cuda, generator=g)
        isw = torch.rand(B, 1, device=cuda, generator=g) + 0.1
        o = hip_ops.td3_critic_loss(*q, batch[:, -1], isw, 0.9)
        e = td3_ref.critic_loss_ref(*(t.double() for t in q), batch[:, -1:].double(),
                                    isw.double(), 0.9)
        for k in ("q_target", "td", "loss", "dq1", "dq2"):
            close(o[k], e[k], f"{what} critic loss {k}")
        o2 = hip_ops.td3_critic_loss(*q, batch[:, -1], isw, 0.9)
        assert all(torch.equal(o[k], o2[k]) for k in o)


def test_act_tie_takes_the_lower_index(cuda):
    from rl_ctr_prediction_amd import hip_ops
    pre_d = torch.tensor([[0.1, 0.7, 0.7, -0.2], [0.3, 0.3, 0.3, 0.3], [-1.0, 0.5, 0.2, 0.5]],
                         device=cuda)
    r = hip_ops.td3_act(torch.zeros_like(pre_d), pre_d)
    assert r["d_index"].reshape(-1).tolist() == [2, 1, 2]
    # saturated by the clamp: every element of the row is 1
    big = torch.full((3, 4), 100.0, device=cuda)
    r = hip_ops.td3_act(torch.zeros_like(pre_d), pre_d, noise=(big, big), sigma=0.1)
    assert bool((r["d_actions"] == 1).all()) and r["d_index"].reshape(-1).tolist() == [1, 1, 1]


def test_noise_statistics(cuda):
    from rl_ctr_prediction_amd import hip_ops
    n = 1 << 20
    z = hip_ops.td3_noise(n, 42, device=cuda).double()
    mean, var = float(z.mean()), float(z.var())
    frac = float((z.abs() > 2).double().mean())
    p = 0.04550026389635842  # P(|z| > 2)
    print(f"noise: mean {mean:.3g} (5 sigma {5 / n ** 0.5:.3g}), var - 1 {var - 1:.3g} "
          f"(5 sigma {5 * (2 / n) ** 0.5:.3g}), tail {frac - p:.3g} "
          f"(5 sigma {5 * (p * (1 - p) / n) ** 0.5:.3g})")
    assert abs(mean) < 5 / n ** 0.5
    assert abs(var - 1) < 5 * (2 / n) ** 0.5
    assert abs(frac - p) < 5 * (p * (1 - p) / n) ** 0.5
    assert bool(torch.isfinite(z).all()) and float(z.abs().max()) < 5.9
    z2 = hip_ops.td3_noise(n, 43, device=cuda).double()
    assert float((z2 == z).double().mean()) < 1e-3 and abs(float((z * z2).mean())) < 5 / n ** 0.5
    assert torch.equal(hip_ops.td3_noise(n, 42, device=cuda).double(), z)
    # an offset continues the stream
    assert torch.equal(hip_ops.td3_noise(1000, 42, 500, device=cuda).double(), z[500:1500])


def test_soft_update_multi(cuda):
    from rl_ctr_prediction_amd import hip_ops
    g = torch.Generator(device=cuda).manual_seed(9)
    sizes = [1, 3, 64, 65, 120000]
    tgt = [torch.randn(n, device=cuda, generator=g) for n in sizes]
    src = [torch.randn(n, device=cuda, generator=g) for n in sizes]
    tbuf = torch.randn(1004, device=cuda, generator=g)
    sbuf = torch.randn(1004, device=cuda, generator=g)
    tgt.append(tbuf[1:1002])   # 4 bytes off a 16-byte boundary
    src.append(sbuf[2:1003])   # and its source 8 bytes off
    tgt.append(torch.randn(12, 11, device=cuda, generator=g))
    src.append(torch.randn(12, 11, device=cuda, generator=g))
    for tau in (0.005, 0.3, 0.0, 1.0):
        t0 = [t.clone() for t in tgt]
        edge = (tbuf[0].clone(), tbuf[1002:].clone())
        expect = [t * (1.0 - tau) + s * tau for t, s in zip(tgt, src)]  # the reference's line
        hip_ops.soft_update_multi(hip_ops.SoftUpdateTable(tgt, src), tau)
        for i, (t, e) in enumerate(zip(tgt, expect)):
            assert torch.equal(t, e), f"tau={tau} tensor {i}"
        if tau == 0.0:
            assert all(torch.equal(t, a) for t, a in zip(tgt, t0))
        if tau == 1.0:
            assert all(torch.equal(t, s) for t, s in zip(tgt, src))
        assert torch.equal(tbuf[0], edge[0]) and torch.equal(tbuf[1002:], edge[1])


# --------------------------------------------------------------------- the agent ------
@pytest.fixture(scope="module")
def gold():
    return td3_ref.load_golden(["g_td3.npz", "g_td3_f32_b.npz", "g_td3_f64_d.npz"])


def make_agent(gold, dev, seed=0):
    from rl_ctr_prediction_amd import Feature_Embedding, Hybrid_TD3_Model
    V, F, K, A, B, MEM, _ = (int(v) for v in gold["shapes"])
    torch.manual_seed(seed)
    agent = Hybrid_TD3_Model(V, field_nums=F, latent_dims=K, action_nums=A, memory_size=MEM,
                             batch_size=B, device=dev)
    fe = Feature_Embedding(V, F, K).to(dev)
    fe.feature_embedding.weight.data.copy_(torch.from_numpy(gold["emb"]))
    trans = torch.from_numpy(gold["transitions"]).to(dev)
    agent.store_transition(trans[:40])
    agent.store_transition(trans[40:])
    return agent, fe


def recorded(gold, i, dev):
    t = f"c{i}"
    sample = tuple(torch.from_numpy(gold[f"{t}/{k}"]).to(dev) for k in ("idx", "batch", "isw"))
    noise = tuple(torch.from_numpy(gold[f"{t}/{k}"]).to(dev) for k in ("n_c", "n_d"))
    return sample, noise


def adam64(p, g, m, v, step, lr, b1=0.9, b2=0.999, eps=1e-8):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - (lr / (1 - b1 ** step)) * m / (np.sqrt(v / (1 - b2 ** step)) + eps)


def test_teacher_forced_step_parity(cuda, gold):
    """Four consecutive learns, each started from the HIP agent's own state copied into td3_ref
    in fp64 (parameters, buffers, Adam state), on the recorded samples and noise.

    The forcing also covers the one place inside a learn where Adam's sensitivity enters: the
    4th learn runs Critic.evaluate_q_1 AFTER the critic's step, and a Linear bias in front of a
    BatchNorm has a gradient of pure rounding noise that Adam turns into a step of ~lr (see
    td3_ref.RefTD3), which then shifts that BatchNorm's running_mean by momentum x the step. So
    td3_ref continues from the HIP path's stepped critic parameters, which are themselves
    checked against Adam applied in fp64 to the HIP path's own gradients."""
    V, F, K, A, B, MEM, _ = (int(v) for v in gold["shapes"])
    D = F * (F - 1) // 2 + F * K
    agent, fe = make_agent(gold, cuda)
    emb64 = fe.feature_embedding.weight.detach().double()
    ref = td3_ref.RefTD3(D, F, A, dtype=torch.float64, device=cuda, batch_size=B)
    worst = {}

    def note(k, a, d):
        a, d = _np(a), _np(d)
        worst[k] = max(worst.get(k, 0.0), float(np.max(np.abs(a - d) / grad_bound(d))))

    for i in range(4):
        ref.load_from(agent)
        before = {n: {k: _np(v) for k, v in getattr(agent, n).state_dict().items()}
                  for n in ref.nets()}
        adam = {}
        for tag, opt, net in (("c", agent.optimizer_c, agent.Critic),
                              ("a", agent.optimizer_a, agent.Hybrid_Actor)):
            for n, p in net.named_parameters():
                st = opt.state.get(p)
                adam[tag, n] = (_np(st["exp_avg"]), _np(st["exp_avg_sq"]), int(st["step"])) \
                    if st else (0.0, 0.0, 0)
        sample, noise = recorded(gold, i, cuda)
        loss = agent.learn(fe, sample=sample, noise=noise)

        def force_stepped_critic():
            with torch.no_grad():
                for pr, p in zip(ref.Critic.parameters(), agent.Critic.parameters()):
                    pr.copy_(p.double())

        o = ref.learn(lambda ids: td3_ref.embed_state(emb64, ids), sample=sample, noise=noise,
                      after_critic_step=force_stepped_critic)
        what = f"learn {i}"
        for k in ("q1", "q2", "q_target", "td"):
            note(k, agent.last[k], o[k])
            close(agent.last[k], o[k], f"{what} {k}")
        note("loss", np.float64(loss), o["loss"])
        close(np.array([loss]), o["loss"].reshape(1), what + " loss")
        actor_step = (i + 1) % 4 == 0
        assert ("ga" in o) == actor_step
        for tag, net, lr in (("gc", agent.Critic, agent.lr_C), ("ga", agent.Hybrid_Actor,
                                                                  agent.lr_C_A)):
            if tag == "ga" and not actor_step:
                for n, t in net.state_dict().items():  # untouched by this learn, buffers too
                    assert np.array_equal(_np(t), before["Hybrid_Actor"][n]), n
                continue
            netname = "Critic" if tag == "gc" else "Hybrid_Actor"
            for n, p in net.named_parameters():
                cond = o[tag + "_cond"].get(n)
                if cond is None:
                    note(tag, p.grad, o[tag][n])
                close(p.grad, o[tag][n], f"{what} {tag}/{n}", cond=cond)
                m, v, step = adam[tag[1], n]
                want = adam64(before[netname][n], _np(p.grad), m, v, step + 1, lr)
                np.testing.assert_allclose(_np(p), want, rtol=1e-6, atol=1e-6,
                                           err_msg=f"{what} {netname}.{n} after Adam")
        for n, net in ref.nets().items():
            mine = getattr(agent, n)
            for k, b in net.named_buffers():
                got = dict(mine.named_buffers())[k]
                if k.endswith("num_batches_tracked"):
                    assert int(got) == int(b), f"{what} {n}.{k}"
                else:
                    note("bn buffers", got, b)
                    close(got, b, f"{what} {n}.{k}")
        for n, src in (("Critic_", "Critic"), ("Hybrid_Actor_", "Hybrid_Actor")):
            now = dict(getattr(agent, src).named_parameters())
            for k, p in getattr(agent, n).named_parameters():
                want = before[n][k]
                if actor_step:
                    want = want * (1.0 - agent.tau) + _np(now[k]) * agent.tau
                np.testing.assert_allclose(_np(p), want, rtol=1e-6, atol=1e-6 if actor_step else 0,
                                           err_msg=f"{what} {n}.{k} after the soft update")
        idx = sample[0]
        note("priorities", agent.memory.prioritys_[idx], td3_ref.priority(o["td"]))
        close(agent.memory.prioritys_[idx], td3_ref.priority(o["td"]), what + " priorities")
    print("teacher-forced: worst error / bar:", {k: round(v, 4) for k, v in worst.items()})
    assert agent.learn_iter == 4 and agent.Hybrid_Actor.training and agent.Critic_.training


def test_free_running_parity_with_the_reference_record(cuda, gold):
    """Eight learns from the seeded state on the recorded samples and noise. Per quantity and
    call the bar is 10 x the reference's own fp32-vs-fp64 distance (its largest element), never
    less than the kernel bar; the distance is taken to the fp64 record."""
    agent, fe = make_agent(gold, cuda)
    rows = []

    def judge(what, got, f32, f64):
        got, f32, f64 = (np.asarray(a, dtype=np.float64) for a in (got, f32, f64))
        gap = float(np.max(np.abs(f32 - f64))) if f64.size else 0.0
        dist = float(np.max(np.abs(got - f64))) if f64.size else 0.0
        bar = np.maximum(10.0 * gap, grad_bound(f64))
        rows.append((what, gap, dist, float(np.max(np.abs(got - f64) / bar)) if f64.size else 0.0))
        return bool((np.abs(got - f64) <= bar).all())

    ok = True
    for i in range(8):
        sample, noise = recorded(gold, i, cuda)
        loss = agent.learn(fe, sample=sample, noise=noise)
        t = f"c{i}"
        for k in ("q1", "q2", "q_target", "td"):
            ok &= judge(f"{t}/{k}", _np(agent.last[k]), gold[f"{t}/{k}"], gold[f"f64/{t}/{k}"])
        ok &= judge(f"{t}/loss", [loss], [gold[f"{t}/loss"]], [gold[f"f64/{t}/loss"]])
    for n in ("Hybrid_Actor", "Hybrid_Actor_", "Critic", "Critic_"):
        for k, v in getattr(agent, n).state_dict().items():
            a = _np(v)
            key = f"c7/{n}/{k}"
            if key not in gold:
                a, key = a[::37, ::11], key + "@s"
            ok &= judge(key, a, gold[key], gold["f64/" + key])
    ok &= judge("c7/prio", _np(agent.memory.prioritys_), gold["c7/prio"], gold["f64/c7/prio"])
    print("free-running parity: quantity, reference fp32-vs-fp64 gap, HIP distance to fp64, "
          "distance / bar")
    for what, gap, dist, frac in rows:
        if "/" not in what[3:] or frac > 0.5:
            print(f"  {what:48s} {gap:10.3g} {dist:10.3g} {frac:8.3g}")
    state = [r for r in rows if r[0].count("/") == 2]
    print(f"  final state: {len(state)} entries, largest gap {max(r[1] for r in state):.3g}, "
          f"largest HIP distance {max(r[2] for r in state):.3g}, "
          f"largest distance / bar {max(r[3] for r in state):.3g}")
    assert ok, [r for r in rows if r[3] > 1]

    # the actions of the trained actor, eval-mode BatchNorm, against the record
    ids = torch.from_numpy(gold["states5"]).to(cuda)
    with torch.no_grad():
        s5 = fe(ids)
    noise = (torch.from_numpy(gold["act/n_c"]).to(cuda), torch.from_numpy(gold["act/n_d"]).to(cuda))
    c, sm, d, ix = agent.choose_action(s5, noise=noise)
    assert agent.Hybrid_Actor.training
    rows.clear()
    ok = judge("act/c_actions", _np(c), gold["act/c_actions"], gold["f64/act/c_actions"])
    ok &= judge("act/c_softmax", _np(sm), gold["act/c_softmax"], gold["f64/act/c_softmax"])
    ok &= judge("act/d_actions", _np(d), gold["act/d_actions"], gold["f64/act/d_actions"])
    bix, bsm = agent.choose_best_action(s5)
    assert agent.Hybrid_Actor.training
    ok &= judge("best/c_softmax", _np(bsm), gold["best/c_softmax"], gold["f64/best/c_softmax"])
    for r in rows:
        print(f"  {r[0]:48s} {r[1]:10.3g} {r[2]:10.3g} {r[3]:8.3g}")
    assert ok, rows
    top = np.sort(gold["f64/act/d_actions"], axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-3
    assert np.array_equal(ix.cpu().numpy()[clear], gold["act/d_index"][clear])
    assert ix.dtype == torch.int64 and tuple(ix.shape) == (5, 1) and tuple(bix.shape) == (5, 1)
    agent.Hybrid_Actor.eval()
    with torch.no_grad():
        means = _np(agent.Hybrid_Actor.evaluate(s5)[1])
    agent.Hybrid_Actor.train()
    top = np.sort(means, axis=1)
    clear = (top[:, -1] - top[:, -2]) > 1e-3
    assert np.array_equal(bix.cpu().numpy()[clear], gold["best/d_index"][clear])
    assert np.array_equal(bix.cpu().numpy().reshape(-1), means.argmax(1) + 1)


def test_learn_makes_no_host_synchronisation(cuda, gold):
    agent, fe = make_agent(gold, cuda)
    for _ in range(4):  # warm-up, the actor update and both soft updates included
        agent.learn(fe, return_tensor=True)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [agent.learn(fe, return_tensor=True) for _ in range(4)]
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert agent.learn_iter == 8
    assert all(l.is_cuda and l.dim() == 0 and bool(torch.isfinite(l)) for l in losses)
    assert isinstance(agent.learn(fe), float)


def test_seeded_free_runs_are_bitwise_equal(cuda, gold):
    def run():
        agent, fe = make_agent(gold, cuda, seed=3)
        losses = [agent.learn(fe, return_tensor=True) for _ in range(8)]
        ids = torch.from_numpy(gold["states5"]).to(cuda)
        with torch.no_grad():
            acts = agent.choose_action(fe(ids))
        state = [v.clone() for n in ("Hybrid_Actor", "Hybrid_Actor_", "Critic", "Critic_")
                 for v in getattr(agent, n).state_dict().values()]
        return torch.stack(losses), state + list(acts) + [agent.memory.prioritys_.clone()]
    l1, s1 = run()
    l2, s2 = run()
    assert torch.equal(l1, l2) and len(s1) == len(s2)
    assert all(torch.equal(a, b) for a, b in zip(s1, s2))
    assert float(l1.std()) > 0  # the learns differ from one another: samples and noise move


def test_state_dict_round_trip(cuda, gold):
    from rl_ctr_prediction_amd import Critic, hybrid_actors
    V, F, K, A, B, MEM, _ = (int(v) for v in gold["shapes"])
    D = F * (F - 1) // 2 + F * K
    g = torch.Generator().manual_seed(4)
    for mine, theirs in ((Critic(D, A, A), td3_ref.RefCritic(D, A, A)),
                         (hybrid_actors(D, A), td3_ref.RefActor(D, A))):
        sd = theirs.state_dict()  # a checkpoint with the reference's keys
        for k, v in sd.items():
            if v.is_floating_point():
                v.copy_(torch.rand(v.shape, generator=g) + 0.5)
            else:
                v.fill_(7)
        mine.load_state_dict(sd, strict=True)
        mine.to(cuda)
        theirs.to(cuda)
        back = mine.state_dict()
        assert list(back) == list(sd) and all(torch.equal(back[k].cpu(), sd[k].cpu()) for k in sd)
        s = torch.randn(B, D, device=cuda)
        with torch.no_grad():
            if isinstance(mine, Critic):
                c, d = torch.rand(B, A, device=cuda), torch.rand(B, A, device=cuda)
                got, want = mine.evaluate(s, c, d), theirs.double().evaluate(s.double(), c.double(),
                                                                             d.double())
            else:
                got, want = mine.evaluate(s), theirs.double().evaluate(s.double())
        for a, b in zip(got, want):
            close(a, b, type(mine).__name__ + " after load_state_dict")
        assert int(mine.bn_input.num_batches_tracked) == 8
