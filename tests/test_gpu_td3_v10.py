"""The v10 hybrid TD3 agent on the GPU: the kernels of csrc/td3_v10.hip against fp64 evaluations
of the formulas (td3_v10_ref), and the agent against td3_v10_ref (teacher-forced, one learn at a
time) and against the reference's recorded run (free-running, tests/golden/g_v10_td3*.npz).

Bars. Kernels and the teacher-forced agent: the project's kernel bar, 1e-5 relative + 1e-6 x
max|expected| (conftest.assert_grad_close). A Gumbel-softmax output additionally carries the
rounding of its own fp32 logit z = (...) / T: z is the result of four fp32 operations and a
logf, each within 2^-24 |z| (the logf within 2 ulp), and an error dz of a logit moves a
probability p by at most 2 p dz (its own exponent and the normaliser), so such outputs get
16 x 2^-24 x max|z| x p on top (softmax_bar), max|z| taken over the output's own row: 1.9e-5 p
at |z| = 20, about twice the relative part of the kernel bar, and nothing where the logits are
small.
Free-running: per quantity and call 10 x the reference's own fp32-versus-fp64 distance from the
fixture, never less than the kernel bar; the distance is taken to the fp64 record. Discrete
outputs must be equal: the fixture's decision margin leaves no example out.
Every test prints what it measured before it asserts."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import td3_v10_ref as R
from conftest import assert_grad_close, grad_bound
from test_gpu_td3 import LAYOUTS, adam64, strided

pytestmark = pytest.mark.gpu

BS, AS = [1, 2, 3, 64, 65, 257], [1, 2, 3, 6, 64]


def _np(t):
    if not torch.is_tensor(t):
        return np.asarray(t, dtype=np.float64)
    return t.detach().double().cpu().numpy()


def close(actual, desired, what, extra=None):
    a, d = _np(actual), _np(desired)
    if extra is None:
        assert_grad_close(a, d, err_msg=what)
        return
    bar = grad_bound(d) + _np(extra)
    bad = np.abs(a - d) > bar
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.size} outside the bar, worst " \
                          f"{np.max(np.abs(a - d) / bar):.3g} x"


def softmax_bar(z, p):
    """The share of a softmax output's bar that its fp32 logits' own rounding accounts for."""
    return 16.0 * 2.0 ** -24 * z.abs().max(1, keepdim=True)[0] * p


def gumbel_logits(d_q, n_d, u, T, doubled):
    g = R.gumbel(u.double())
    base = d_q.double() + (0.2 * n_d.double() + d_q.double()) if doubled else d_q.double()
    return (base + g) / T


def first_argmax(t):
    return t.cpu().numpy().argmax(1) + 1  # numpy: the first of equal maxima


# ------------------------------------------------------------------ action heads ------
@pytest.mark.parametrize("A", AS)
def test_heads_against_fp64(cuda, A):
    from rl_ctr_prediction_amd import hip_ops as H
    g = torch.Generator(device=cuda).manual_seed(500 + A)
    for B, (lname, (pad, off)) in ((B, lay) for B in BS for lay in LAYOUTS.items()):
        ld = 2 * A + pad
        buf, _ = strided(cuda, B, 2 * A, ld, off, gen=g, scale=1.5)
        pre_c, pre_d = buf[:, :A], buf[:, A:]       # two column blocks with one row stride
        n_c = torch.randn(B, A, device=cuda, generator=g) * 3   # the random mode's clamp is active
        n_d = torch.randn(B, A, device=cuda, generator=g)
        u = torch.rand(B, A, device=cuda, generator=g).clamp_(1e-7, 1 - 1e-7)
        if A > 1:                                   # a tie in d: equal logits, noise and uniforms
            pre_d[0, :] = 0.25
            n_d[0, :] = -0.5
            u[0, :] = 0.5
        what = f"B={B} A={A} {lname}"
        for T in (1.0, 0.37):
            r = H.td3v10_heads(H.V10_ACT, pre_c, pre_d, noise_c=n_c, noise_d=n_d, uniform=u,
                               temperature=T)
            e = R.act_ref(pre_c.double(), pre_d.double(), n_c.double(), n_d.double(), u.double(), T)
            z = gumbel_logits(pre_d, n_d, u, T, True)
            close(r["c_means"], e[0], what + " act c_means")
            close(r["c_softmax"], e[1], what + " act c_softmax")
            close(r["d_action"], e[2], what + " act d_action", softmax_bar(z, e[2]))
            assert np.array_equal(r["d_index"].cpu().numpy().reshape(-1), first_argmax(r["d_action"]))
            if A > 1:
                assert int(r["d_index"][0]) == 1, what + ": a tie takes the lowest index"
                top = torch.topk(e[2], 2, dim=1).values
                clear = ((top[:, 0] - top[:, 1]) > 1e-4).cpu().numpy()
                assert np.array_equal(r["d_index"].cpu().numpy()[clear], e[3].cpu().numpy()[clear])
            r = H.td3v10_heads(H.V10_PLAIN, pre_c, pre_d, uniform=u, temperature=T)
            e = R.plain_ref(pre_c.double(), pre_d.double(), u.double(), T)
            close(r["c_means"], e[0], what + " plain c_means")
            close(r["c_softmax"], e[1], what + " plain c_softmax")
            close(r["d_action"], e[2], what + " plain d_action",
                  softmax_bar(gumbel_logits(pre_d, n_d, u, T, False), e[2]))
            assert np.array_equal(r["d_index"].cpu().numpy().reshape(-1), first_argmax(r["d_action"]))
        r = H.td3v10_heads(H.V10_RANDOM, noise_c=n_c, noise_d=n_d)
        e = R.random_ref(n_c.double(), n_d.double())
        if B * A >= 64:
            assert bool((e[0].abs() == 1).any()) and bool((e[0].abs() < 1).any()), "clamp inactive"
        assert torch.equal(r["c_means"], torch.clamp(n_c, -1, 1))
        close(r["c_softmax"], e[1], what + " random c_softmax")
        close(r["d_action"], e[2], what + " random d_action")
        assert np.array_equal(r["d_index"].cpu().numpy().reshape(-1), first_argmax(r["d_action"]))
        r = H.td3v10_heads(H.V10_BEST, pre_c, pre_d, uniform=u, temperature=0.1)
        ix, cm, sm = R.best_ref(pre_c.double(), pre_d.double(), u.double())
        assert r["d_action"] is None
        close(r["c_means"], cm, what + " best c_means")
        close(r["c_softmax"], sm, what + " best softmax")
        y = pre_d.double() + R.gumbel(u.double())
        if A > 1:
            assert int(r["d_index"][0]) == 1
            top = torch.topk(y, 2, dim=1).values
            clear = ((top[:, 0] - top[:, 1]) > 1e-4).cpu().numpy()
            assert np.array_equal(r["d_index"].cpu().numpy()[clear], ix.cpu().numpy()[clear])
        else:
            assert bool((r["d_index"] == 1).all()) and bool((r["c_softmax"] == 1).all())
        r2 = H.td3v10_heads(H.V10_BEST, pre_c, pre_d, uniform=u, temperature=0.1)
        assert all(torch.equal(r[k], r2[k]) for k in ("c_means", "c_softmax", "d_index"))


def test_heads_saturated_softmax_is_finite(cuda):
    from rl_ctr_prediction_amd import hip_ops as H
    g = torch.Generator(device=cuda).manual_seed(8)
    for A in (2, 6, 64):
        B = 65
        pre_d = torch.randn(B, A, device=cuda, generator=g) * 40   # z = d_q / 0.1: +-1000s
        pre_c = torch.randn(B, A, device=cuda, generator=g) * 40   # tanh saturates at +-1
        u = torch.rand(B, A, device=cuda, generator=g).clamp_(1e-7, 1 - 1e-7)
        u[0, 0], u[1, 0] = 2.0 ** -25, 1 - 2.0 ** -24                # the ends of (0, 1)
        n = torch.randn(B, A, device=cuda, generator=g)
        for mode, kw in ((H.V10_PLAIN, {}), (H.V10_ACT, dict(noise_c=n, noise_d=n))):
            r = H.td3v10_heads(mode, pre_c, pre_d, uniform=u, temperature=0.1, **kw)
            for k in ("c_means", "c_softmax", "d_action"):
                assert bool(torch.isfinite(r[k]).all()), k
            s = r["d_action"].double().sum(1)
            print(f"saturated A={A}: largest |row sum - 1| {float((s - 1).abs().max()):.3g}, "
                  f"largest p {float(r['d_action'].max()):.6g}")
            assert float((s - 1).abs().max()) <= 1e-6
            assert float((r["c_softmax"].double().sum(1) - 1).abs().max()) <= 1e-6
            assert bool((r["d_action"].max(1).values > 0.999).any())  # it does saturate
            assert bool(((r["d_index"] >= 1) & (r["d_index"] <= A)).all())


# -------------------------------------------------------------------- rank mask -------
@pytest.mark.parametrize("A", AS)
def test_rank_mask_against_fp64(cuda, A):
    from rl_ctr_prediction_amd import hip_ops as H
    g = torch.Generator(device=cuda).manual_seed(900 + A)
    for B, (lname, (pad, off)) in ((B, lay) for B in BS for lay in LAYOUTS.items()):
        ld = 2 * A + pad
        src, _ = strided(cuda, B, 2 * A, ld, off, gen=g)
        d, c = src[:, :A], src[:, A:]
        noise = torch.randn(B, A, device=cuda, generator=g) * 3    # 0.2 n of 0.6 std: clamp active
        if A > 1:
            c[0, :] = 0.25                       # every value equal: the lower indices win
            c[B // 2, A - 1] = c[B // 2, 0]      # a tie across the row
            d[B - 1, :] = 0.5                    # equal d: choice 1
        d[0, A - 1] = 9.0                        # choice A
        what = f"B={B} A={A} {lname}"
        for nz in (None, noise):
            out, obuf = strided(cuda, B, 2 * A + 3, 2 * A + 3 + pad, off)
            r = H.td3v10_rank_mask(d, c, noise=nz, out_c=out[:, A + 3:], out_d=out[:, 3:A + 3])
            e, keep = R.rank_mask_ref(d.double(), c.double(), None if nz is None else nz.double())
            assert torch.equal(r["keep"].bool(), keep), what + " keep"
            close(out[:, A + 3:], e, what + " masked c")
            assert torch.equal(out[:, 3:A + 3], d), what + " d copy"
            assert bool((out[:, :3] == 777.0).all()), what + ": wrote outside its columns"
            inside = torch.zeros_like(obuf, dtype=torch.bool)
            inside[off:off + B * (2 * A + 3 + pad)].view(B, -1)[:, :2 * A + 3] = True
            assert bool((obuf[~inside] == 777.0).all()), what + ": wrote outside out"
            if nz is not None and B * A >= 64:
                assert bool((e.abs() == 1).any()), "clamp inactive"
            assert bool(keep[0].all()) and int(keep[B - 1].sum()) == (A if B == 1 else 1)
            r2 = H.td3v10_rank_mask(d, c, noise=nz)   # contiguous outputs, no d copy
            assert torch.equal(r2["c"], out[:, A + 3:]) and torch.equal(r2["keep"], r["keep"])


def test_rank_mask_ties_rank_by_index(cuda):
    from rl_ctr_prediction_amd import hip_ops as H
    c = torch.tensor([[0.3, 0.7, 0.7, 0.1]], device=cuda).repeat(4, 1)
    d = torch.eye(4, device=cuda)
    r = H.td3v10_rank_mask(d, c)
    assert r["keep"].tolist() == [[0, 1, 0, 0], [0, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 1]]
    assert torch.equal(r["c"], c * r["keep"].float())
    d2 = torch.tensor([[0.2, 0.9, 0.9, 0.9]], device=cuda)    # a tie in d: choice 2
    assert H.td3v10_rank_mask(d2, c[:1])["keep"].tolist() == [[0, 1, 1, 0]]


# --------------------------------------------- actor loss backward through the heads ---
@pytest.mark.parametrize("A", AS)
def test_heads_backward_against_autograd_fp64(cuda, A):
    from rl_ctr_prediction_amd import hip_ops as H
    g = torch.Generator(device=cuda).manual_seed(1300 + A)
    T, reg = 0.1, 1e-2
    for B in BS:
        pre_c = torch.randn(B, A, device=cuda, generator=g)
        d_q = torch.randn(B, A, device=cuda, generator=g) * 0.3
        u = torch.rand(B, A, device=cuda, generator=g).clamp_(1e-7, 1 - 1e-7)
        D = 5
        G, _ = strided(cuda, B, D + 2 * A, D + 2 * A + 3, 1, gen=g)   # the critic input's gradient
        g_d, g_c = G[:, D:D + A], G[:, D + A:]
        h = H.td3v10_heads(H.V10_PLAIN, pre_c, d_q, uniform=u, temperature=T, want_softmax=False)
        keep = H.td3v10_rank_mask(h["d_action"], h["c_means"])["keep"]
        # fp64 autograd of the same graph, the mask and the softmax the kernel was given
        pc, dq = pre_c.double().requires_grad_(True), d_q.double().requires_grad_(True)
        cm = torch.tanh(pc)
        p = torch.softmax((dq + R.gumbel(u.double())) / T, dim=-1)
        c_m = torch.clamp(torch.where(keep.bool(), cm, torch.zeros_like(cm)), -1, 1)
        loss = (g_c.double() * c_m).sum() + (g_d.double() * p).sum() + \
            reg * ((cm ** 2).mean() + (dq ** 2).mean())
        loss.backward()
        a, b = H.td3v10_heads_backward(g_c, g_d, keep, h["c_means"], d_q, h["d_action"], T, reg)
        what = f"B={B} A={A}"
        close(a, pc.grad, what + " d pre_c")
        # d d_q = p (g - p.g) / T: the softmax's own bar, through the same factor
        z = (dq.detach() + R.gumbel(u.double())) / T
        extra = softmax_bar(z, p.detach()) * (2 * g_d.double().abs().max(1, keepdim=True)[0] / T)
        close(b, dq.grad, what + " d d_q", extra)
        a2, b2 = H.td3v10_heads_backward(g_c, g_d, keep, h["c_means"], d_q, h["d_action"], T, reg)
        assert torch.equal(a, a2) and torch.equal(b, b2)


# ------------------------------------------------------------- gradient clipping ------
def test_clip_grad_norm(cuda):
    from rl_ctr_prediction_amd import hip_ops as H
    g = torch.Generator(device=cuda).manual_seed(21)
    sizes = [1, 3, 5, 64, 65, 257, 1001, 120000, (12, 11)]   # none a multiple of a vector but 64
    base = [torch.randn(*(s if isinstance(s, tuple) else (s,)), device=cuda, generator=g)
            for s in sizes]
    base.append(torch.randn(1001, device=cuda, generator=g))
    n0 = float(torch.sqrt(sum((t.double() ** 2).sum() for t in base)))
    for name, target in (("below", 0.3), ("above", 7.0), ("far above", 3000.0)):
        grads = [(t * (target / n0)).contiguous() for t in base]
        buf = torch.full((1004,), 777.0, device=cuda)
        buf[1:1002] = grads[-1]
        grads[-1] = buf[1:1002]                              # 4 bytes off a 16-byte boundary
        ref = [t.double() for t in grads]
        norm64 = torch.sqrt(sum((t ** 2).sum() for t in ref))
        coef = torch.clamp(0.5 / (norm64 + 1e-6), max=1.0)
        keep = [t.clone() for t in grads]
        norm = H.clip_grad_norm_(grads, 0.5)
        print(f"clip {name}: norm {float(norm):.9g} vs fp64 {float(norm64):.9g}")
        close(norm.reshape(1), norm64.reshape(1), f"clip {name} norm")
        for i, (a, e) in enumerate(zip(grads, ref)):
            close(a, e * coef, f"clip {name} tensor {i}")
        if target < 0.5:
            assert all(torch.equal(a, k) for a, k in zip(grads, keep)), "a norm below: unchanged"
        again = [k.clone() for k in keep]
        norm2 = H.clip_grad_norm_(again, 0.5)
        assert torch.equal(norm, norm2) and all(torch.equal(a, b) for a, b in zip(grads, again))
        assert float(buf[0]) == 777.0 and bool((buf[1002:] == 777.0).all())
    # at the threshold: 0.3, 0.4 has norm 0.5, and torch's factor 0.5 / (0.5 + 1e-6) applies
    t = [torch.tensor([0.3], device=cuda), torch.tensor([0.4], device=cuda)]
    norm = H.clip_grad_norm_(t, 0.5)
    close(norm.reshape(1), [0.5], "norm at the threshold")
    close(torch.cat(t), np.array([0.3, 0.4]) * (0.5 / (0.5 + 1e-6)), "clip at the threshold")
    assert float(t[0]) < 0.3
    with pytest.raises(ValueError, match="outside"):
        H.clip_grad_norm_([torch.ones(1, device=cuda)] * 65, 0.5)


# ------------------------------------------------------------------ v10 memory --------
def test_memory_store_max_update_and_sample(cuda):
    from rl_ctr_prediction_amd import hip_ops as H
    from rl_ctr_prediction_amd.v10_hybrid_td3_model_per import Memory
    g = torch.Generator(device=cuda).manual_seed(31)
    N, T = 50, 7
    m = Memory(N, T, cuda)
    ref = R.RefMemory(N, T, cuda)

    def rows(n, reward_scale):
        t = torch.randn(n, T, device=cuda, generator=g)
        t[:, -1] = torch.rand(n, device=cuda, generator=g) * reward_scale
        return t

    t1 = rows(30, 0.5)
    m.add_seeded(t1)
    ref.store_transition(t1)
    assert bool((m.prioritys_[:30, 0] == 1).all()), "the seed is 1 on an empty memory"
    assert torch.equal(m.prioritys_[:30, 1], t1[:, -1]) and bool((m.prioritys_[30:] == 0).all())
    assert torch.equal(m.memory, ref.memory) and torch.equal(m.prioritys_, ref.prio)
    t2 = rows(10, 3.0)           # rewards above 1: the next max comes from the reward column
    m.add_seeded(t2)
    ref.store_transition(t2)
    t3 = rows(25, 0.5)           # wraps: rows 40..49 and 0..14 are overwritten
    wide = torch.full((25, T + 4), 777.0, device=cuda)
    wide[:, 2:T + 2] = t3
    m.add_seeded(wide[:, 2:T + 2])   # a row-strided view
    ref.store_transition(t3)
    seed = float(t2[:, -1].max())
    assert seed > 1 and bool((m.prioritys_[40:, 0] == seed).all()) and \
        bool((m.prioritys_[:15, 0] == seed).all()), "the max is taken over both columns"
    assert torch.equal(m.memory, ref.memory) and torch.equal(m.prioritys_, ref.prio)
    assert m.memory_counter == 65
    # add() overwrites both columns with what it is given (no max)
    td2 = torch.randn(12, 2, device=cuda, generator=g) * 0.01
    t4 = rows(12, 1.0)
    m.add(td2, t4)
    ref.add(td2, t4)
    assert torch.equal(m.memory, ref.memory) and torch.equal(m.prioritys_, ref.prio)
    assert torch.equal(m.prioritys_[15:27], td2)
    # batch_update: the raw signed error into column 0, column 1 untouched
    idx = torch.tensor([3, 49, 0, 17], device=cuda)
    td = torch.tensor([[-2.5], [0.125], [-0.0625], [4.0]], device=cuda)
    before = m.prioritys_.clone()
    m.batch_update(idx, td)
    assert torch.equal(m.prioritys_[idx, 0], td.view(-1))
    assert torch.equal(m.prioritys_[:, 1], before[:, 1])
    rest = torch.ones(N, dtype=torch.bool, device=cuda)
    rest[idx] = False
    assert torch.equal(m.prioritys_[rest], before[rest])
    ref.batch_update(idx, td)
    # the sample against a numpy evaluation of the seed's keys
    seed_s, k = 1234, 16
    idx_s, batch, isw = m.stochastic_sample(k, seed=seed_s)
    p = R.priority(ref.prio[:, 0].double())    # (|p0| + 1e-3)^0.6 of the (all filled) rows, fp64
    keys = H.td3v10_keys(m.prioritys_, N, m.epsilon, m.alpha, seed_s)
    # the keys are per_keys of the transformed priorities (log p + Gumbel of the seed) ...
    p32 = torch.pow(m.prioritys_[:, 0].abs() + 1e-3, 0.6)
    close(keys, H.per_keys(p32.contiguous(), N, H.PER_STOCHASTIC, seed_s).double(),
          "keys against per_keys of the priorities", 4e-7 * (1 + keys.double().abs()))
    # ... and the sample is their k largest, ties by index
    keys = keys.cpu().numpy()
    order = np.lexsort((np.arange(N), -keys))[:k]
    assert np.array_equal(idx_s.cpu().numpy(), order)
    assert torch.equal(batch, m.memory[idx_s])
    close(isw, (p[idx_s] / p.min()).pow(-1.0).view(-1, 1), "isw")
    prio_before = m.prioritys_.clone()
    assert m.beta == 1.0 and len(set(idx_s.tolist())) == k
    i2, b2, w2 = m.stochastic_sample(k, seed=seed_s)
    assert torch.equal(i2, idx_s) and torch.equal(w2, isw)
    assert torch.equal(m.prioritys_, prio_before), "sampling writes nothing to prioritys_"
    # a prioritys_ that is not 16-byte aligned takes the scalar loads: the same sample
    shifted = torch.empty(2 * N + 2, device=cuda)[2:].view(N, 2)
    shifted.copy_(m.prioritys_)
    assert shifted.data_ptr() % 16 == 8
    o = H.td3v10_sample(m.memory, shifted, N, k, seed_s, 1.0, m.epsilon, m.alpha)
    assert torch.equal(o["idx"], idx_s) and torch.equal(o["isw"], isw)
    # partially filled: only the filled rows are sampled
    m2 = Memory(64, T, cuda)
    m2.add_seeded(rows(20, 0.5))
    i3, _, _ = m2.stochastic_sample(20, seed=5)
    assert sorted(i3.tolist()) == list(range(20))
    with pytest.raises(ValueError, match="outside"):
        m2.stochastic_sample(21)
    with pytest.raises(NotImplementedError, match="ill-formed"):
        m2.greedy_sample(4)


def test_memory_max_over_a_large_memory(cuda):
    """More than one block of the max, and more partials than one wave."""
    from rl_ctr_prediction_amd import hip_ops as H
    N, T = 300001, 4
    mem, prio = torch.zeros(N, T, device=cuda), torch.zeros(N, 2, device=cuda)
    ws = torch.empty(4096, dtype=torch.uint8, device=cuda)
    seed = torch.zeros((), device=cuda)
    rows = torch.ones(3, T, device=cuda)
    for where in ((0, 0), (N - 1, 1), (123457, 1), (200000, 0)):
        prio.zero_()
        prio[:, 0] = -1.0          # negative errors elsewhere
        prio[where] = 2.5
        H.td3v10_store_seeded(mem, prio, 5, rows, ws, seed_out=seed)
        assert float(seed) == 2.5 and bool((prio[5:8, 0] == 2.5).all()), where
    prio.fill_(-3.0)               # a max that is neither 0 nor positive is taken as it is
    H.td3v10_store_seeded(mem, prio, N - 1, rows[:2], ws, seed_out=seed)
    assert float(seed) == -3.0 and float(prio[N - 1, 0]) == -3.0 and float(prio[0, 0]) == -3.0
    assert float(prio[0, 1]) == 1.0 and bool((mem[N - 1] == 1).all()) and bool((mem[0] == 1).all())


# ------------------------------------------- eval-mode BatchNorm parameter backward ----
@pytest.mark.parametrize("N", [1, 3, 39, 64, 65, 255])
def test_bn_eval_backward(cuda, N):
    from rl_ctr_prediction_amd import hip_ops as H
    g = torch.Generator(device=cuda).manual_seed(1700 + N)
    rm = torch.randn(N, device=cuda, generator=g)
    rv = torch.rand(N, device=cuda, generator=g) + 0.1
    for bi, B in enumerate(BS):
        lname, (pad, off) = list(LAYOUTS.items())[bi % len(LAYOUTS)]
        x, _ = strided(cuda, B, N, N + pad, off, gen=g, scale=2.0)
        dy, _ = strided(cuda, B, N, N + pad, off, gen=g)
        gam = torch.ones(N, device=cuda, dtype=torch.float64, requires_grad=True)
        bet = torch.zeros(N, device=cuda, dtype=torch.float64, requires_grad=True)
        y = (x.double() - rm.double()) / torch.sqrt(rv.double() + 1e-5) * gam + bet
        y.backward(dy.double())
        dg, db = H.bn_eval_backward(dy, x, rm, rv, 1e-5)
        cond = (dy.double().abs() * ((x.double() - rm.double()) /
                                     torch.sqrt(rv.double() + 1e-5)).abs()).sum(0)
        assert_grad_close(_np(dg), _np(gam.grad), cond=_np(cond), err_msg=f"B={B} N={N} {lname} dgamma")
        assert_grad_close(_np(db), _np(bet.grad), cond=_np(dy.double().abs().sum(0)),
                          err_msg=f"B={B} N={N} {lname} dbeta")
        dg2, db2 = H.bn_eval_backward(dy, x, rm, rv, 1e-5)
        assert torch.equal(dg, dg2) and torch.equal(db, db2)


def test_eval_mode_actor_takes_parameter_gradients_only(cuda):
    from rl_ctr_prediction_amd.v10_hybrid_td3_model_per import Hybrid_Actor
    from rl_ctr_prediction_amd.hybrid_td3_model_per import _BatchNorm1d
    torch.manual_seed(2)
    actor, ref = Hybrid_Actor(39, 3).to(cuda), R.RefActor(39, 3)
    ref.load_state_dict(actor.state_dict())
    ref = ref.to(cuda).double()
    s = torch.randn(16, 39, device=cuda)
    actor.train()
    ref.train()
    with torch.no_grad():                        # move the running statistics off (0, 1)
        actor._pre(s)
        ref.pre(s.double())
    actor.eval()
    ref.eval()
    gc, gd = torch.randn(16, 3, device=cuda), torch.randn(16, 3, device=cuda)
    pc, pd = actor._pre(s)
    grads = torch.autograd.grad([pc, pd], list(actor.parameters()), [gc, gd])
    rc, rd = ref.pre(s.double())
    want = torch.autograd.grad([rc, rd], list(ref.parameters()), [gc.double(), gd.double()])
    for (n, _), a, e in zip(actor.named_parameters(), grads, want):
        close(a, e, f"eval-mode actor gradient {n}")
    with pytest.raises(RuntimeError, match="no backward"):   # the states carry no gradient
        actor._pre(s.clone().requires_grad_(True))
    base = _BatchNorm1d(39).to(cuda).eval()      # the base agent's BatchNorm still refuses
    with pytest.raises(RuntimeError, match="no backward"):
        base(s)


# --------------------------------------------------------------------- the agent ------
@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def make_agent(gold, dev):
    from rl_ctr_prediction_amd import Feature_Embedding
    from rl_ctr_prediction_amd import v10_hybrid_td3_model_per as M
    V, F, K, A, B, MEM, _, DL, TB = (int(v) for v in gold["shapes"])
    agent = M.Hybrid_TD3_Model(V, field_nums=F, latent_dims=K, action_nums=A, memory_size=MEM,
                               batch_size=B, data_len=DL, train_batch_size=TB, device=dev)
    fe = Feature_Embedding(V, F, K).to(dev)
    fe.feature_embedding.weight.data.copy_(torch.from_numpy(gold["emb"]))
    return agent, fe


def recorded(gold, i, dev):
    t = f"c{i}"
    sample = tuple(torch.from_numpy(gold[f"{t}/{k}"]).to(dev) for k in ("idx", "batch", "isw"))
    noise = {k: torch.from_numpy(gold[f"{t}/{k}"]).to(dev)
             for k in ("n_d", "n_c", "u", "u_actor") if f"{t}/{k}" in gold}
    return sample, noise


def act_store(agent, fe, gold, tag, rows, random, dev):
    """One choose_action on the recorded draws and the store of its transitions."""
    ids = torch.from_numpy(gold["ids"]).to(dev)[rows]
    rew = torch.from_numpy(gold["rewards"]).to(dev)[rows]
    names = ("r_c", "r_d") if random else ("n_c", "n_d", "u")
    noise = tuple(torch.from_numpy(gold[f"{tag}/{k}"]).to(dev) for k in names)
    with torch.no_grad():
        s = fe(ids)
    c, sm, d, ix = agent.choose_action(s, random, noise=noise)
    assert agent.Hybrid_Actor.training == (not random)
    agent.store_transition(torch.cat([ids.float(), c, d, ix.float(), rew], dim=1))
    return c, sm, d, ix


def best(agent, fe, gold, dev):
    with torch.no_grad():
        s5 = fe(torch.from_numpy(gold["states5"]).to(dev))
    out = agent.choose_best_action(s5, noise=torch.from_numpy(gold["best/u"]).to(dev))
    assert not agent.Hybrid_Actor.training
    return out


def test_teacher_forced_step_parity(cuda, gold):
    """Twenty consecutive learns, each started from the HIP agent's own state copied into
    td3_v10_ref in fp64 (parameters, buffers, modes, Adam state), on the recorded samples and
    draws. td3_v10_ref continues from the HIP path's stepped critic parameters, which are
    themselves checked against Adam applied in fp64 to the HIP path's own clipped gradients.
    The 10th learn updates the actor in training mode, the 20th in eval mode."""
    V, F, K, A, B, MEM, _, DL, TB = (int(v) for v in gold["shapes"])
    D = F * (F - 1) // 2 + F * K
    agent, fe = make_agent(gold, cuda)
    act_store(agent, fe, gold, "ra", slice(0, 40), True, cuda)
    act_store(agent, fe, gold, "na", slice(40, 80), False, cuda)
    emb64 = fe.feature_embedding.weight.detach().double()
    ref = R.RefTD3v10(D, F, A, dtype=torch.float64, device=cuda, data_len=DL, train_batch_size=TB)
    worst = {}

    def note(k, a, d, extra=None):
        a, d = _np(a), _np(d)
        bar = grad_bound(d) + (0 if extra is None else _np(extra))
        worst[k] = max(worst.get(k, 0.0), float(np.max(np.abs(a - d) / bar)))

    for i in range(20):
        if i == 10:
            best(agent, fe, gold, cuda)
        ref.load_from(agent)
        before = {n: {k: _np(v) for k, v in getattr(agent, n).state_dict().items()}
                  for n in ref.nets()}
        adam = {}
        for tag, opt, net in (("c", agent.optimizer_c, agent.Hybrid_Critic),
                              ("a", agent.optimizer_a, agent.Hybrid_Actor)):
            for n, p in net.named_parameters():
                st = opt.state.get(p)
                adam[tag, n] = (_np(st["exp_avg"]), _np(st["exp_avg_sq"]), int(st["step"])) \
                    if st else (0.0, 0.0, 0)
        sample, noise = recorded(gold, i, cuda)
        loss = agent.learn(fe, sample=sample, noise=noise)

        def force_stepped_critic():
            with torch.no_grad():
                for pr, p in zip(ref.Hybrid_Critic.parameters(), agent.Hybrid_Critic.parameters()):
                    pr.copy_(p.double())

        o = ref.learn(lambda ids: R.embed_state(emb64, ids), sample=sample, noise=noise,
                      after_critic_step=force_stepped_critic)
        what = f"learn {i}"
        for k in ("q1", "q2", "q_target", "td"):
            note(k, agent.last[k], o[k])
            close(agent.last[k], o[k], f"{what} {k}")
        note("loss", np.float64(loss), o["loss"])
        close(np.array([loss]), o["loss"].reshape(1), what + " loss")
        note("gnorm_c", agent.last["grad_norm_c"].reshape(1), o["gnorm_c"].reshape(1))
        close(agent.last["grad_norm_c"].reshape(1), o["gnorm_c"].reshape(1), what + " gnorm_c")
        actor_step = (i + 1) % 10 == 0
        assert ("ga" in o) == actor_step and agent.Hybrid_Actor.training == (i < 10)
        if actor_step:
            note("gnorm_a", agent.last["grad_norm_a"].reshape(1), o["gnorm_a"].reshape(1))
            close(agent.last["grad_norm_a"].reshape(1), o["gnorm_a"].reshape(1), what + " gnorm_a")
        for tag, net, lr in (("gc", agent.Hybrid_Critic, agent.lr_C),
                             ("ga", agent.Hybrid_Actor, agent.lr_C_A)):
            if tag == "ga" and not actor_step:
                for n, t in net.state_dict().items():  # untouched by this learn, buffers too
                    assert np.array_equal(_np(t), before["Hybrid_Actor"][n]), n
                continue
            netname = "Hybrid_Critic" if tag == "gc" else "Hybrid_Actor"
            for n, p in net.named_parameters():
                note(tag, p.grad, o[tag][n])
                close(p.grad, o[tag][n], f"{what} {tag}/{n}")
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
        for n, src in (("Hybrid_Critic_", "Hybrid_Critic"), ("Hybrid_Actor_", "Hybrid_Actor")):
            now = dict(getattr(agent, src).named_parameters())
            for k, p in getattr(agent, n).named_parameters():
                want = before[n][k]
                if actor_step:
                    want = want * (1.0 - agent.tau) + _np(now[k]) * agent.tau
                np.testing.assert_allclose(_np(p), want, rtol=1e-6, atol=1e-6 if actor_step else 0,
                                           err_msg=f"{what} {n}.{k} after the soft update")
        idx = sample[0]
        assert torch.equal(agent.memory.prioritys_[idx, 0], agent.last["td"].view(-1))
    print("teacher-forced: worst error / bar:", {k: round(v, 4) for k, v in worst.items()})
    assert agent.learn_iter == 20 and agent.Hybrid_Critic_.training and agent.Hybrid_Actor_.training
    assert int(agent.Hybrid_Critic.bn_input.num_batches_tracked) == 22  # twice on actor steps


@pytest.fixture(scope="module")
def free_run(cuda, gold):
    """The fixture's whole script on the HIP agent, once: rows of (what, call, reference gap,
    HIP distance to the fp64 record, distance / bar, within the bar) and the discrete outputs."""
    agent, fe = make_agent(gold, cuda)
    rows, discrete = [], {}

    def judge(what, call, got, key):
        f32, f64 = gold[key], gold["f64/" + key]
        got, f32, f64 = (np.asarray(a, dtype=np.float64).reshape(np.shape(f64))
                         for a in (got, f32, f64))
        gap = float(np.max(np.abs(f32 - f64))) if f64.size else 0.0
        dist = float(np.max(np.abs(got - f64))) if f64.size else 0.0
        bar = np.maximum(10.0 * gap, grad_bound(f64))
        frac = float(np.max(np.abs(got - f64) / bar)) if f64.size else 0.0
        rows.append((what, call, gap, dist, frac, frac <= 1.0))

    def packed(prefix, call, named):
        """Vectors and small matrices in full, large matrices by their recorded strided sample."""
        for k, t in named:
            a, key = _np(t), f"{prefix}/{k}"
            if key not in gold:
                a, key = a[::37, ::11], key + "@s"
            judge(key.split("/", 1)[1], call, a, key)

    def action(tag, r, random):
        c, sm, d, ix = act_store(agent, fe, gold, tag, r, random, cuda)
        for k, v in (("c", c), ("softmax", sm), ("d", d)):
            judge(f"{tag}/{k}", tag, _np(v), f"{tag}/{k}")
        discrete[tag] = (ix.cpu().numpy(), gold[f"{tag}/index"])
        judge(f"{tag}/prio", tag, _np(agent.memory.prioritys_), f"{tag}/prio")
        judge(f"{tag}/memory", tag, _np(agent.memory.memory), f"{tag}/memory")

    def learns(lo, hi):
        for i in range(lo, hi):
            sample, noise = recorded(gold, i, cuda)
            loss = agent.learn(fe, sample=sample, noise=noise)
            t = f"c{i}"
            for k in ("q1", "q2", "q_target", "td"):
                judge(f"{t}/{k}", i, _np(agent.last[k]), f"{t}/{k}")
            judge(f"{t}/loss", i, [loss], f"{t}/loss")
            judge(f"{t}/gnorm_c", i, [float(agent.last["grad_norm_c"])], f"{t}/gnorm_c")
            packed(f"{t}/gc", i, [(n, p.grad) for n, p in agent.Hybrid_Critic.named_parameters()])
            if (i + 1) % 10 == 0:
                judge(f"{t}/gnorm_a", i, [float(agent.last["grad_norm_a"])], f"{t}/gnorm_a")
                packed(f"{t}/ga", i, [(n, p.grad) for n, p in agent.Hybrid_Actor.named_parameters()])
            for n in R.NETS:
                packed(f"{t}/{n}", i, list(getattr(agent, n).state_dict().items()))
            judge(f"{t}/prio", i, _np(agent.memory.prioritys_), f"{t}/prio")
            assert gold[f"{t}/temperature"] == agent.temprature

    action("ra", slice(0, 40), True)
    action("na", slice(40, 80), False)
    learns(0, 10)
    bix, bcm, bsm = best(agent, fe, gold, cuda)
    discrete["best"] = (bix.cpu().numpy(), gold["best/index"])
    judge("best/c_means", "best", _np(bcm), "best/c_means")
    judge("best/softmax", "best", _np(bsm), "best/softmax")
    learns(10, 20)
    assert not agent.Hybrid_Actor.training
    action("nb", slice(80, 120), False)
    return rows, discrete


def _report(rows, title):
    print(f"{title}: quantity, reference fp32-vs-fp64 gap, HIP distance to fp64, distance / bar")
    for what, call, gap, dist, frac, ok in rows:
        if not what.startswith(("gc/", "ga/", "Hybrid_")) or frac > 0.5:
            print(f"  {what:52s} {gap:10.3g} {dist:10.3g} {frac:8.3g}")
    print(f"  {len(rows)} entries, largest gap {max(r[2] for r in rows):.3g}, largest HIP "
          f"distance {max(r[3] for r in rows):.3g}, largest distance / bar "
          f"{max(r[4] for r in rows):.3g}")


def test_free_running_parity_with_the_reference_record(free_run):
    """Calls 0..18 and the three action calls: per quantity the bar is 10 x the reference's own
    fp32-vs-fp64 distance, never less than the kernel bar; discrete outputs are equal."""
    rows, discrete = free_run
    mine = [r for r in rows if r[1] != 19]
    _report(mine, "free-running parity")
    for tag, (got, want) in discrete.items():
        assert np.array_equal(got, want), f"{tag}: discrete actions differ"
    assert all(r[5] for r in mine), [r[:5] for r in mine if not r[5]]


def test_eval_mode_actor_update_matches_the_record(free_run):
    """The 20th learn updates the actor with bn_input in eval mode (after choose_best_action):
    its gradients, states and priorities within the same bar. The test of the eval-mode
    BatchNorm parameter backward inside the agent."""
    rows, _ = free_run
    mine = [r for r in rows if r[1] == 19]
    assert any(r[0].startswith("c19/ga/bn_input") or r[0].startswith("ga/bn_input")
               for r in mine), [r[0] for r in mine][:8]
    _report(mine, "eval-mode actor update (call 19)")
    assert all(r[5] for r in mine), [r[:5] for r in mine if not r[5]]


def test_learn_and_store_make_no_host_synchronisation(cuda, gold):
    agent, fe = make_agent(gold, cuda)
    act_store(agent, fe, gold, "ra", slice(0, 40), True, cuda)
    act_store(agent, fe, gold, "na", slice(40, 80), False, cuda)
    trans = agent.memory.memory[:40].clone()
    for _ in range(10):  # warm-up, the actor update and both soft updates included
        agent.learn(fe, return_tensor=True)
    agent.store_transition(trans)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [agent.learn(fe, return_tensor=True) for _ in range(10)]
        agent.store_transition(trans)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert agent.learn_iter == 20 and agent.memory.memory_counter == 160
    assert all(l.is_cuda and l.dim() == 0 and bool(torch.isfinite(l)) for l in losses)
    assert isinstance(agent.learn(fe), float)


def test_temperature_anneals_on_the_host(cuda, gold):
    """The 999th call lowers the temperature by (T - T_min) * 999 / (data_len //
    train_batch_size), not below T_min; no other call moves it."""
    agent, fe = make_agent(gold, cuda)
    act_store(agent, fe, gold, "ra", slice(0, 40), True, cuda)
    agent.data_len, agent.train_batch_size = 80000, 40      # 2000 batches a pass
    agent.learn_iter = 997
    agent.learn(fe, return_tensor=True)
    assert agent.temprature == 1.0
    agent.learn(fe, return_tensor=True)
    assert agent.learn_iter == 999 and agent.temprature == 1.0 - (1.0 - 0.1) * 999 / 2000
    agent.learn(fe, return_tensor=True)
    assert agent.temprature == 1.0 - (1.0 - 0.1) * 999 / 2000
    agent.data_len, agent.learn_iter = 80, 1998             # 2 batches: the floor holds
    agent.learn(fe, return_tensor=True)
    assert agent.temprature == 0.1


def test_seeded_free_runs_are_bitwise_equal(cuda, gold):
    def run():
        agent, fe = make_agent(gold, cuda)
        ids = torch.from_numpy(gold["ids"]).to(cuda)
        rew = torch.from_numpy(gold["rewards"]).to(cuda)
        torch.manual_seed(3)
        outs = []
        with torch.no_grad():
            s = fe(ids[:80])
        for random, r in ((True, slice(0, 40)), (False, slice(40, 80))):
            c, sm, d, ix = agent.choose_action(s[r], random)
            outs += [c, sm, d, ix]
            agent.store_transition(torch.cat([ids[r].float(), c, d, ix.float(), rew[r]], dim=1))
        losses = [agent.learn(fe, return_tensor=True) for _ in range(10)]
        outs += list(agent.choose_best_action(s[:5]))
        losses += [agent.learn(fe, return_tensor=True) for _ in range(10)]
        state = [v.clone() for n in R.NETS for v in getattr(agent, n).state_dict().values()]
        return torch.stack(losses), state + outs + [agent.memory.prioritys_.clone(),
                                                    agent.memory.memory.clone()]
    l1, s1 = run()
    l2, s2 = run()
    assert torch.equal(l1, l2) and len(s1) == len(s2)
    assert all(torch.equal(a, b) for a, b in zip(s1, s2))
    assert float(l1.std()) > 0  # the learns differ from one another: samples and noise move


def test_state_dict_round_trip(cuda, gold):
    from rl_ctr_prediction_amd.v10_hybrid_td3_model_per import Hybrid_Actor, Hybrid_Critic
    V, F, K, A, B, MEM, _, DL, TB = (int(v) for v in gold["shapes"])
    D = F * (F - 1) // 2 + F * K
    g = torch.Generator().manual_seed(4)
    for mine, theirs in ((Hybrid_Critic(D, A), R.RefCritic(D, A)),
                         (Hybrid_Actor(D, A), R.RefActor(D, A))):
        assert list(mine.state_dict()) == [str(k) for k in gold[f"keys/{type(mine).__name__}"]]
        sd = theirs.state_dict()  # a checkpoint with the reference's keys
        for k, v in sd.items():
            if v.is_floating_point():
                v.copy_((torch.rand(v.shape, generator=g) - 0.5) * (0.2 if v.dim() == 2 else 1.0)
                        + (1.0 if "running_var" in k else 0.0))
            else:
                v.fill_(7)
        mine.load_state_dict(sd, strict=True)
        mine.to(cuda)
        theirs.to(cuda)
        back = mine.state_dict()
        assert list(back) == list(sd) and all(torch.equal(back[k].cpu(), sd[k].cpu()) for k in sd)
        s = torch.randn(B, D, device=cuda)
        with torch.no_grad():
            if isinstance(mine, Hybrid_Critic):
                c, d = torch.rand(B, A, device=cuda), torch.rand(B, A, device=cuda)
                got = mine.evaluate(s, c, d)
                want = theirs.double().evaluate(s.double(), c.double(), d.double())
            else:
                got = mine.evaluate(s)
                rc, rd = theirs.double().pre(s.double())
                want = (torch.tanh(rc), rd)
        for a, b in zip(got, want):
            close(a, b, type(mine).__name__ + " after load_state_dict")
        assert int(mine.bn_input.num_batches_tracked) == 8
