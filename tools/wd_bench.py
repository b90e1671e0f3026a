"""Time the W&D input kernel, its scatter and the fused W&D step beside their DeepFM counterparts
(the form of tools/opnn_bench.py):

    python tools/wd_bench.py [--V 2000000] [--B 8192] [--F 26] [--K 64] [--steps 200]
                             [--ids criteo|uniform]
    python tools/wd_bench.py --F 15 --K 10 --B 4096        # the drivers' default latent_dims

  * ctr_wd_forward as the fused step calls it (planes + z_lin, no fp32 copy) against DeepFM's
    input at the same shape: ctr_fm_forward_planes where it exists (K % 4 == 0, (K/4) | 64,
    F <= 64), else the pair the DeepFM step runs (ctr_fm_forward writing the fp32 copy, then
    ctr_split_planes). us per launch (pair: per pair), and for the W&D kernel the achieved bytes/s
    from the shape-derived byte count below (not measured traffic) as a share of the 8 TB/s HBM
    peak:   ids + B*F*K*4 row bytes + B*F*4 weight bytes read, 6 bytes per plane element and
    B*4 written;
  * the scatter with the fused deferred-Adam apply, ctr_wd_embedding_grad_adam against
    ctr_fm_embedding_grad_adam, on the same plans and tables — where the fused apply exists
    (K % 4 == 0); else the sums alone, ctr_wd_embedding_grad against ctr_fm_embedding_grad;
  * the fused W&D step (FusedCTRTrainer) alternating, in this same call, with the fused DeepFM
    step of the same build on the same batches: us per step and examples/s. `--step_kinds`
    names the trainers of the call in build order; two trainers in one process share the
    process's few hardware queues between their streams, so `--step_kinds W&D --steps_only` and
    `--step_kinds DeepFM --steps_only`, run in turn, give each kind a process of its own;
  * the same WideAndDeep stepped by AutogradTrainer (the reference's step through autograd).

Every region is timed with device events after a warm-up and is taken `--runs` times, the
variants in turn and the first of each pair alternating (the second finds what the first left
in the Infinity Cache). The kernels alone cycle over `--rotate` sets of their dense operands and
outputs (more than the 256 MiB Infinity Cache holds at the large shape), so no launch reads what
the one before left in cache; the table rows a batch names more than once are still cache hits,
as in a step. Batches: `--batches` different id sets, cycled: `--ids criteo` (the default) draws
them like bench.py does, `--ids uniform` uniformly over the table. One JSON line is printed and
appended to profiles/wd_bench.jsonl. No GPU: an error, no fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import rl_ctr_prediction_amd as P  # noqa: E402
from rl_ctr_prediction_amd import hip_ops as H  # noqa: E402
from rl_ctr_prediction_amd.pretrain_main import AutogradTrainer  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (spec)


def _region(fn, n):
    """us per call of n back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, default=2_000_000)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--F", type=int, default=26)
    ap.add_argument("--K", type=int, default=64)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--ids", default="criteo", choices=["criteo", "uniform"])
    ap.add_argument("--rotate", type=int, default=6, help="buffer sets the kernel launches cycle")
    ap.add_argument("--iters", type=int, default=50, help="kernel rounds per run")
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200, help="fused steps per region")
    ap.add_argument("--autograd_steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--step_kinds", default="W&D,DeepFM",
                    help="the fused trainers of this call, in build order: W&D,DeepFM | "
                         "DeepFM,W&D | W&D | DeepFM (one kind: a process of its own)")
    ap.add_argument("--steps_only", action="store_true", help="only the fused steps")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wd_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wd_bench: no ROCm device (a timing needs the GPU; no fallback)")
    dev = torch.device("cuda:0")
    V, B, F, K = a.V, a.B, a.F, a.K
    W, S = F * K, B * F
    g = torch.Generator().manual_seed(0)
    if a.ids == "uniform":
        xs = [torch.randint(0, V, (B, F), generator=g).to(dev) for _ in range(a.batches)]
        ys = [(torch.rand(B, generator=g) < 0.3).float().to(dev) for _ in range(a.batches)]
    else:
        from rl_ctr_prediction_amd.synthetic import CriteoSynth
        host = list(CriteoSynth(V, F, seed=11).batches(a.batches, B))
        xs = [torch.tensor(x, device=dev) for x, _ in host]
        ys = [torch.tensor(y, device=dev).float() for _, y in host]
    unique_rows = [int(torch.unique(x).numel()) for x in xs]
    nb, nr = a.batches, a.rotate

    kern_runs, in_bytes, deepfm_input, scatter = {}, 0, None, None
    if not a.steps_only:
        # ---------------------------------------------------------------- the kernels alone
        E = (torch.randn(V, K, generator=g) * 0.05).to(dev)
        lin = (torch.randn(V, 1, generator=g) * 0.05).to(dev)
        bias = torch.zeros(1, device=dev)
        planes = [H.Planes(B, W, dev, ones_col=True) for _ in range(nr)]
        z = [torch.empty(B, device=dev) for _ in range(nr)]
        sum_e = [torch.empty(B, K, device=dev) for _ in range(nr)]
        planes_ok = H.fm_forward_planes_ok(K, F)
        if planes_ok:
            deepfm_input = "fm_forward_planes"

            def fm_in(i):
                H.fm_forward_planes(xs[i % nb], E, lin, bias, planes[i % nr], z[i % nr], sum_e[i % nr])
        else:
            deepfm_input = "fm_forward+split_planes"
            fmo = [H.FMForward(z=z[j], sum_e=sum_e[j], emb_out=torch.empty(B, W, device=dev), p=None,
                               loss_elem=None, gz=None) for j in range(nr)]

            def fm_in(i):
                r = H.fm_forward(xs[i % nb], E, lin, bias, want_sum=True, want_emb=True, want_p=False,
                                 out=fmo[i % nr])
                H.split_planes(r.emb_out, out=planes[i % nr])

        def wd_in(i):
            H.wd_forward(xs[i % nb], E, lin, bias, out=None, planes=planes[i % nr], z_lin=z[i % nr])

        # the scatter: one plan per batch, gz / dX per buffer set (in a step dX comes from the dX
        # GEMM), real field sums for the DeepFM mode, one set of tables for both variants
        plans = [H.SparsePlanBuffers(S, dev).build(x, V) for x in xs]
        gz = [1e-3 * torch.randn(B, device=dev) for _ in range(nr)]
        dx = [1e-4 * torch.randn(B, W, device=dev) for _ in range(nr)]
        for j in range(nr):
            fm_in(j)  # sum_e[j] = batch j % nb's field sums
        grad_rows = torch.empty(S, K, device=dev)
        grad_lin = torch.empty(S, device=dev)
        fused_apply = K % 4 == 0 and K <= 256
        if fused_apply:
            scatter = "embedding_grad_adam"
            table = (E.clone(), torch.zeros(V, K, device=dev), torch.zeros(V, K, device=dev),
                     lin.view(-1).clone(), torch.zeros(V, device=dev), torch.zeros(V, device=dev),
                     torch.zeros(V, dtype=torch.int32, device=dev))
            tab = H.AdamStepTable(1e-3, (0.9, 0.999), dev)
            sdev = torch.ones(1, dtype=torch.int32, device=dev)
            kw = dict(step_dev=sdev, step_table=tab, step=1, weight_decay=1e-5, grad_rows=grad_rows,
                      grad_lin=grad_lin)

            def wd_sc(i):
                H.wd_embedding_grad_adam(plans[i % nb], F, gz[i % nr], dx[i % nr], table, **kw)

            def fm_sc(i):  # sum_e[j] belongs to batch j % nb: nr is a multiple of nb or the sums
                H.fm_embedding_grad_adam(plans[i % nb], F, gz[i % nr], sum_e[i % nr], dx[i % nr],
                                         table, **kw)  # are another batch's (timing only)
        else:
            scatter = "embedding_grad"

            def wd_sc(i):
                H.wd_embedding_grad(plans[i % nb], F, K, gz[i % nr], dx[i % nr], grad_rows=grad_rows,
                                    grad_lin=grad_lin)

            def fm_sc(i):
                H.fm_embedding_grad(plans[i % nb], F, E, gz[i % nr], sum_e[i % nr], dx[i % nr],
                                    grad_rows=grad_rows, grad_lin=grad_lin)

        kern = {"wd_forward": wd_in, deepfm_input: fm_in, "wd_" + scatter: wd_sc, "fm_" + scatter: fm_sc}
        in_bytes = B * F * xs[0].element_size() + B * W * 4 + B * F * 4 + B * W * 6 + B * 4
        kern_runs = {k: [] for k in kern}
        for _ in range(a.runs):
            times = {k: [] for k in kern}
            for it in range(a.warmup + a.iters):
                # each pair in both orders, round about: the second of a pair finds what the first
                # left in the Infinity Cache (the scatters share their tables' rows)
                names = list(kern)
                if it % 2:
                    names = [names[1], names[0], names[3], names[2]]
                for name in names:
                    fn = kern[name]
                    t = _region(lambda j, fn=fn, it=it: fn(it * a.inner + j), a.inner)
                    if it >= a.warmup:
                        times[name].append(t)
            for k, v in times.items():
                kern_runs[k].append(statistics.median(v))
        del E, planes, dx, plans, grad_rows, grad_lin
        if fused_apply:
            del table
        else:
            del fmo

    # ------------------------------------------- the fused steps, W&D beside DeepFM
    def model(kind):
        torch.manual_seed(0)
        with torch.device(dev):
            m = P.WideAndDeep(V, F, K) if kind == "W&D" else P.DeepFM(V, F, K)
        with torch.no_grad():
            (m.embedding if kind == "W&D" else m.feature_embedding).weight.mul_(0.05)
            m.linear.weight.mul_(0.05)
        return m

    trainers = {kind: P.FusedCTRTrainer(model(kind), lr=1e-3, weight_decay=1e-5, seed=1)
                for kind in a.step_kinds.split(",")}

    def fused(tr):
        def step(i):
            nxt = [xs[(i + 1) % nb], xs[(i + 2) % nb]]
            tr.step(xs[i % nb], ys[i % nb], next_x=nxt, return_loss=False,
                    next_y=[ys[(i + 1) % nb], ys[(i + 2) % nb]])
        return step

    step_runs = {k: [] for k in trainers}
    for kind, tr in trainers.items():  # eager first steps, graph captures, the lookahead ring
        _region(fused(tr), 3 * nb)
    for r in range(a.runs):  # the two kinds in turn, the first of a run alternating
        for kind in (list(trainers) if r % 2 == 0 else list(trainers)[::-1]):
            step_runs[kind].append(_region(fused(trainers[kind]), a.steps))
    for tr in trainers.values():
        tr.flush()
        tr.check_errors()
    del trainers

    # ------------------------------------------- the same model through autograd
    auto_runs = []
    if not a.steps_only:
        at = AutogradTrainer(model("W&D"), 1e-3, 1e-5)
        auto = lambda i: at.step(xs[i % nb], ys[i % nb])  # noqa: E731
        _region(auto, 2)
        auto_runs = [_region(auto, a.autograd_steps) for _ in range(a.runs)]

    r2 = lambda v: [round(t, 2) for t in v]  # noqa: E731
    res = dict(tool="wd_bench", device=torch.cuda.get_device_name(0), V=V, B=B, F=F, K=K, W=W,
               batches=nb, rotate=nr, ids=a.ids, unique_rows_per_batch=unique_rows, runs=a.runs,
               step_kinds=a.step_kinds.split(","),
               fused_step_us=dict((k, r2(v)) for k, v in step_runs.items()),
               fused_examples_per_s={k: [round(B / (t * 1e-6)) for t in v]
                                     for k, v in step_runs.items()})
    if len(step_runs) == 2:
        res["wd_over_deepfm_step"] = round(min(step_runs["W&D"]) / min(step_runs["DeepFM"]), 3)
    if not a.steps_only:
        best = {k: min(v) for k, v in kern_runs.items()}
        res.update(
            deepfm_input=deepfm_input, scatter=scatter,
            kernel_us=dict((k, r2(v)) for k, v in kern_runs.items()),
            wd_forward_model_bytes=in_bytes,
            wd_forward_gbytes_per_s=[round(in_bytes / t / 1e3, 1) for t in kern_runs["wd_forward"]],
            wd_forward_hbm_peak_share=round(in_bytes / (best["wd_forward"] * 1e-6) / HBM_PEAK, 3),
            wd_over_deepfm_input=round(best["wd_forward"] / best[deepfm_input], 3),
            wd_over_deepfm_scatter=round(best["wd_" + scatter] / best["fm_" + scatter], 3),
            autograd_step_us=r2(auto_runs))
        if "W&D" in step_runs:
            res["fused_speedup_vs_autograd"] = round(min(auto_runs) / min(step_runs["W&D"]), 1)
    line = json.dumps(res)
    print(line)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
