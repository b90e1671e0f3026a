"""Time the OPNN input / gradient kernels and the fused OPNN step at the C3 shape (F=26, K=64,
B=8192, a table of >= 1M rows):

    python tools/opnn_bench.py [--V 2000000] [--B 8192] [--F 26] [--K 64] [--steps 20]
                               [--ids criteo|uniform]

  * ctr_opnn_forward as the fused step calls it (planes + sum_e, no fp32 copy) and
    ctr_opnn_backward, alone: us per launch and achieved bytes/s from the shape-derived byte
    counts below (not measured traffic), as a share of the 8 TB/s HBM peak;
      forward:  ids + B*F*K*4 row bytes read, 6 bytes per valid plane element and B*K*4 written
      backward: B*W*4 + B*K*4 read, B*F*K*4 written                       (W = F*K + K)
  * the fused OPNN step (FusedCTRTrainer) alternating, in this same call, with the fused IPNN
    step of the same build on the same batches: us per step and examples/s;
  * the same OuterPNN stepped by AutogradTrainer (the reference's step through autograd).

Every region is timed with device events after a warm-up and is taken twice (`runs`), the
variants in turn. The kernels alone cycle over `--rotate` sets of their dense operands and
outputs (more than the 256 MiB Infinity Cache holds), so no launch reads what the one before
left in cache; the table rows a batch names more than once are still cache hits, as in a step. Batches: `--batches` different id sets, cycled: `--ids criteo` (the default)
draws them like bench.py does (rl_ctr_prediction_amd.synthetic.CriteoSynth: skewed per-field
vocabularies, ~1/3 as many unique rows per batch), `--ids uniform` uniformly over the table
(every slot its own row, nearly: the scatter's and the Adam apply's worst case). One JSON line
is printed and appended to profiles/opnn_bench.jsonl. No GPU: an error, no fallback.
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
    ap.add_argument("--steps", type=int, default=20, help="fused steps per region")
    ap.add_argument("--autograd_steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "opnn_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("opnn_bench: no ROCm device (a timing needs the GPU; no fallback)")
    dev = torch.device("cuda:0")
    V, B, F, K = a.V, a.B, a.F, a.K
    W = F * K + K
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
    nb = a.batches

    # ---------------------------------------------------------------- the kernels alone
    E = (torch.randn(V, K, generator=g) * 0.05).to(dev)
    ksum = torch.full((K,), float(K), device=dev)
    # every launch works on the next of `--rotate` buffer sets, so that a launch does not find
    # its operands in the 256 MiB Infinity Cache from the launch before (in the fused step dcat
    # comes from the dX GEMM and dslot goes to the scatter): 6 sets are 0.5 GB of planes for the
    # forward and 0.68 GB of dcat + dslot for the backward
    nr = a.rotate
    planes = [H.Planes(B, W, dev, ones_col=True) for _ in range(nr)]
    sum_e = [torch.empty(B, K, device=dev) for _ in range(nr)]
    dcat = [torch.randn(B, W, device=dev) for _ in range(nr)]
    dslot = [torch.empty(B * F, K, device=dev) for _ in range(nr)]
    for j in range(nr):  # the backward's field sums are real ones
        H.opnn_forward(xs[j % nb], E, ksum, planes=planes[j], sum_e=sum_e[j])
    kern = {
        "opnn_forward": lambda i: H.opnn_forward(xs[i % nb], E, ksum, planes=planes[i % nr],
                                                 sum_e=sum_e[i % nr]),
        "opnn_backward": lambda i: H.opnn_backward(sum_e[i % nr], ksum, dcat[i % nr], F,
                                                   out=dslot[i % nr]),
    }
    kbytes = {"opnn_forward": B * F * xs[0].element_size() + B * F * K * 4 + B * W * 6 + B * K * 4,
              "opnn_backward": B * W * 4 + B * K * 4 + B * F * K * 4}
    kern_runs = {k: [] for k in kern}
    for _ in range(a.runs):
        times = {k: [] for k in kern}
        for it in range(a.warmup + a.iters):
            for name, fn in kern.items():
                t = _region(lambda j, fn=fn, it=it: fn(it * a.inner + j), a.inner)
                if it >= a.warmup:
                    times[name].append(t)
        for k, v in times.items():
            kern_runs[k].append(statistics.median(v))
    del E, planes, dcat, dslot

    # ------------------------------------------- the fused steps, OPNN beside IPNN
    def model(kind):
        torch.manual_seed(0)
        with torch.device(dev):
            m = P.OuterPNN(V, F, K) if kind == "OPNN" else P.InnerPNN(V, F, K)
        with torch.no_grad():
            m.feature_embedding.weight.mul_(0.05)
        return m

    trainers = {kind: P.FusedCTRTrainer(model(kind), lr=1e-3, weight_decay=1e-5, seed=1)
                for kind in ("OPNN", "IPNN")}

    def fused(tr):
        def step(i):
            nxt = [xs[(i + 1) % nb], xs[(i + 2) % nb]]
            tr.step(xs[i % nb], ys[i % nb], next_x=nxt, return_loss=False,
                    next_y=[ys[(i + 1) % nb], ys[(i + 2) % nb]])
        return step

    step_runs = {k: [] for k in trainers}
    for kind, tr in trainers.items():  # eager first steps, graph captures, the lookahead ring
        _region(fused(tr), 3 * nb)
    for _ in range(a.runs):
        for kind, tr in trainers.items():
            step_runs[kind].append(_region(fused(tr), a.steps))
    for tr in trainers.values():
        tr.flush()
        tr.check_errors()
    del trainers

    # ------------------------------------------- the same model through autograd
    at = AutogradTrainer(model("OPNN"), 1e-3, 1e-5)
    auto = lambda i: at.step(xs[i % nb], ys[i % nb])  # noqa: E731
    _region(auto, 2)
    auto_runs = [_region(auto, a.autograd_steps) for _ in range(a.runs)]

    r2 = lambda v: [round(t, 2) for t in v]  # noqa: E731
    best = {k: min(v) for k, v in kern_runs.items()}
    res = dict(tool="opnn_bench", device=torch.cuda.get_device_name(0), V=V, B=B, F=F, K=K, W=W,
               batches=nb, rotate=nr, ids=a.ids, unique_rows_per_batch=unique_rows, runs=a.runs,
               kernel_us=dict((k, r2(v)) for k, v in kern_runs.items()),
               kernel_model_bytes=kbytes,
               kernel_gbytes_per_s={k: [round(kbytes[k] / t / 1e3, 1) for t in v]
                                    for k, v in kern_runs.items()},
               kernel_hbm_peak_share={k: round(kbytes[k] / (best[k] * 1e-6) / HBM_PEAK, 3)
                                      for k in kern_runs},
               fused_step_us=dict((k, r2(v)) for k, v in step_runs.items()),
               fused_examples_per_s={k: [round(B / (t * 1e-6)) for t in v]
                                     for k, v in step_runs.items()},
               opnn_over_ipnn_step=round(min(step_runs["OPNN"]) / min(step_runs["IPNN"]), 3),
               autograd_step_us=r2(auto_runs),
               fused_speedup_vs_autograd=round(min(auto_runs) / min(step_runs["OPNN"]), 1))
    line = json.dumps(res)
    print(line)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
