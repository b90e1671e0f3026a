"""Time the evaluation metrics of an epoch: DeviceMetrics (csrc/metrics.hip) against the
drivers' host path, on synthetic predictions at N = 1,000,000 and 4,096,000 in batches of 4096.

    python tools/metrics_bench.py [--N 1000000 4096000] [--batch 4096] [--iters 5] [--host-iters 2]

device: reset + one add() per batch + compute() (its single state-block read included), HIP
        events around the whole sequence, after a warm-up; also the add loop and compute()
        apart (compute() by a host clock around its device-to-host read).
host:   what pretrain_main._predict does with the same predictions: per batch one BCELoss
        .item() and two .tolist() into Python lists, then sklearn.metrics.roc_auc_score; a host
        clock around the loop, which ends in host reads of every batch.
The model's forward is in neither side. Both AUCs are compared (abs 1e-12) before any figure is
reported. One JSON line per N is printed and appended to profiles/metrics_bench.jsonl; run it at
least twice and quote the range. No GPU: an error, no fallback.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rl_ctr_prediction_amd.metrics import DeviceMetrics  # noqa: E402


def bench_shape(a, dev, N):
    from sklearn.metrics import roc_auc_score
    g = torch.Generator().manual_seed(N)
    y = (torch.rand(N, generator=g) < 0.2).float()
    # predictions correlated with the labels, strictly inside (0, 1)
    p = torch.sigmoid(torch.randn(N, generator=g) + 1.5 * y - 1.5).clamp(1e-6, 1 - 1e-6)
    p, y = p.to(dev).view(-1, 1), y.to(dev)
    bounds = [(s, min(s + a.batch, N)) for s in range(0, N, a.batch)]
    m = DeviceMetrics(N, dev)

    def device_adds():
        m.reset()
        for s, e in bounds:
            m.add(p[s:e], y[s:e])

    total, adds, comp, res = [], [], [], None
    for it in range(a.warmup + a.iters):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        torch.cuda.synchronize()
        e0.record()
        device_adds()
        e1.record()
        t0 = time.perf_counter()
        res = m.compute()
        t1 = time.perf_counter()
        e2.record()
        e2.synchronize()
        if it >= a.warmup:
            total.append(e0.elapsed_time(e2))
            adds.append(e0.elapsed_time(e1))
            comp.append((t1 - t0) * 1e3)  # includes waiting for the adds still in flight

    loss = torch.nn.BCELoss()
    host, host_auc, host_loss = [], None, None
    for it in range(1 + a.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        targets, predicts, tot = [], [], 0.0
        for s, e in bounds:
            yy, lab = p[s:e], y[s:e]
            tot += loss(yy, lab.view(-1, 1)).item()
            targets.extend(lab.view(-1, 1).tolist())
            predicts.extend(yy.tolist())
        host_auc = roc_auc_score(targets, predicts)
        host_loss = tot / len(bounds)
        if it:
            host.append((time.perf_counter() - t0) * 1e3)
    if abs(host_auc - res["auc"]) > 1e-12 or abs(host_loss - res["loss"]) > 1e-5 * host_loss:
        raise SystemExit(f"metrics_bench: device {res} disagrees with host auc {host_auc!r} "
                         f"loss {host_loss!r}")
    dev_ms, host_ms = statistics.median(total), statistics.median(host)
    return dict(tool="metrics_bench", device=torch.cuda.get_device_name(0), N=N, batch=a.batch,
                batches=len(bounds), iters=a.iters, host_iters=a.host_iters,
                device_ms=round(dev_ms, 3), device_ms_min_max=[round(min(total), 3),
                                                               round(max(total), 3)],
                device_add_loop_ms=round(statistics.median(adds), 3),
                device_compute_host_clock_ms=round(statistics.median(comp), 3),
                host_ms=round(host_ms, 1), host_ms_min_max=[round(min(host), 1),
                                                            round(max(host), 1)],
                host_over_device=round(host_ms / dev_ms, 1), auc=res["auc"],
                auc_abs_diff=abs(host_auc - res["auc"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="*", default=[1000000, 4096000])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "metrics_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench: no ROCm device (a timing needs the GPU; no fallback)")
    dev = torch.device("cuda:0")
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for N in a.N:
        line = json.dumps(bench_shape(a, dev, N))
        print(line, flush=True)
        with out.open("a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
