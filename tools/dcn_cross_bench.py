"""Time DCN's cross network at the C3 shape (B=8192, D=1664, L=5): the fused HIP forward
(z only) and backward (rank-1 form) against the same maths composed from torch ops on the
same GPU (the per-layer matmul / mul / add of the reference's forward, autograd backward).

    python tools/dcn_cross_bench.py [--iters 200] [--inner 4] [--B 8192] [--D 1664] [--L 5]

Each of the `iters` rounds times every variant once, in turn (device events around `inner`
back-to-back calls), after a warm-up; the figure is the median over the rounds. Bytes are the
algorithmic ones (forward: x0 read once; backward: x0 read and dx0 written once; plus s, z / gz
and the parameters), the share is of the 8 TB/s HBM peak. `bwd_blocks<N>` repeats the backward
with at most N partial slabs (CTR_DCN_BLOCKS), the reduction design's one knob. One JSON line
is printed and appended to profiles/dcn_cross_bench.jsonl. No GPU: an error, no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from rl_ctr_prediction_amd import hip_ops as H  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--inner", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--D", type=int, default=1664)
    ap.add_argument("--L", type=int, default=5)
    ap.add_argument("--blocks", type=int, nargs="*", default=[128, 64])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dcn_cross_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dcn_cross_bench: no ROCm device (a timing needs the GPU; no fallback)")
    dev = torch.device("cuda:0")
    B, D, L = a.B, a.D, a.L
    g = torch.Generator().manual_seed(0)
    r = D ** -0.5
    x0 = (torch.randn(B, D, generator=g) * 0.1).to(dev)
    W = ((torch.rand(L, D, generator=g) * 2 - 1) * r).to(dev)
    b = (torch.randn(L, D, generator=g) * 0.05).to(dev)
    wt = ((torch.rand(D, generator=g) * 2 - 1) * r).to(dev)
    gz = (torch.randn(B, generator=g) / B).to(dev)

    fo = H.dcn_cross_forward(x0, W, b, wt, want_xl=False)
    bo = H.dcn_cross_backward(x0, W, b, fo["s"], gz=gz, w_tail=wt)

    # the composed version: leaves that require grad, the reference's per-layer ops
    xr = x0.clone().requires_grad_(True)
    Ws = [W[i:i + 1].clone().requires_grad_(True) for i in range(L)]
    bs = [b[i].clone().requires_grad_(True) for i in range(L)]
    wr = wt.clone().requires_grad_(True)
    leaves = [xr, *Ws, *bs, wr]

    def composed_forward():
        x = xr
        for i in range(L):
            xw = torch.matmul(x, Ws[i].t())
            x = xr * xw + bs[i] + x
        return torch.matmul(x, wr)

    zc = composed_forward()
    gc = torch.autograd.grad(zc, leaves, gz, retain_graph=True)
    agree = dict(z=float((zc.detach() - fo["z"]).abs().max()),
                 dx0=float((gc[0] - bo["dx0"]).abs().max()),
                 dW=float((torch.cat(gc[1:1 + L]) - bo["dW"]).abs().max()),
                 dw_tail=float((gc[-1] - bo["dw_tail"]).abs().max()))

    def bwd_with(cap):
        def run():
            if cap:
                os.environ["CTR_DCN_BLOCKS"] = str(cap)
            H.dcn_cross_backward(x0, W, b, fo["s"], gz=gz, w_tail=wt, out=bo)
            os.environ.pop("CTR_DCN_BLOCKS", None)
        return run

    def composed_fwd_nograd():
        with torch.no_grad():
            composed_forward()

    variants = {
        "fused_fwd": lambda: H.dcn_cross_forward(x0, W, b, wt, out=fo),
        "fused_bwd": bwd_with(0),
        "composed_fwd": composed_fwd_nograd,
        "composed_bwd": lambda: torch.autograd.grad(zc, leaves, gz, retain_graph=True),
    }
    for cap in a.blocks:
        variants[f"fused_bwd_blocks{cap}"] = bwd_with(cap)
    times = {k: [] for k in variants}
    for it in range(a.warmup + a.iters):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    us = {k: statistics.median(v) for k, v in times.items()}
    par = (2 * L * D + D) * 4
    nbytes = {"fused_fwd": B * D * 4 + B * L * 4 + B * 4 + par,
              "fused_bwd": 2 * B * D * 4 + B * L * 4 + B * 4 + 2 * par}
    res = dict(tool="dcn_cross_bench", device=torch.cuda.get_device_name(0), B=B, D=D, L=L,
               iters=a.iters, inner=a.inner,
               us={k: round(v, 2) for k, v in us.items()},
               us_p10_p90={k: [round(sorted(v)[len(v) // 10], 2), round(sorted(v)[(9 * len(v)) // 10], 2)]
                           for k, v in times.items()},
               algorithmic_bytes=nbytes,
               gbytes_per_s={k: round(nbytes[k] / us[k] / 1e3, 1) for k in nbytes},
               hbm_peak_share={k: round(nbytes[k] / (us[k] * 1e-6) / HBM_PEAK, 3) for k in nbytes},
               speedup_vs_composed=dict(fwd=round(us["composed_fwd"] / us["fused_fwd"], 2),
                                        bwd=round(us["composed_bwd"] / us["fused_bwd"], 2)),
               max_abs_diff_vs_composed=agree)
    line = json.dumps(res)
    print(line)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
