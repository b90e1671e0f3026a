"""Time the hybrid TD3 agent (hybrid_td3_model_per.Hybrid_TD3_Model over csrc/td3.hip and the
GEMMs) at the RL driver's shape: F = 15 fields, K = 10, A = 6 actions (input_dims 255,
transitions of 29 floats), batch 256, a memory of 1,000,000 transitions, full.

    python tools/td3_bench.py [--iters 60] [--inner 8] [--memory 1000000] [--states 4096]

Operations: learn(return_tensor=True) (every 4th call includes the actor update and both soft
updates, so `inner` is a multiple of 4 and a figure is the mean over such a group) and
choose_action on `states` states.
Baseline on the same GPU: tests/td3_ref.RefTD3 in fp32, the same agent from stock torch ops
(nn.Linear, nn.BatchNorm1d, torch.randn_like, torch.optim.Adam, a Python loop for the soft
update, `.item()` on the loss; built with instrument=False, so none of the parity tests'
recording runs), sampling from its own copy of the same HIP replay memory and
encoding states with the same Feature_Embedding: what differs is the agent, not its inputs.
`learn_no_item` is the baseline without the `.item()`.

Each of the `iters` rounds times every variant once, in turn (device events around `inner`
back-to-back calls), after a warm-up; the figure is the median over the rounds, with the 10th
and 90th percentiles. One JSON line is printed and appended to profiles/td3_bench.jsonl.

Launch counts: run the tool under `rocprofv3 --kernel-trace --stats` twice,
    ... -- python tools/td3_bench.py --trace hip --learns 8     (then --learns 16)
and give the two kernel_stats.csv files to
    python tools/td3_bench.py --summarise A_kernel_stats.csv B_kernel_stats.csv --learns-diff 8
which prints launches and device time per learn (the difference of the two runs: the set-up
cancels). No GPU: an error, no fallback.
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

V, F, K, A, B = 100000, 15, 10, 6, 256


def build(dev, memory, which):
    from rl_ctr_prediction_amd import Feature_Embedding, Hybrid_TD3_Model
    from rl_ctr_prediction_amd.replay_memory import Memory
    import td3_ref
    torch.manual_seed(0)
    fe = Feature_Embedding(V, F, K).to(dev)
    g = torch.Generator().manual_seed(1)
    T = F + 2 * A + 2

    def fill(mem):
        for s in range(0, memory, 1 << 17):
            n = min(1 << 17, memory - s)
            tr = torch.cat([torch.randint(0, V, (n, F), generator=g).float(),
                            torch.rand(n, 2 * A, generator=g) * 2 - 1,
                            torch.randint(1, A + 1, (n, 1), generator=g).float(),
                            torch.rand(n, 1, generator=g)], dim=1).to(dev)
            mem.add(torch.randn(n, 1, generator=g).to(dev), tr)

    out = {}
    if which in ("hip", "both"):
        agent = Hybrid_TD3_Model(V, field_nums=F, latent_dims=K, action_nums=A,
                                 memory_size=memory, batch_size=B, device=dev)
        fill(agent.memory)
        out["hip"] = agent
    if which in ("ref", "both"):
        D = F * (F - 1) // 2 + F * K
        mem = Memory(memory, T, dev)
        fill(mem)
        out["ref"] = td3_ref.RefTD3(D, F, A, device=dev, memory=mem, batch_size=B,
                                    instrument=False)  # the bare agent: no test recording
    return fe, out


def bench(a, dev):
    fe, ag = build(dev, a.memory, "both")
    hip, ref = ag["hip"], ag["ref"]
    ids = torch.randint(0, V, (a.states, F), device=dev)
    with torch.no_grad():
        s = fe(ids)

    def ref_choose():
        c, d = torch.empty(a.states, A, device=dev), torch.empty(a.states, A, device=dev)
        return ref.choose_action(s, (torch.randn_like(c), torch.randn_like(d)))

    variants = {
        "learn": (lambda: hip.learn(fe, return_tensor=True), a.inner),
        "ref_learn": (lambda: float(ref.learn(fe)["loss"]), a.inner),
        "ref_learn_no_item": (lambda: ref.learn(fe), a.inner),
        "choose_action": (lambda: hip.choose_action(s), a.inner),
        "ref_choose_action": (ref_choose, a.inner),
    }
    times = {name: [] for name in variants}
    for it in range(a.warmup + a.iters):
        for name, (fn, inner) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / inner)
    us = {name: statistics.median(v) for name, v in times.items()}
    return dict(tool="td3_bench", device=torch.cuda.get_device_name(0), F=F, K=K, A=A, batch=B,
                memory=a.memory, states=a.states, iters=a.iters, inner=a.inner,
                us={n: round(v, 1) for n, v in us.items()},
                us_p10_p90={n: [round(sorted(v)[len(v) // 10], 1),
                                round(sorted(v)[(9 * len(v)) // 10], 1)] for n, v in times.items()},
                speedup=dict(learn=round(us["ref_learn"] / us["learn"], 2),
                             learn_vs_no_item=round(us["ref_learn_no_item"] / us["learn"], 2),
                             choose_action=round(us["ref_choose_action"] / us["choose_action"], 2)))


def trace(a, dev):
    fe, ag = build(dev, min(a.memory, 100000), a.trace)
    agent = ag[a.trace]
    for _ in range(a.learns):
        agent.learn(fe, return_tensor=True) if a.trace == "hip" else agent.learn(fe)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="td3_bench", trace=a.trace, learns=a.learns)))


def summarise(a):
    def load(p):
        return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"]))
                for r in csv.DictReader(open(p))}
    x, y = load(a.summarise[0]), load(a.summarise[1])
    rows = []
    for name, (calls, ns) in y.items():
        c0, n0 = x.get(name, (0, 0.0))
        if calls != c0:
            rows.append(((calls - c0) / a.learns_diff, (ns - n0) / a.learns_diff / 1e3,
                         name.replace("void ", "").split("(")[0][:90]))
    rows.sort(key=lambda r: -r[1])
    total = sum(r[0] for r in rows)
    busy = sum(r[1] for r in rows)
    print(json.dumps(dict(tool="td3_bench", launches_per_learn=round(total, 2),
                          device_us_per_learn=round(busy, 1), kernels=len(rows))))
    for c, u, n in rows[:a.top]:
        print(f"{c:8.2f} launches {u:9.2f} us  {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--memory", type=int, default=1000000)
    ap.add_argument("--states", type=int, default=4096)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "td3_bench.jsonl"))
    ap.add_argument("--trace", choices=["hip", "ref"])
    ap.add_argument("--learns", type=int, default=8)
    ap.add_argument("--summarise", nargs=2)
    ap.add_argument("--learns-diff", type=int, default=8)
    ap.add_argument("--top", type=int, default=25)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a)
    if a.inner % 4:
        raise SystemExit("td3_bench: --inner must be a multiple of 4 (the actor update's period)")
    if not torch.cuda.is_available():
        raise SystemExit("td3_bench: no ROCm device (a timing needs the GPU; no fallback)")
    dev = torch.device("cuda:0")
    if a.trace:
        return trace(a, dev)
    line = json.dumps(bench(a, dev))
    print(line, flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
