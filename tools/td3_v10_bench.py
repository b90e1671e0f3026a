"""Time the v10 hybrid TD3 agent (v10_hybrid_td3_model_per.Hybrid_TD3_Model over
csrc/td3_v10.hip, csrc/td3.hip and the GEMMs) at the RL driver's shape: F = 15 fields, K = 10,
A = 6 actions (input_dims 255, transitions of 29 floats), batch 256, a memory of 1,000,000
transitions, full.

    python tools/td3_v10_bench.py [--iters 40] [--inner 8] [--memory 1000000] [--rows 4096]

Operations: learn(return_tensor=True) without the actor update (policy_freq out of reach),
learn with the actor update and both soft updates in every call (policy_freq = 1), and
store_transition of `rows` rows.
Baselines on the same GPU, all fp32: tests/td3_v10_ref.RefTD3v10 (instrument=False), the same
agent from stock torch ops (nn.Linear, nn.BatchNorm1d, torch.randn / torch.rand draws,
torch.optim.Adam, clip_grad_norm_, a Python loop for the soft update, `.item()` on the loss),
sampling from its own copy of the same HIP replay memory and encoding states with the same
Feature_Embedding: what differs is the agent, not its inputs. `ref_*` uses the vectorised rank
mask, `loops_*` the mask written as A^2 grouped passes with nonzero() (the shape of the
original implementation, several host waits per call). store_transition's baseline is
td3_v10_ref.RefMemory (torch.max, where, cat and index assignments on the device).

Each of the `iters` rounds times every variant once, in turn (device events around `inner`
back-to-back calls), after a warm-up; the figure is the median over the rounds, with the 10th
and 90th percentiles. One JSON line is printed and appended to profiles/td3_v10_bench.jsonl.

Launch counts: run the tool under `rocprofv3 --kernel-trace --stats` twice,
    ... -- python tools/td3_v10_bench.py --trace hip --learns 10     (then --learns 20)
and give the two kernel_stats.csv files to
    python tools/td3_v10_bench.py --summarise A_kernel_stats.csv B_kernel_stats.csv \
        --learns-diff 10 --label hip
which prints launches and device time per learn (the difference of the two runs: the set-up
cancels; ten learns hold one actor update) and, with --label, appends that line to the jsonl.
No GPU: an error, no fallback.
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
T = F + 2 * A + 2


def transitions(n, g, dev):
    return torch.cat([torch.randint(0, V, (n, F), generator=g).float(),
                      torch.rand(n, 2 * A, generator=g) * 2 - 1,
                      torch.randint(1, A + 1, (n, 1), generator=g).float(),
                      torch.rand(n, 1, generator=g)], dim=1).to(dev)


def fill(mem, memory, g, dev):
    for s in range(0, memory, 1 << 17):
        n = min(1 << 17, memory - s)
        mem.add(torch.randn(n, 2, generator=g).to(dev) * 0.1, transitions(n, g, dev))


class RefAgent:
    """RefTD3v10 with the sampling and the draws a learn needs."""

    def __init__(self, dev, memory, g, loops):
        import td3_v10_ref as R
        from rl_ctr_prediction_amd.v10_hybrid_td3_model_per import Memory
        D = F * (F - 1) // 2 + F * K
        self.mem = Memory(memory, T, dev)
        fill(self.mem, memory, g, dev)
        mask = (lambda d, c, n: (R.rank_mask_group_loops(d, c, n), None)) if loops else None
        self.ref = R.RefTD3v10(D, F, A, device=dev, memory=self.mem, rank_mask=mask,
                               instrument=False)
        self.dev = dev

    def learn(self, fe, item=True):
        sample = self.mem.stochastic_sample(B)
        noise = dict(n_d=torch.randn(B, A, device=self.dev), n_c=torch.randn(B, A, device=self.dev),
                     u=torch.rand(B, A, device=self.dev), u_actor=torch.rand(B, A, device=self.dev))
        loss = self.ref.learn(fe, sample=sample, noise=noise)["loss"]
        return loss.item() if item else loss


def build(dev, memory, which):
    from rl_ctr_prediction_amd import Feature_Embedding
    from rl_ctr_prediction_amd import v10_hybrid_td3_model_per as M
    torch.manual_seed(0)
    fe = Feature_Embedding(V, F, K).to(dev)
    g = torch.Generator().manual_seed(1)
    out = {}
    if "hip" in which:
        agent = M.Hybrid_TD3_Model(V, field_nums=F, latent_dims=K, action_nums=A,
                                   memory_size=memory, batch_size=B, device=dev)
        fill(agent.memory, memory, g, dev)
        out["hip"] = agent
    if "ref" in which:
        out["ref"] = RefAgent(dev, memory, g, False)
    if "loops" in which:
        out["loops"] = RefAgent(dev, memory, g, True)
    return fe, out


def bench(a, dev):
    import td3_v10_ref as R
    fe, ag = build(dev, a.memory, ("hip", "ref", "loops"))
    hip, ref, loops = ag["hip"], ag["ref"], ag["loops"]
    g = torch.Generator().manual_seed(2)
    rows = transitions(a.rows, g, dev)
    refmem = R.RefMemory(a.memory, T, dev)
    refmem.prio.copy_(hip.memory.prioritys_)

    def freq(n):
        hip.policy_freq = ref.ref.policy_freq = loops.ref.policy_freq = n

    def learn(agent_learn, n):
        def run():
            freq(n)
            return agent_learn()
        return run

    never = 1 << 40
    variants = {
        "learn": (learn(lambda: hip.learn(fe, return_tensor=True), never), a.inner),
        "ref_learn": (learn(lambda: ref.learn(fe), never), a.inner),
        "ref_learn_no_item": (learn(lambda: ref.learn(fe, item=False), never), a.inner),
        "loops_learn": (learn(lambda: loops.learn(fe), never), a.inner),
        "learn_actor": (learn(lambda: hip.learn(fe, return_tensor=True), 1), a.inner),
        "ref_learn_actor": (learn(lambda: ref.learn(fe), 1), a.inner),
        "loops_learn_actor": (learn(lambda: loops.learn(fe), 1), a.inner),
        "store": (lambda: hip.store_transition(rows), a.inner),
        "ref_store": (lambda: refmem.store_transition(rows), a.inner),
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
    ratio = lambda x, y: round(us[x] / us[y], 2)  # noqa: E731
    return dict(tool="td3_v10_bench", device=torch.cuda.get_device_name(0), F=F, K=K, A=A, batch=B,
                memory=a.memory, rows=a.rows, iters=a.iters, inner=a.inner,
                us={n: round(v, 1) for n, v in us.items()},
                us_p10_p90={n: [round(sorted(v)[len(v) // 10], 1),
                                round(sorted(v)[(9 * len(v)) // 10], 1)] for n, v in times.items()},
                speedup=dict(learn=ratio("ref_learn", "learn"),
                             learn_vs_no_item=ratio("ref_learn_no_item", "learn"),
                             learn_vs_loops=ratio("loops_learn", "learn"),
                             learn_actor=ratio("ref_learn_actor", "learn_actor"),
                             learn_actor_vs_loops=ratio("loops_learn_actor", "learn_actor"),
                             store=ratio("ref_store", "store")))


def trace(a, dev):
    fe, ag = build(dev, min(a.memory, 100000), (a.trace,))
    agent = ag[a.trace]
    for _ in range(a.learns):
        agent.learn(fe, return_tensor=True) if a.trace == "hip" else agent.learn(fe)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="td3_v10_bench", trace=a.trace, learns=a.learns)))


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
    line = json.dumps(dict(tool="td3_v10_bench", summary=a.label, learns_diff=a.learns_diff,
                           launches_per_learn=round(total, 2),
                           device_us_per_learn=round(busy, 1), kernels=len(rows)))
    print(line)
    if a.label:  # kept beside the timings: the traces themselves are not
        with Path(a.out).open("a") as f:
            f.write(line + "\n")
    for c, u, n in rows[:a.top]:
        print(f"{c:8.2f} launches {u:9.2f} us  {n}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--memory", type=int, default=1000000)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "td3_v10_bench.jsonl"))
    ap.add_argument("--trace", choices=["hip", "ref", "loops"])
    ap.add_argument("--learns", type=int, default=10)
    ap.add_argument("--summarise", nargs=2)
    ap.add_argument("--learns-diff", type=int, default=10)
    ap.add_argument("--top", type=int, default=25)
    ap.add_argument("--label", help="with --summarise: append the summary line to --out as this")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a)
    if not torch.cuda.is_available():
        raise SystemExit("td3_v10_bench: no ROCm device (a timing needs the GPU; no fallback)")
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
