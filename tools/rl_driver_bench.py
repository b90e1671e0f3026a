"""Time one batch of the hybrid TD3 ensemble driver's train loop
(rl_ctr_prediction_amd.hybrid_td3_main_per.train) at the RL driver's shape: F = 15 fields,
K = 10, M = 3 frozen models (LR, FM, FFM) = 3 actions, batch 4096, a memory of 1,000,000
transitions (full), the agent's learn on 256 samples, after tools/td3_bench.py.

    python tools/rl_driver_bench.py [--iters 30] [--batches 8] [--memory 1000000]

One batch = state encoding, choose_action, the three model forwards, the ensemble kernel, the
store, one learn, the metrics. Three comparisons, each variant timed once per round in turn
after a warm-up, the figure the median over the rounds with the 10th and 90th percentiles:
  device    train(metrics="device"): DeviceMetrics.add, store_step, learn(return_tensor=True);
            the epoch waits for the device once, in compute()
  composed  the same loop composed from what the package had before this driver: the two casts,
            torch.cat, store_transition (ones + Memory.add), .tolist() twice and .item() twice
            per batch, sklearn's AUC at the end (the reference's loop, and train(metrics="host")
            minus the fused ensemble entry point: it calls ctr_ensemble_preds with c_actions =
            prob_weights). The models, the agent and the data are the same objects' twins.
  store     Memory.add_step alone against casts + cat + ones + Memory.add alone.
The two epochs are timed with a host clock from a device synchronise to the end of the call
(both end in a wait: compute() / the last .item()), over `batches` batches (a multiple of 4: the
actor update's period), and divided by `batches`; the two stores with device events around
`batches` calls. Host waits per batch are counted with torch's sync debug mode in "warn"
(compute()'s one read is the device epoch's only one). One JSON line is printed and appended to
profiles/rl_driver_bench.jsonl.

Launch counts: run the tool under `rocprofv3 --kernel-trace --stats` twice per path,
    ... -- python tools/rl_driver_bench.py --trace device --batches 8     (then --batches 16)
and give the two kernel_stats.csv files to
    python tools/rl_driver_bench.py --summarise A_kernel_stats.csv B_kernel_stats.csv \
        --batches-diff 8 --path device
which prints (and appends) launches and device time per batch (the difference of the two runs:
the set-up cancels). No GPU: an error, no fallback.
"""
from __future__ import annotations

import argparse
import csv
import json
import statistics
import sys
import time
import warnings
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

V, F, K, M, B = 100000, 15, 10, 3, 4096


def build(dev, memory, n_batches):
    from rl_ctr_prediction_amd import FFM, FM, LR, Feature_Embedding
    from rl_ctr_prediction_amd import hybrid_td3_main_per as D
    torch.manual_seed(0)
    models = [LR(V), FM(V, K), FFM(V, F, K)]
    with torch.no_grad():
        for m in models:
            for n, p in m.named_parameters():
                if n != "bias":
                    p.mul_(0.1)
    fe = Feature_Embedding(V, F, K).to(dev)
    fe.load_embedding(models[1].state_dict())
    model_dict = {i: m.to(dev).eval() for i, m in enumerate(models)}
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, V, (n_batches * B, F), generator=g).to(dev)
    y = (torch.rand(n_batches * B, generator=g) < 0.3).float().to(dev)
    T = F + 2 * M + 2

    def agent():
        torch.manual_seed(2)
        a = D.get_model(M, V, F, K, 1e-3, 1e-3, B, memory, dev, "")
        gg = torch.Generator().manual_seed(3)
        for s in range(0, memory, 1 << 17):
            n = min(1 << 17, memory - s)
            tr = torch.cat([torch.randint(0, V, (n, F), generator=gg).float(),
                            torch.rand(n, 2 * M, generator=gg) * 2 - 1,
                            torch.randint(1, M + 1, (n, 1), generator=gg).float(),
                            (torch.rand(n, 1, generator=gg) < 0.5).float()], dim=1).to(dev)
            a.memory.add(torch.randn(n, 1, generator=gg).to(dev), tr)
        assert a.memory.transition_lens == T
        return a

    loader = D.DeviceBatches.__new__(D.DeviceBatches)  # over the generated, device-resident data
    loader.x, loader.y, loader.batch_size = x, y, B
    return D, model_dict, fe, agent, loader, (x, y)


def composed_epoch(D, agent, model_dict, fe, data):
    """The train loop composed from the parts the package had before the driver."""
    from sklearn.metrics import roc_auc_score
    from rl_ctr_prediction_amd import hip_ops
    x, yf = data
    yi = yf.long().view(-1, 1)
    targets, predicts = [], []
    total_rewards, loss, n = 0.0, 0.0, 0
    for s in range(0, x.shape[0], B):
        features, labels = x[s:s + B], yi[s:s + B]
        state = fe.forward(features)
        c_actions, prob_weights, d_values, d_actions = agent.choose_action(state)
        with torch.no_grad():
            preds = torch.cat([model_dict[i](features).detach().reshape(-1, 1)
                               for i in range(len(model_dict))], dim=1)
        y_preds, rewards, _ = hip_ops.ensemble_preds(preds, d_actions, prob_weights, prob_weights,
                                                     labels)
        targets.extend(labels.tolist())
        predicts.extend(y_preds.tolist())
        transitions = torch.cat([features.float(), c_actions, d_values, d_actions.float(), rewards],
                                dim=1)
        agent.store_transition(transitions)
        loss = agent.learn(fe)
        total_rewards += torch.sum(rewards, dim=0).item()
        n += 1
    return loss, total_rewards / n, roc_auc_score(targets, predicts), n


def count_waits(fn):
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    return sum("synchroniz" in str(i.message).lower() for i in w)


def bench(a, dev):
    D, model_dict, fe, make_agent, loader, data = build(dev, a.memory, a.batches)
    new, old = make_agent(), make_agent()
    epochs = {
        "device": lambda: D.train(new, model_dict, loader, fe, 1.0, dev, metrics="device"),
        "composed": lambda: composed_epoch(D, old, model_dict, fe, data),
    }
    x, yf = data
    state = fe.forward(x[:B])
    c, pw, d, act = new.choose_action(state)
    r = (torch.rand(B, 1, device=dev) < 0.5).float()
    feats = x[:B]
    stores = {
        "store_step": lambda: new.memory.add_step(feats, c, d, act, r),
        "store_composed": lambda: old.store_transition(
            torch.cat([feats.float(), c, d, act.float(), r], dim=1)),
    }
    times = {k: [] for k in list(epochs) + list(stores)}
    for it in range(a.warmup + a.iters):
        for name, fn in epochs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e6 / a.batches)
        for name, fn in stores.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.batches):
                fn()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.batches)
    waits = {name: count_waits(fn) for name, fn in epochs.items()}
    us = {k: statistics.median(v) for k, v in times.items()}
    return dict(tool="rl_driver_bench", device=torch.cuda.get_device_name(0), F=F, K=K, M=M,
                batch=B, learn_batch=256, memory=a.memory, batches=a.batches, iters=a.iters,
                us_per_batch={k: round(v, 1) for k, v in us.items()},
                us_p10_p90={k: [round(sorted(v)[len(v) // 10], 1),
                                round(sorted(v)[(9 * len(v)) // 10], 1)] for k, v in times.items()},
                host_waits_per_epoch=waits,
                host_waits_per_batch={k: round(v / a.batches, 2) for k, v in waits.items()},
                speedup=dict(batch=round(us["composed"] / us["device"], 3),
                             store=round(us["store_composed"] / us["store_step"], 3)))


def trace(a, dev):
    D, model_dict, fe, make_agent, loader, data = build(dev, min(a.memory, 100000), a.batches)
    agent = make_agent()
    if a.trace == "device":
        D.train(agent, model_dict, loader, fe, 1.0, dev, metrics="device")
    else:
        composed_epoch(D, agent, model_dict, fe, data)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="rl_driver_bench", trace=a.trace, batches=a.batches)))


def summarise(a):
    def load(p):
        return {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"]))
                for r in csv.DictReader(open(p))}
    x, y = load(a.summarise[0]), load(a.summarise[1])
    rows = []
    for name, (calls, ns) in y.items():
        c0, n0 = x.get(name, (0, 0.0))
        if calls != c0:
            rows.append(((calls - c0) / a.batches_diff, (ns - n0) / a.batches_diff / 1e3,
                         name.replace("void ", "").split("(")[0][:90]))
    rows.sort(key=lambda r: -r[1])
    line = json.dumps(dict(tool="rl_driver_bench", path=a.path,
                           launches_per_batch=round(sum(r[0] for r in rows), 2),
                           device_us_per_batch=round(sum(r[1] for r in rows), 1),
                           kernels=len(rows)))
    print(line)
    for c, u, n in rows[:a.top]:
        print(f"{c:8.2f} launches {u:9.2f} us  {n}")
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--memory", type=int, default=1000000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rl_driver_bench.jsonl"))
    ap.add_argument("--trace", choices=["device", "composed"])
    ap.add_argument("--summarise", nargs=2)
    ap.add_argument("--batches-diff", type=int, default=8)
    ap.add_argument("--path", default="device")
    ap.add_argument("--top", type=int, default=25)
    a = ap.parse_args()
    if a.summarise:
        line = summarise(a)
    else:
        if a.batches % 4:
            raise SystemExit("rl_driver_bench: --batches must be a multiple of 4 (the actor "
                             "update's period)")
        if not torch.cuda.is_available():
            raise SystemExit("rl_driver_bench: no ROCm device (a timing needs the GPU; no fallback)")
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
