"""Capture the WideAndDeep (W&D) golden vectors from the reference implementation (survey
container only), with the protocol of make_golden_opnn.py.

Imports jqsl2012/RL_CTR_Prediction from /root/reference (read-only, never copied) and runs it
on CPU. The fixtures are data: inputs, initial parameters and the reference's outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wd.py

  g_wd*.npz  WideAndDeep fwd/bwd + 2 Adam steps, dropout p=0 (train mode), std 0.1 embeddings,
             ``linear.weight`` ~ N(0, 0.5) and ``bias`` = 0.25 (the reference starts the bias at
             zero and the wide weights at N(0, 1): overwritten so that the wide part is visible
             next to the MLP and an ignored bias shows), split over g_wd.npz, g_wd_step1.npz and
             g_wd_step2.npz as make_golden_opnn.py splits
V,F,K,B = 500,8,16,64; torch.manual_seed(0); Adam lr 1e-3, weight decay 1e-5;
`seeded_init/*` = the state right after torch.manual_seed(0) + construction (before any
overwrite), `init/*`, then per step s: x, y, p, loss, grad{s}/*, step{s+1}/*.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path(os.environ.get("CTR_REFERENCE", "/root/reference"))


def _import_reference():
    if not REF.exists():
        raise SystemExit(f"{REF} not found: goldens are generated in the survey container only")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    import src.models.p_model as P  # noqa: E402
    return P


def _np(t):
    return t.detach().cpu().numpy().copy()


def _hot_ids(g, B, F, V):  # make_golden.py's batches
    x = torch.randint(0, V, (B, F), generator=g)
    x[:, 0] = 7                              # one row owning B slots
    x[: B // 2, 1] = 3                       # two rows sharing a field
    x[B // 2:, 1] = 4
    x[:, 2] = x[:, 3]                        # duplicates inside an example
    return x


def gen(P):
    out = {}
    V, F, K, B = 500, 8, 16, 64
    torch.manual_seed(0)
    m = P.WideAndDeep(V, F, K)
    keys = list(m.state_dict())
    for k, v in m.state_dict().items():
        out[f"seeded_init/{k}"] = _np(v)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    with torch.no_grad():
        m.embedding.weight.normal_(0, 0.1)
        m.linear.weight.normal_(0, 0.5)
        m.bias.fill_(0.25)
    sd = m.state_dict()
    for k in keys:
        out[f"init/{k}"] = _np(sd[k])
    g = torch.Generator().manual_seed(3)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-5)
    crit = torch.nn.BCELoss()
    m.train()
    for s in range(2):
        x = _hot_ids(g, B, F, V)
        y = (torch.rand(B, 1, generator=g) < 0.3).float()
        p = m(x)
        loss = crit(p, y)
        m.zero_grad()
        loss.backward()
        out[f"x{s}"] = _np(x)
        out[f"y{s}"] = _np(y)
        out[f"p{s}"] = _np(p)
        out[f"loss{s}"] = np.float32(loss.item())
        named = dict(m.named_parameters())
        for k in keys:
            out[f"grad{s}/{k}"] = _np(named[k].grad)
        opt.step()
        sd = m.state_dict()
        for k in keys:
            out[f"step{s + 1}/{k}"] = _np(sd[k])
    # three files, each under the repository's 1 MiB limit for a committed file:
    #   g_wd.npz        init/*, the batches (x, y, p, loss) and grad0/*
    #   g_wd_step1.npz  seeded_init/* and step1/*
    #   g_wd_step2.npz  grad1/* and step2/*
    parts = {"": {}, "_step1": {}, "_step2": {}}
    for k, v in out.items():
        head = k.split("/")[0]
        part = "_step1" if head in ("seeded_init", "step1") else \
            "_step2" if head in ("grad1", "step2") else ""
        parts[part][k] = v
    for suffix, d in parts.items():
        np.savez_compressed(HERE / f"g_wd{suffix}.npz", **d)


def main():
    P = _import_reference()
    torch.set_num_threads(1)
    gen(P)
    for f in sorted(HERE.glob("g_wd*.npz")):
        print(f"wrote {f.name} ({f.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
