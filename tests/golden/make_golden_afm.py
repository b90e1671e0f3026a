"""Capture the AFM golden vectors from the reference implementation (survey container only),
with the protocol of make_golden_opnn.py.

Imports jqsl2012/RL_CTR_Prediction from /root/reference (read-only, never copied) and runs it
on CPU. The fixtures are data: inputs, initial parameters and the reference's outputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_afm.py

  g_afm.npz   AFM (src/models/p_model.py:438-486) fwd/bwd + 2 Adam steps with both dropouts
              switched off: the reference module's ``F.dropout`` (which ignores eval()) is the
              identity in this process only.
V,F,K,B = 500,8,16,64; torch.manual_seed(0); Adam lr 1e-3, weight decay 1e-5;
`seeded_init/*` = the state right after torch.manual_seed(0) + construction (before any
overwrite), `init/*`, then per step s: x, y, p, loss, grad{s}/*, step{s+1}/*.

The attention has to bite. With std-0.1 embeddings the pair products are ~1e-2, the scores
barely move and the attention stays within 3% of 1/28: a fixture that cannot tell a broken
attention path from a correct one. So the capture uses feature_embedding.weight ~ N(0, 1) and
8 x the seeded attention_softmax.weight, and asserts a peaked attention on batch 0.
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path(os.environ.get("CTR_REFERENCE", "/root/reference"))


class _NoDropout:
    """torch.nn.functional with dropout as the identity, for the reference module alone."""

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    @staticmethod
    def dropout(x, p=0.5, training=True, inplace=False):
        return x


def _import_reference():
    if not REF.exists():
        raise SystemExit(f"{REF} not found: goldens are generated in the survey container only")
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(REF))
    import src.models.p_model as P  # noqa: E402
    P.F = _NoDropout()  # this process only
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


def _attention(m, x):
    """The reference's attention weights [B, P] (p_model.py:473-478), recomputed."""
    e = m.feature_embedding(x)
    q = e[:, m.row] * e[:, m.col]
    h = torch.relu(m.attention_net(q))
    return torch.softmax(m.attention_softmax(h), dim=1).squeeze(-1)


def gen(P):
    out = {}
    V, F, K, B = 500, 8, 16, 64
    torch.manual_seed(0)
    m = P.AFM(V, F, K)
    keys = list(m.state_dict())
    for k, v in m.state_dict().items():
        out[f"seeded_init/{k}"] = _np(v)
    with torch.no_grad():
        m.feature_embedding.weight.normal_(0, 1.0)
        m.attention_softmax.weight.mul_(8.0)
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
        if s == 0:
            with torch.no_grad():
                a = _attention(m, x)
            print(f"attention on batch 0: min {float(a.min()):.3g} max {float(a.max()):.3g}")
            assert float(a.max()) > 0.3 and float(a.min()) < 1e-3, "the attention does not bite"
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
    np.savez_compressed(HERE / "g_afm.npz", **out)


def main():
    P = _import_reference()
    torch.set_num_threads(1)
    gen(P)
    for f in sorted(HERE.glob("g_afm*.npz")):
        print(f"wrote {f.name} ({f.stat().st_size} bytes)")
        assert f.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
