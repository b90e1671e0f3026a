"""bench.py's plain run and --dump-outputs: the dump helpers on the host, and one tiny plain
run of the benchmark itself on the GPU (the command line is what is under test)."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module")
def bench():
    import bench as B
    return B


def _state(V=300_000, K=8):
    g = torch.Generator().manual_seed(0)
    return {"feature_embedding.weight": torch.randn(V, K, generator=g),   # 9.6 MB: sampled
            "linear.weight": torch.randn(V, 1, generator=g),              # 1.2 MB: whole
            "mlp.0.weight": torch.randn(7, 5, generator=g),
            "steps": torch.tensor(3)}                                     # not floating: left out


def test_sample_rows_fixed_sorted_and_holds_the_batch_rows(bench):
    ids = np.random.default_rng(1).integers(0, 300_000, size=(64, 26))
    rows = bench.sample_rows(300_000, ids)
    assert np.array_equal(rows, bench.sample_rows(300_000, ids))  # the same from call to call
    assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0)
    assert rows.min() >= 0 and rows.max() < 300_000
    assert np.isin(np.unique(ids), rows).all()
    # more batch rows than the sample holds: a seeded choice of them, the size bounded
    many = bench.sample_rows(10_000_000, np.arange(0, 10_000_000, 7))
    assert many.size <= 2 * bench.DUMP_SAMPLE_ROWS
    # a table smaller than the sample: every row at most once
    assert np.array_equal(np.unique(bench.sample_rows(100)), bench.sample_rows(100))


def test_collect_and_dump_outputs(bench, tmp_path):
    st = _state()
    ids = np.random.default_rng(2).integers(0, 300_000, size=(64, 26))
    scal = {"loss_last_step": torch.tensor([0.25]),
            "loss_sum": torch.tensor([1.5], dtype=torch.float64)}
    out = bench.collect_outputs(st, scal, table_ids=ids, table_rows=300_000)
    assert set(out) == {"loss_last_step", "loss_sum", "feature_embedding.weight",
                        "feature_embedding.weight.rows", "linear.weight", "mlp.0.weight"}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    rows = out["feature_embedding.weight.rows"].astype(np.int64)
    assert np.array_equal(rows, bench.sample_rows(300_000, ids))
    assert np.array_equal(out["feature_embedding.weight"],
                          st["feature_embedding.weight"].numpy()[rows])
    assert np.array_equal(out["linear.weight"], st["linear.weight"].numpy())
    assert out["loss_sum"].dtype == np.float64 and out["loss_sum"][0] == 1.5
    # copies: training on does not change what was collected
    st["mlp.0.weight"].add_(1.0)
    assert not np.array_equal(out["mlp.0.weight"], st["mlp.0.weight"].numpy())
    bench.dump_outputs(tmp_path / "d", out)
    assert sorted(p.name for p in (tmp_path / "d").iterdir()) == sorted(k + ".npy" for k in out)
    for k, a in out.items():
        assert np.array_equal(np.load(tmp_path / "d" / (k + ".npy")), a)


def test_dump_refuses_more_than_the_limit(bench, tmp_path):
    big = {"x": np.zeros(bench.DUMP_LIMIT_BYTES // 4 + 1, dtype=np.float32)}
    with pytest.raises(RuntimeError, match="exceed"):
        bench.dump_outputs(tmp_path / "d", big)
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_outputs(cuda, tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` at the smallest config: the
    result line has the headline keys with K timed steps and none of --full's, and DIR holds
    the loss and the parameters as float32 / float64 arrays within the size limit."""
    import bench as B
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "2", "--config", "c2", "--dump-outputs", str(tmp_path / "d")],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["warmup"] == 2 and res["full"] is False
    assert res["unit"] == "examples/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["ms_per_step"] > 0
    # value = examples of the K steps over their time
    assert res["value"] == pytest.approx(B.CONFIGS["c2"]["B"] / (res["ms_per_step"] * 1e-3))
    for k in ("roofline", "step_roofline", "kernels", "driver_loop", "cpu_baseline"):
        assert k not in res
    files = {p.stem: np.load(p) for p in (tmp_path / "d").glob("*.npy")}
    assert {"loss_last_step", "loss_sum", "bias", "linear.weight", "feature_embedding.weight",
            "feature_embedding.weight.rows"} <= set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(np.isfinite(a).all() for a in files.values())
    assert files["loss_last_step"][0] > 0.0  # a mean BCE (of N(0,1)-initialised tables: large)
    assert files["feature_embedding.weight"].shape == (
        files["feature_embedding.weight.rows"].size, B.CONFIGS["c2"]["K"])
