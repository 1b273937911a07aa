"""bench.py's plain run: the headline line only, --steps timed steps, and --dump-outputs writing what the last timed
step computed (the same arrays from run to run with the same arguments)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_outputs_full_and_sampled(tmp_path, monkeypatch):
    import torch
    import bench
    d = torch.arange(7 * 1000, dtype=torch.float64).reshape(1000, 7)
    bench.dump_outputs(d, str(tmp_path / "all"), 0, 1)
    assert sorted(os.listdir(tmp_path / "all")) == ["params.npy"]
    got = np.load(tmp_path / "all" / "params.npy")
    assert got.dtype == np.float64 and np.array_equal(got, d.numpy())
    # beyond the budget: a seeded sample of rows, the same one every time, with its row numbers
    monkeypatch.setattr(bench, "OUTPUT_BUDGET_BYTES", 64 * 100)
    for sub in ("s1", "s2"):
        bench.dump_outputs(d, str(tmp_path / sub), 0, 1)
    rows = np.load(tmp_path / "s1" / "params_rows.npy")
    part = np.load(tmp_path / "s1" / "params.npy")
    assert rows.dtype == np.float64 and part.shape == (100, 7) and part.nbytes + rows.nbytes <= 64 * 100
    assert np.array_equal(part, d.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "params_rows.npy"))
    # several ranks: one file per rank, the budget shared
    bench.dump_outputs(d, str(tmp_path / "r"), 1, 2)
    assert sorted(os.listdir(tmp_path / "r")) == ["params_rank1.npy", "params_rank1_rows.npy"]
    assert np.load(tmp_path / "r" / "params_rank1.npy").shape == (50, 7)


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MFX_BENCH_STUB"):
        env.pop(k, None)
    V = 3000
    outs = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--voxels", str(V),
                            "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, p.stdout
        r = lines[0]
        assert r["steps"] == 3 and r["warmup"] == 1 and r["full"] is False
        assert r["ms_per_step"] > 0 and r["unit"] == "voxels/s" and r["higher_is_better"] is True
        assert abs(r["value"] * r["ms_per_step"] * 1e-3 / V - 1.0) < 1e-2
        # nothing but the headline
        assert r["roofline"] is None and r["cpu_baseline"] is None
        assert not {"fp64_kernel", "c4", "c1", "c5", "k2_csf", "host_api"} & set(r)
        assert os.listdir(tmp_path / run) == ["params.npy"]
        P = np.load(tmp_path / run / "params.npy")
        assert P.dtype == np.float64 and P.shape == (V, 7)
        assert np.all((P[:, 3:5] >= 0) & (P[:, 3:5] < 782)) and np.allclose(P[:, 1] + P[:, 2], 1.0)
        outs.append(P)
    assert np.array_equal(outs[0], outs[1])
