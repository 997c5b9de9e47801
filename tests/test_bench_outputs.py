"""bench.py's result line and --dump-outputs: a plain run carries only the headline measurement, --full adds the
mid- and large-batch legs and the CPU baselines, and the dumped arrays of two runs with the same arguments are equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SMALL = ["--gpus", "1", "--batch", "256", "--tsteps", "30", "--steps", "3", "--warmup", "1"]


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in ("state", "nr_iters", "status", "instance")}


def test_dump_outputs_writes_a_fixed_sample_of_a_large_batch(tmp_path, monkeypatch):
    import bench
    n, b = 5, 1000
    rng = np.random.default_rng(7)
    x, iters, status = rng.standard_normal((n, b)), rng.integers(0, 100, b), np.zeros(b, dtype=np.int32)

    bench.dump_outputs(str(tmp_path / "all"), x, iters, status)
    got = _load(str(tmp_path / "all"))
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["state"], x) and np.array_equal(got["nr_iters"], iters)
    assert np.array_equal(got["instance"], np.arange(b))

    monkeypatch.setattr(bench, "DUMP_LIMIT", 100 * (n + 3) * 8)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), x, iters, status)
    s1, s2 = _load(str(tmp_path / "s1")), _load(str(tmp_path / "s2"))
    cols = s1["instance"].astype(np.int64)
    assert len(cols) == 100 and np.all(np.diff(cols) > 0)
    assert sum(a.nbytes for a in s1.values()) <= bench.DUMP_LIMIT
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)           # the same sample every time
    assert np.array_equal(s1["state"], x[:, cols]) and np.array_equal(s1["nr_iters"], iters[cols])


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path, dbmixer_nl):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    recs, outs = [], []
    for d in ("one", "two"):
        recs.append(_bench(SMALL + ["--dump-outputs", str(tmp_path / d)]))
        outs.append(_load(str(tmp_path / d)))
    rec = recs[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in rec, key
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert not {"cpu_baseline", "mid_batch", "large_batch"} & set(rec)
    a, b = outs
    assert a["state"].shape == (dbmixer_nl.n_unknowns, 256) and a["nr_iters"].shape == (256,)
    assert np.all(np.isfinite(a["state"])) and np.all(a["nr_iters"] > 0)
    assert not np.any(a["status"].astype(np.int64) & 0xA7)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert recs[0]["config"]["nr_iters_per_step"] == recs[1]["config"]["nr_iters_per_step"]


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    rec = _bench(SMALL + ["--full", "--mid-batch", "512", "--large-batch", "1024", "--cpu-iters", "2e4",
                          "--cpu-seconds", "0.5"])
    assert rec["mid_batch"]["batch_per_gpu"] == 512 and rec["mid_batch"]["value"] > 0
    assert rec["large_batch"]["batch_per_gpu"] == 1024 and rec["large_batch"]["value"] > 0
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["cores"] == 1
