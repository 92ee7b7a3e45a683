"""bench.py's output contract, as the round-end driver reads it (task brief, "Maintain bench.py"):
one JSON line on rank 0 with the metric / config of BASELINE.json, the whole-job value, and the
`roofline` and `cpu_baseline` objects (`--full`).  Runs a short bench in a child process (the same
command shape the driver uses at N = 1) and checks the line's fields and their arithmetic; a plain
run carries the headline fields only and writes its last step's arrays with `--dump-outputs`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_line_contract():
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        base = json.load(f)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "8", "--warmup", "2",
           "--profile-steps", "1", "--dropin-batches", "2", "--cpu-train", "512"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == base["metric"]
    assert d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic"
    B = d["config"]["per_gpu_batch"]
    assert B == 512 and "workload" in d["config"]
    # value = utterances per second of the whole job = B * N / ms_per_step (4 significant digits rounded)
    assert abs(d["value"] - B * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert 0.0 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) <= 1e-3
    # the dominant kernel's average launch lies inside the step
    assert 0.0 < r["avg_launch_ms"] < d["ms_per_step"]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["value"] > 0 and c["cores"] >= 1


def test_bench_plain_run_dumps_outputs(tmp_path):
    """Without --full the line keeps the headline fields and leaves the side measurements null;
    --dump-outputs writes the last timed step's arrays as float32 / float64 .npy, 64 MB at the most."""
    import numpy as np
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
           "--dump-outputs", str(out)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 5 and d["warmup"] == 2 and d["full"] is False
    assert d["unit"] == "utterances/s" and d["higher_is_better"] is True and d["dtype"].startswith("f32")
    assert abs(d["value"] - 512 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    for k in ("roofline", "cpu_baseline", "dropin"):
        assert d[k] is None, k
    assert d["roofline_by_kernel"] == {} and d["phases_ms_per_launch"] == {}
    # 7 steps of 512 rows went through the counters (warmup included)
    assert d["train_metrics"]["samples"] == 7 * 512
    files = sorted(os.listdir(out))
    assert sorted(n + ".npy" for n in d["dumped_outputs"]["arrays"]) == files
    arrs = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["features"].shape == (512, 1, 100, 40) and arrs["model.fc1.weight"].shape == (128, 3072)
    assert arrs["grads"].shape == arrs["adam.exp_avg"].shape == arrs["adam.exp_avg_sq"].shape
    assert all(np.isfinite(a).all() for a in arrs.values())
    assert np.abs(arrs["grads"]).max() > 0 and arrs["metrics"][1] == 7 * 512


def test_bench_gpus2_spawns_two_ranks():
    """`bench.py --gpus 2` with no launcher: the parent spawns two ranks itself (here both
    on the one GPU, gloo), rank 0 prints ONE line with n_gpus 2 / dp2 and the whole-job value."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--steps", "8",
           "--warmup", "2", "--profile-steps", "1", "--no-cpu", "--dropin-batches", "0", "--n-train", "2048"]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 1024
    assert abs(d["value"] - 1024 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert abs(d["value_per_gpu"] - d["value"] / 2) <= 0.1 + 1e-3 * d["value"]
