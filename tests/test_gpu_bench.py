"""bench.py's plain run at a small configuration: ONE JSON line of the headline alone (ms_per_step = the time of one timed step), and
--dump-outputs writes what the last timed step computed as float32 / float64 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_step(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--size", "128", "--boxes", "8", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3e-3)) <= 1e-6 * d["value"]
    assert "roofline" not in d and "cpu_baseline" not in d      # (measured by --full only)
    names = {f"dec{l}_{h}" for l in range(4) for h in ("kp", "short", "mid")} | {"loss", "seg_masks", "params", "grads"}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in names)
    a = {n: np.load(out / (n + ".npy"), allow_pickle=False) for n in names}
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    assert sum(os.path.getsize(out / (n + ".npy")) for n in names) <= 64e6
    assert a["loss"].shape == (1,) and a["loss"][0] == d["config"]["last_loss"]
    # below the sampling threshold the maps are whole: batch 2 x 5 kp channels x 128^2 at level 0, sigmoid probabilities
    assert a["dec0_kp"].size == 2 * 5 * 128 * 128 and a["dec0_kp"].min() >= 0 and a["dec0_kp"].max() <= 1
    assert a["seg_masks"].size > 0 and a["params"].size == a["grads"].size and np.abs(a["grads"]).max() > 0
