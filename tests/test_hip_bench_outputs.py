"""`bench.py --dump-outputs DIR` on the device: a plain run times exactly --steps closed-loop steps, prints the headline line and
writes the rollout log of its timed region (W prime + K closed-loop slots) as float32 .npy files; two runs with the same arguments
write the same arrays (same inputs, same result)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _bench(out_dir):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2", "--agents", "32", "--polylines", "128", "--lights", "32",
           "--pre-roll-ms", "0", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=str(ROOT), env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_bench_dumps_its_timed_rollout_log(tmp_path):
    line = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 8 and line["warmup"] == 2 and line["finite"] and line["repeats"] == 1
    assert abs(line["value"] - 32 * 8 / (line["ms_per_step"] * 8e-3)) < 2e-5 * line["value"]
    assert "cpu_baseline" not in line and line["roofline"] is None and "wosac_shape" not in line and "training" not in line
    a = {p.stem: np.load(p) for p in sorted((tmp_path / "a").glob("*.npy"))}
    assert {"out_pose", "out_valid", "out_motion", "out_action", "out_tl_state", "out_reward"} <= set(a)
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["out_pose"].shape == (1, 32, 10, 3) and a["out_valid"].shape == (1, 32, 10)
    assert np.isfinite(a["out_pose"]).all() and a["out_valid"][:, :, -1].sum() > 0  # (the last closed-loop step was logged)
    _bench(tmp_path / "b")
    b = {p.stem: np.load(p) for p in sorted((tmp_path / "b").glob("*.npy"))}
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.allclose(a[k], b[k], rtol=1e-5, atol=1e-5), k
