"""bench.py end to end at a small size: a plain run prints the headline line with `roofline` / `cpu_baseline` null and dumps the last
timed step's outputs; --full fills both."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--px", "128"]


def _bench(*extra, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *extra], env=env, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return lines[0]


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert line["steps"] == 2 and line["warmup"] == 1 and line["unit"] == "images/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 1000.0 / line["ms_per_step"]) <= 0.01 * line["value"]
    assert line["roofline"] is None and line["cpu_baseline"] is None
    out = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(out) == ["bn_running_mean", "bn_running_var", "grads", "head0", "head1", "head2", "loss", "weights"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 * 2 ** 20
    assert out["loss"].shape == (12,) and abs(float(out["loss"][0]) - line["loss_last"]) <= 1e-3 * abs(line["loss_last"]) + 1e-4
    # 128 px: heads of 4 x 4, 8 x 8 and 16 x 16 cells, small enough to be kept whole
    assert sorted(out[f"head{k}"].size for k in range(3)) == [2 * 255 * g * g for g in (4, 8, 16)]
    assert np.abs(out["grads"]).sum() > 0


@pytest.mark.gpu
def test_full_run_adds_roofline_and_cpu_baseline():
    line = _bench("--full")
    assert line["roofline"]["launches"] == 75 and line["roofline"]["achieved"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "images/s"
