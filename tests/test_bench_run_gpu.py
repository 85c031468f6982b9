"""GPU: bench.py end to end in a process of its own -- the plain run (the headline alone, a few seconds besides its
steps) and a trimmed --full run (what moved behind the option still lands on the line)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config")


def _bench(*args, timeout=300):
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(args), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), wall


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(dev, tmp_path):
    rec, wall = _bench("--steps", "20", "--warmup", "5", "--dump-outputs", str(tmp_path))
    for k in CONTRACT:
        assert k in rec, k
    assert rec["metric"] == "point-clouds/sec" and rec["unit"] == "point-clouds/sec" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and rec["steps"] == 20 and rec["warmup"] == 5
    assert rec["value"] == pytest.approx(rec["config"]["clouds_total"] * 1e3 / rec["ms_per_step"], rel=1e-6)
    assert rec["config"]["steps_in_flight"] == 4 and rec["extras"] is None
    for gone in ("one_step_at_a_time", "at_100_steps", "value_streaming", "global", "roofline", "cpu_baseline", "repeats"):
        assert gone not in rec, gone
    out = np.load(tmp_path / "xyz_feat.npy")
    assert out.dtype == np.float32 and out.shape == (8, 8192, 131) and np.isfinite(out).all()
    # the issue's budget: at most 30 s of the whole run outside the warm-up and timed steps
    assert wall - (rec["steps"] + rec["warmup"]) * rec["ms_per_step"] * 1e-3 < 30.0


@pytest.mark.gpu
def test_full_run_keeps_what_moved(dev, tmp_path):
    side = tmp_path / "extras.json"
    rec, _ = _bench("--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline", "--no-pmc", "--no-global-line",
                    "--extras-file", str(side))
    for k in CONTRACT:
        assert k in rec, k
    assert set(rec["one_step_at_a_time"]) == {"value", "ms_per_step"}
    assert set(rec["at_100_steps"]) == {"value", "ms_per_step"}
    assert rec["value_streaming"]["steps_in_flight"] == 4
    assert rec["roofline"]["kernel"].startswith("flex_conv_x6_kernel<64,64>")
    back = json.load(open(side))
    assert len(back["repeats"]["ms_per_step"]) == 7 and back["value"] == pytest.approx(rec["value"], rel=1e-6)
