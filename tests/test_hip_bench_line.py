"""bench.py on one GPU, plain and with --full: a plain run prints the headline line and nothing it had to run extra steps
or measurements for; --full adds the gate, the roofline and the accepted-step rate.  Both compute the same timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--lead", "1", "--window", "2", "--dims", "32", "32", "16",
        "--brick", "8", "8", "2", "--spmv-reps", "3"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("check", "roofline", "value_accepted_steps", "accepted_newton_steps", "device_state_after_timed_region")


def _line(extra, dump):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "WAI_BENCH_LOOPBACK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra + ["--dump-outputs", dump],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(1200)
def test_plain_and_full_lines(tmp_path):
    plain = _line([], str(tmp_path / "plain"))
    full = _line(["--full", "--no-cpu"], str(tmp_path / "full"))
    for out in (plain, full):
        assert all(k in out for k in HEADLINE), sorted(out)
        assert out["unit"] == "Newton steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
        assert out["steps"] == 3 and out["value"] > 0 and abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-6
        assert "cpu_baseline" not in out
    assert not [k for k in FULL_ONLY if k in plain], sorted(plain)
    assert "pc_reference_default" not in plain["config"]
    assert all(k in full for k in FULL_ONLY), sorted(full)
    assert max(full["check"]["step_balance_defect_per_equation"]) < 1e-4, full["check"]
    assert full["roofline"]["ms_per_launch"] > 0 and full["config"]["ms_per_krylov_iteration_device_only"] > 0
    assert all(r["accepted"] in (True, False) for r in full["config"]["timed_newton_steps"])
    # the same timed steps either way: records of the steps, and what the last one computed
    key = lambda out: [(r["time_step"], r["dt"], r["newton"], r["krylov"], r["reason"]) for r in out["config"]["timed_newton_steps"]]
    assert key(plain) == key(full)
    for name in ("cell", "solution", "residual", "region", "newton_step"):
        a, b = np.load(tmp_path / "plain" / (name + ".npy")), np.load(tmp_path / "full" / (name + ".npy"))
        assert a.shape == b.shape and np.array_equal(a, b), name
