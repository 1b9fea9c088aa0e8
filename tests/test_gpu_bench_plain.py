"""``bench.py --gpus 1 --steps K --warmup W`` without ``--full``: exactly K timed steps (an episode end inside them is crossed with the
clock stopped), ``ms_per_step`` of one of them, none of the extra measurements, no detail file, and ``--dump-outputs`` writing the
same arrays from run to run (seeded inputs, order-independent reductions)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETAIL = os.path.join(ROOT, "profiles", "bench_detail.json")


def _bench(out_dir, steps):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2", "--envs-per-gpu", "4",
           "--dump-outputs", str(out_dir)]
    run = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, f"bench failed:\n{run.stdout[-3000:]}\n{run.stderr[-6000:]}"
    return json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_run_times_the_steps_asked_for_and_dumps_the_same_outputs(tmp_path):
    detail_before = os.path.getmtime(DETAIL) if os.path.exists(DETAIL) else None
    steps = 85                      # longer than an 80-step episode
    lines = [_bench(tmp_path / d, steps) for d in ("a", "b")]
    for line in lines:
        assert line["steps"] == steps and line["warmup"] == 2 and line["n_gpus"] == 1
        assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["value"] > 0 and line["ms_per_step"] > 0
        assert abs(line["value"] - 4 * 1e3 / line["ms_per_step"]) < 1e-3 * line["value"]
        assert line["repeats"] == 1 and line["value_spread"]["min"] == line["value_spread"]["max"] == line["value"]
        assert line["roofline"] is None and line["detail"] is None
        for k in ("legs", "poisson_256", "cpu_baseline", "value_unforced"):
            assert k not in line, k
    assert (os.path.getmtime(DETAIL) if os.path.exists(DETAIL) else None) == detail_before
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"obs_velocity.npy", "reward.npy", "terminated.npy", "truncated.npy"} <= set(names), names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), n
        assert np.array_equal(a, b), n
    assert np.load(tmp_path / "a" / "reward.npy").shape == (4,)
