"""bench.py --dump-outputs: what the timed loop's last step computed, in the caller's observation order, small enough to keep."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_a_run_without_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_bench_has_the_full_option():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_a_plain_run_reports_the_headline_alone_and_full_adds_the_rest():
    """Without --full the line carries the headline and its workload, and nothing that takes a run of its own after the timed steps;
    with --full the same command also prices the kernel and the LM iteration (C2: the small scene)."""
    def run(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--config", "C2", *extra],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    moved = {"roofline", "roofline_lm", "lm", "lm_headline", "cpu_baseline", "next_rows", "shard_eval_n8", "device_memory"}
    plain = run()
    assert not moved & set(plain)
    assert plain["metric"] == "residual+Jacobian evals/sec" and plain["unit"] == "obs evals/s" and plain["higher_is_better"] is True and plain["dtype"] == "f64"
    assert plain["steps"] == 5 and plain["warmup"] == 1 and plain["ms_per_step"] > 0
    assert abs(plain["value"] - plain["config"]["observations_total"] / (plain["ms_per_step"] * 1e-3)) <= 1e-9 * plain["value"]
    full = run("--full", "--lm-iters", "6", "--no-cpu-baseline")
    assert {"roofline", "roofline_lm", "lm", "lm_headline", "device_memory"} <= set(full)
    assert {k: v for k, v in full.items() if k in plain and k not in ("value", "ms_per_step")} == {k: v for k, v in plain.items() if k not in ("value", "ms_per_step")}
    assert full["roofline"]["kernel_ms"] > 0 and "error" not in full["lm"] and full["lm_headline"]["ms_per_lm_iteration"] > 0


@pytest.mark.gpu
def test_dumped_outputs_are_the_evaluation_of_the_headline_scene(tmp_path):
    """C4 (2.04 M observations) does not fit the budget: a seeded sample is written, with its indices; every sampled row equals
    rsba_evaluate's residuals and raw Jacobian blocks for that observation of the same scene, to the bit."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "C4", "--no-lm",
                        "--no-cpu-baseline", "--no-next-rows", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3
    files = sorted(os.listdir(out))
    assert files == ["jacobians.npy", "observation_index.npy", "residuals.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64_000_000
    res, jac, idx = (np.load(out / f) for f in ("residuals.npy", "jacobians.npy", "observation_index.npy"))
    assert res.dtype == jac.dtype == idx.dtype == np.float64

    from rsba_amd import capi
    from rsba_amd.scene import SEED, make_config
    prob = make_config("C4", seed=SEED).problem
    n, k = prob.num_observations, prob.jacobian_cols
    pick = idx.astype(np.int64)
    assert np.array_equal(pick, idx) and 100_000 < len(pick) < n and np.all(np.diff(pick) > 0) and pick[-1] < n
    assert res.shape == (len(pick), 2) and jac.shape == (len(pick), 2, k)
    with capi.DeviceProblem(prob) as dp:
        ref = dp.evaluate()
    assert np.array_equal(res, ref["residuals"][pick]) and np.array_equal(jac, ref["jacobians"][pick])
