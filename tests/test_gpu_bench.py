"""bench.py's contract on a small instance of its workload (run with -m gpu): one JSON line with the fields the
driver reads, `value` = the job's average rate whatever --steps / --warmup are, exactly --steps timed iterations;
a plain run only times, --full adds the rest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra, full=True):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--points", "2048", "--no-cpu-baseline",
                        "--min-timed", "0.05", *(("--full",) if full else ()), *extra], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_line_and_job_average():
    a = run_bench("--steps", "20", "--warmup", "5")
    b = run_bench("--steps", "150", "--warmup", "0")
    for d, k, w in ((a, 20, 5), (b, 150, 0)):
        assert d["metric"].startswith("relaxation iterations/sec") and d["unit"] == "iterations/s"
        assert d["n_gpus"] == 1 and d["steps"] == k and d["warmup"] == w and d["higher_is_better"] is True
        assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
        assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
        t = d["timing"]
        # exactly K timed iterations, in order, inside the run's first max(K, job) iterations
        assert t["timed_steps"] == k and sum(ln for _s, ln in t["slices"]) == k
        ends = [a + ln for a, ln in t["slices"]]
        assert all(e <= a for e, (a, _l) in zip(ends, t["slices"][1:])) and ends[-1] <= max(k, t["job_iterations"])
        assert abs(d["ms_per_step"] - 1e3 * t["timed_seconds"] / k) < 1e-9 * d["ms_per_step"]
        assert t["slices_per_rotation"] == -(-t["job_iterations"] // k) and t["rotations"] >= 3
        assert len(t["iterations_per_s_by_slice"]) == t["slices_per_rotation"]
        r = d["roofline"]
        assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and r["launches"] > 0
        assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_us"] * 1e-6) / 1e9) < 1e-6 * r["achieved"]
        w_run = d["whole_run"]
        assert w_run["converged"] and w_run["iterations_run"] == t["job_iterations"]
    # the same job: the two slicings agree with each other and with the job timed in one piece
    assert a["timing"]["job_iterations"] == b["timing"]["job_iterations"]
    # (at this size an iteration is ~15 us, so the two synchronisations around a 20-iteration slice weigh 10-20 %; at
    # config 3's size the same comparison is within 2 %: DESIGN.md section 6)
    assert abs(a["value"] / b["value"] - 1.0) < 0.35, (a["value"], b["value"])
    assert abs(a["value"] / a["whole_run"]["iterations_per_s"] - 1.0) < 0.35


def test_plain_run_times_only_and_dumps_its_outputs(tmp_path):
    """A plain run carries the headline and nothing that needs runs of its own; --dump-outputs writes what the timed
    run returned, the same arrays from run to run (seeded inputs, fixed-order sums, a run the controller cannot stop)."""
    runs = []
    for tag in ("a", "b"):
        d = run_bench("--steps", "150", "--warmup", "5", "--dump-outputs", str(tmp_path / tag), full=False)
        assert d["steps"] == 150 and d["warmup"] == 5 and d["timing"]["timed_steps"] == 150
        assert d["value"] > 0 and abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
        assert d["dtype"] == "f32" and d["higher_is_better"] is True and d["unit"] == "iterations/s"
        for key in ("roofline", "whole_run", "precision_f64", "cpu_baseline", "mae_check"):
            assert key not in d, key
        assert "rotations" not in d["timing"]
        runs.append({f: np.load(tmp_path / tag / f) for f in ("positions.npy", "check_trace.npy", "result.npy")})
    a, b = runs
    assert a["positions.npy"].shape == (2048, 5) and a["positions.npy"].dtype == np.float64
    assert np.isfinite(a["positions.npy"]).all() and a["result.npy"].shape == (4,)
    total = sum(v.nbytes for v in a.values())
    assert total <= 64 << 20
    for f in a:
        scale = max(1.0, float(np.abs(a[f]).max()))
        assert a[f].shape == b[f].shape and np.allclose(a[f], b[f], rtol=0, atol=1e-6 * scale), f


@pytest.mark.parametrize("k", [20, 50, 100, 200])
def test_fewer_steps_than_the_job_still_price_the_job(k):
    """Config 3 at its own size (a 396-iteration job: 8 sixteen-stage, 43 two-stage, 345 one-stage iterations).  With
    K below the job's length the K timed iterations hold every phase in proportion, so the headline agrees with the
    rotation median of the same process, which times every iteration of the job in K-iteration slices.  At K = 20 the
    unfolding phase's share is 0.4 of an iteration, and its rounding is worth about 5 %."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(k), "--warmup", "5", "--full",
                        "--no-cpu-baseline", "--no-precision-f64"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    t = d["timing"]
    assert t["job_iterations"] > k and t["timed_steps"] == k and sum(ln for _s, ln in t["slices"]) == k
    assert t["slices"][0][0] < 8 or k < 50               # from 50 steps up the sample holds an unfolding iteration
    band = 0.08 if k < 50 else 0.04                      # measured: 0.980-0.997 of the median
    assert abs(d["value"] / t["iterations_per_s"]["median"] - 1) <= band, (k, d["value"], t["iterations_per_s"])


def run_bench_env(env_extra, *args):
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       timeout=900, cwd=ROOT, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_gpus_n_launched_plainly_runs_the_row_sharded_path():
    """`python bench.py --gpus 2` with no launcher around it: the script starts the two ranks itself and the line
    measures ONE config-4-style embedding row-sharded over them (strong scaling), the independent replicas following
    as a secondary field.  Rehearsal on the one GPU of this box: both ranks on device 0, gloo instead of RCCL (RCCL
    refuses two ranks on one device), 4 096 points."""
    d = run_bench_env({"TOPOLOW_BENCH_OVERSUBSCRIBE": "1", "TOPOLOW_DIST_BACKEND": "gloo",
                       "TOPOLOW_SYMMETRIC_MIN_N": "1024"},       # config 4 is above the size gate, 4 096 points are not
                      "--gpus", "2", "--points", "4096", "--steps", "20", "--warmup", "5", "--min-timed", "0.05",
                      "--no-cpu-baseline")
    # one-stage iterations ran as the symmetric sweep sharded over the ranks (tile segments, one all-reduce of the moves)
    assert d["config"]["symmetric_segments"] is True and "symm_sweep_kernel" in d["roofline"]["kernel"]
    assert d["scaling"] == "strong" and d["ranks"] == 2 and d["n_gpus"] == 1      # devices really used: one
    assert d["collective_backend"] == "gloo" and d["rccl_ranks"] == 0
    assert "config 4" in d["config"]["workload"] and d["config"]["parallelism"] == "rows/2"
    assert d["steps"] == 20 and d["warmup"] == 5 and d["value"] > 0
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    t = d["timing"]
    assert t["slices_per_rotation"] == -(-t["job_iterations"] // 20) and t["rotations"] >= 3
    assert d["whole_run"]["iterations_run"] == t["job_iterations"] and d["whole_run"]["converged"]
    r = d["roofline"]
    assert len(r["per_gpu_frac"]) == 2 and all(0 < f < 1 for f in r["per_gpu_frac"])
    rows = [x["rows"] for x in d["breakdown_ms_per_iteration"]["per_rank"]]
    assert rows == [[0, 2048], [2048, 4096]]
    rep = d["replicas"]
    assert rep["scaling"] == "weak" and rep["value"] > 0 and "replicated" in rep["config"]["workload"]
    # the base of the strong-scaling curve: the same code at world size 1
    one = run_bench_env({}, "--gpus", "1", "--mode", "sharded", "--points", "4096", "--steps", "20", "--warmup", "5",
                        "--min-timed", "0.05", "--no-cpu-baseline")
    assert one["scaling"] == "strong" and one["ranks"] == 1 and one["n_gpus"] == 1 and "replicas" not in one
    assert one["timing"]["job_iterations"] > 0 and one["config"]["parallelism"] == "rows/1"
    # same embedding, same schedule: the two runs stop within a few checks of each other at the same error
    assert abs(one["timing"]["job_iterations"] - t["job_iterations"]) <= 30
    assert abs(one["final_mae"] / d["final_mae"] - 1) < 0.02


def test_bench_refuses_more_gpus_than_the_box_has():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode != 0 and "GPU(s) visible" in p.stderr


def test_bench_reports_the_f64_job_and_the_host():
    d = run_bench("--steps", "50", "--warmup", "5")
    f = d["precision_f64"]
    assert f["converged"] and f["iterations_per_s"] > 0 and 0 < f["frac"] < 1
    assert abs(f["final_mae"] / d["whole_run"]["final_mae"] - 1) < 0.03       # same job, same schedule, wider arithmetic
    assert "f64" in d["dtype_note"]
