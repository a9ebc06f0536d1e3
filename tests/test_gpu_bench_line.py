"""bench.py's one-GPU line, plain and with --full.  A plain run does only what its headline needs - it sets up, warms up, times the
K steps, dumps the last step's results and prints the line - and everything measured after the timed region (the roofline's own
runs, `operators`, `cpu_baseline`) comes with --full only.  Both runs time the same K steps, so they hand back the same results.
(The N > 1 branch with --full: tests/test_gpu_bench_dist.py.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ["icp_transformation", "icp_fitness", "icp_rmse", "icp_iterations", "icp_n_corr", "ransac_transformation", "ransac_fitness",
          "ransac_rmse", "ransac_inliers", "ransac_best_iteration", "ransac_iterations_run"]


def _bench(extra, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "TDV_BENCH_FORCE_DIST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1",
                        "--dump-outputs", str(out_dir)] + extra, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_line_has_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench([], tmp_path / "plain")
    assert plain["n_gpus"] == 1 and plain["steps"] == 5 and plain["steps_timed"] == 5 and plain["warmup"] == 1
    assert plain["higher_is_better"] is True and plain["dtype"] == "f32" and plain["unit"].startswith("steps/s")
    assert plain["value"] > 50 and plain["ms_per_step"] == pytest.approx(1e3 / plain["value"], rel=1e-9)
    assert plain["ransac_hyps_per_s"] > 1e6 and plain["icp_iters_per_s"] > 50 and len(plain["per_rank"]) == 1
    assert not {"roofline", "operators", "cpu_baseline", "c5", "icp_iters_per_s_bruteforce_scan"} & set(plain)

    full = _bench(["--full", "--no-cpu-baseline", "--no-operators"], tmp_path / "full")
    assert full["roofline"]["icp_iters_per_s_bruteforce_scan"] > 0 and full["roofline"]["ransac_hyps_per_s_every_test_scored"] > 0
    assert full["icp_iters_per_s_bruteforce_scan"] > 0 and full["icp_iters_per_s_reference_order_sums"] > 0
    assert full["result_check"] == plain["result_check"]
    for name in DUMPED:
        a = np.load(tmp_path / "plain" / (name + ".npy")); b = np.load(tmp_path / "full" / (name + ".npy"))
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
