#!/usr/bin/env python3
"""Study: what the event records on a RANSAC batch's path cost (profiles/r18/ransac_no_events.md).  Makes the headline RANSAC call -
200k pairs built as bench.py builds them, 2,000,000 hypotheses, seed 42, confidence 2.0 - with the score timer on and with it off,
a warm-up call in front of each, and prints one JSON line per call: the host-clock time of the synchronised call, the timer's reading
(total ms, dispatches, mean us per dispatch) and the result's fields.
Under the profiler the calls are told apart by their k_gather_pq (one per call, warm-ups included):
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/studies/ransac_event_gaps.py
    python tools/studies/ransac_batch_split.py --call -3 <kernel_trace.csv>      # timing on  (order on,off: warm, ON, warm, off)
    python tools/studies/ransac_batch_split.py --call -1 <kernel_trace.csv>      # timing off
Without the profiler, --repeats N times every call N times behind its warm-up (the real-use reading: the call with timing off)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--hyps", type=int, default=2000000)
    ap.add_argument("--order", default="on,off")
    ap.add_argument("--repeats", type=int, default=1)
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    ctx = tdv.Context(0)
    dev = torch.device("cuda", 0)
    n = args.points
    voxel = float(np.float32(synth.mean_spacing(n)))
    # bench.py's inputs, rank 0
    tgt_np, _ = synth.sample_object(n, 42)
    src_np, T_gt = synth.make_scene(n, 42)
    nn = ctx.icp_correspondences(src_np, tgt_np, T_gt, 1.0)["corr"]
    rng = np.random.Generator(np.random.PCG64(1234))
    corr_np = np.where(rng.random(n) < 0.5, nn, rng.integers(0, n, n)).astype(np.int32)
    d_src = torch.from_numpy(src_np).to(dev); d_tgt = torch.from_numpy(tgt_np).to(dev); d_corr = torch.from_numpy(corr_np).to(dev)
    torch.cuda.synchronize()

    def call():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ctx.ransac_dev(d_src.data_ptr(), n, d_tgt.data_ptr(), n, None, None, d_corr.data_ptr(), voxel, args.hyps, 2.0, 42)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    for mode in args.order.split(","):
        on = mode == "on"
        ctx.timing_enable(on)
        call()                                   # warm-up: workspace sized, clocks up
        ctx.timing_read(tdv.TIMER_RANSAC_SCORE)
        for rep in range(args.repeats):
            t, r = call()
            ms, launches = ctx.timing_read(tdv.TIMER_RANSAC_SCORE)
            print(json.dumps({"timing": mode, "repeat": rep, "call_ms": t * 1e3, "hyps_per_s": args.hyps / t, "timer_ms": ms, "timer_launches": launches,
                              "timer_us_per_dispatch": ms * 1e3 / max(launches, 1), "best_iteration": int(r.best_iteration), "inliers": int(r.inliers),
                              "iterations_run": int(r.iterations_run), "rmse": float(r.rmse), "T": r.transformation.tobytes().hex(),
                              "scored_share": ctx.last_ransac_scored(), "bound": list(ctx.last_ransac_bound())}), flush=True)
    ctx.timing_enable(False)
    ctx.close()


if __name__ == "__main__":
    main()
