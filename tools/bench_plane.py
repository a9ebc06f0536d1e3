#!/usr/bin/env python3
"""Plane segmentation (tdv_segment_planes_dev) at frame size: one 1280x720 depth frame (a floor tilted 20 degrees 1 m from the camera,
the 6 cm high top of a box on it, ~0.9 M points) unprojected on the device by tdv_depth_to_cloud_dev, as tests/test_gpu_plane.py
builds it.  Per configuration (100 and 1000 hypotheses x 1 and 5 planes; either count is one chunk, so the early stop has nothing
to cut): the median time of --repeats alternating rounds, ms per call, and the (hypothesis, candidate) tests of the rounds that kept a
plane per second of the whole call.  On this frame a 5-plane call keeps the floor and the box top; its later rounds find too few
points.  Only the f64 scoring path exists (DESIGN.md 7 says why), so there is no f32 variant to time.  --cpu also times the numpy
restatement of one configuration, for scale.  Prints one JSON line.

    python tools/bench_plane.py [--repeats 9] [--cpu]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, FX, FY, CX, CY, SCALE, ZMAX = 1280, 720, 900.0, 900.0, 640.0, 360.0, 1000.0, 2.0


def frame():
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    rx, ry = (u - CX) / FX, (v - CY) / FY
    n = np.array([0.0, -np.sin(np.radians(20)), -np.cos(np.radians(20))])
    z = 1.0 / -(n[0] * rx + n[1] * ry + n[2])
    box = (np.abs(u - 560) < 120) & (np.abs(v - 400) < 80)
    z = np.where(box, z - 0.06, z)
    return np.round(z * SCALE).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--cpu", action="store_true", help="also time the numpy restatement (100 hypotheses, 1 plane)")
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)
    raw = frame()
    d_raw = torch.from_numpy(raw.reshape(-1).view(np.int16).copy()).to(dev)
    d_xyz = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    n = ctx.depth_to_cloud_dev(d_raw.data_ptr(), None, None, W, H, SCALE, FX, FY, CX, CY, ZMAX, d_xyz.data_ptr(), None, W * H)
    d_lab = torch.zeros(n, dtype=torch.int32, device=dev)
    d_rest = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    configs = {}
    for hyps in (100, 1000):
        for planes in (1, 5):
            configs["h%d_p%d" % (hyps, planes)] = dict(num_iterations=hyps, max_planes=planes, distance_threshold=0.005, min_inliers=1000)
    run = lambda p: ctx.segment_planes_dev(d_xyz.data_ptr(), n, d_labels=d_lab.data_ptr(), d_rest=d_rest.data_ptr(), **p)   # noqa: E731
    info = {k: run(p) for k, p in configs.items()}        # warm-up (arena growth, code load) and the counts
    torch.cuda.synchronize()
    times = {k: [] for k in configs}
    for _ in range(args.repeats):
        for k, p in configs.items():                        # alternating, so that a slow phase of the machine hits every one
            t = time.perf_counter()
            run(p)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    out = dict(tool="bench_plane", n_points=n, scoring="f64", repeats=args.repeats)
    for k in configs:
        res, n_rest = info[k]
        ms = 1e3 * float(np.median(times[k]))
        tests = sum(r["iterations_run"] * r["candidates"] for r in res)
        out[k] = dict(ms=round(ms, 4), planes=len(res), iterations_run=[r["iterations_run"] for r in res], tests=tests,
                      tests_per_s=float("%.4g" % (tests / (ms * 1e-3))), n_rest=n_rest)
    if args.cpu:
        import plane_restatement as R
        cloud = d_xyz[:3 * n].cpu().numpy().reshape(-1, 3)
        t = time.perf_counter()
        R.segment_planes(cloud, dict(num_iterations=100, max_planes=1, distance_threshold=0.005, min_inliers=1000))
        out["numpy_restatement_h100_p1_ms"] = round(1e3 * (time.perf_counter() - t), 1)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
