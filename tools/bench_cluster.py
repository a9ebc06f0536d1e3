#!/usr/bin/env python3
"""Euclidean clustering (tdv_cluster_dbscan_dev) on two clouds, device-resident, labels + order + grouped rows + offsets per call:
  scene  the bin scene of tests/cluster_restatement.py (six parts on a floor) with the floor taken off by tdv_segment_planes_dev
         (~24 k points), at the three parameter sets of the tests;
  frame  the rest cloud of one 1280x720 depth frame: a floor 1 m from the camera with six box tops 4 to 9 cm above it, unprojected
         by tdv_depth_to_cloud_dev, the floor taken off (~190 k points at pixel pitch), at eps 3 mm / 10 and 5 mm / 20.
Per configuration: the median of --repeats alternating rounds in ms per call, and the result record.  --cpu also times the scipy
restatement of each configuration on this host, once.  Prints one JSON line.

    python tools/bench_cluster.py [--repeats 9] [--cpu]
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
    z = np.full((H, W), 1.0)
    for b in range(6):
        cu, cv = 240 + 400 * (b % 3), 200 + 320 * (b // 3)
        z = np.where((np.abs(u - cu) < 110) & (np.abs(v - cv) < 75), 1.0 - 0.04 - 0.01 * b, z)
    return np.round(z * SCALE).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--cpu", action="store_true", help="also time the scipy restatement of every configuration")
    args = ap.parse_args()
    import torch
    import cluster_restatement as R
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)

    clouds = {}
    pts = R.scene(synth)[0]
    d_pts = torch.from_numpy(pts).to(dev)
    d_rest = torch.zeros(pts.size, dtype=torch.float32, device=dev)
    _, n_rest = ctx.segment_planes_dev(d_pts.data_ptr(), len(pts), d_rest=d_rest.data_ptr(), **R.PLANE)
    clouds["scene"] = (d_rest, n_rest)
    d_raw = torch.from_numpy(frame().reshape(-1).view(np.int16).copy()).to(dev)
    d_xyz = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    n = ctx.depth_to_cloud_dev(d_raw.data_ptr(), None, None, W, H, SCALE, FX, FY, CX, CY, ZMAX, d_xyz.data_ptr(), None, W * H)
    d_frest = torch.zeros(3 * n, dtype=torch.float32, device=dev)
    _, n_frest = ctx.segment_planes_dev(d_xyz.data_ptr(), n, d_rest=d_frest.data_ptr(), max_planes=1, distance_threshold=0.005,
                                        num_iterations=100)
    clouds["frame"] = (d_frest, n_frest)
    torch.cuda.synchronize()

    configs = {"scene_e%d_m%d" % (round(e * 1e3), m): ("scene", e, m) for e, m in R.PARAMS}
    configs.update({"frame_e3_m10": ("frame", 0.003, 10), "frame_e5_m20": ("frame", 0.005, 20)})
    n_max = max(c[1] for c in clouds.values())
    d_lab = torch.zeros(n_max, dtype=torch.int32, device=dev)
    d_ord = torch.zeros(n_max, dtype=torch.int32, device=dev)
    d_grp = torch.zeros(3 * n_max, dtype=torch.float32, device=dev)

    def run(cfg):
        d, m = clouds[cfg[0]]
        return ctx.cluster_dbscan_dev(d.data_ptr(), m, cfg[1], cfg[2], d_labels=d_lab.data_ptr(), d_order=d_ord.data_ptr(),
                                      d_grouped=d_grp.data_ptr())

    info = {k: run(c) for k, c in configs.items()}          # warm-up (arena growth, code load) and the counts
    torch.cuda.synchronize()
    times = {k: [] for k in configs}
    for _ in range(args.repeats):
        for k, c in configs.items():                        # alternating, so that a slow phase of the machine hits every one
            t = time.perf_counter()
            run(c)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    out = dict(tool="bench_cluster", repeats=args.repeats, n_points={k: v[1] for k, v in clouds.items()})
    for k, c in configs.items():
        res, off = info[k]
        out[k] = dict(ms=round(1e3 * float(np.median(times[k])), 4), min_ms=round(1e3 * float(np.min(times[k])), 4), result=res)
        if args.cpu:
            d, m = clouds[c[0]]
            cloud = d[:3 * m].cpu().numpy().reshape(-1, 3)
            t = time.perf_counter()
            ref = R.cluster(cloud, c[1], c[2])
            out[k]["scipy_restatement_ms"] = round(1e3 * (time.perf_counter() - t), 1)
            out[k]["equal"] = bool(ref["result"] == res and off.tobytes() == ref["offsets"].tobytes())
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
