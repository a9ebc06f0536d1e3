#!/usr/bin/env python3
"""Outlier removal (tdv_remove_statistical_outlier_dev, tdv_remove_radius_outlier_dev) on two clouds, device-resident, mask + index + kept
rows per call, beside two yardsticks run in the same process on the same cloud:
  scene  the bin scene of tests/cluster_restatement.py with the floor taken off by tdv_segment_planes_dev (~24 k points);
  frame  the whole cloud of one 1280x720 depth frame (a floor 1 m from the camera, six box tops, 400 flying pixels): ~920 k points.
  statistical (nb_neighbors 20, std_ratio 2.0)  against  tdv_estimate_normals_dev at k = 20 (the same walk, then PCA and an n x k list);
  radius (nb_points 10 at 10 mm on the scene, 3 mm on the frame)  against  tdv_cluster_dbscan_dev at the same eps, min_points 11.
Per configuration the median and minimum of --repeats alternating rounds in ms per call, and the two ratios.  --buys also measures
what the filter buys ICP on the robust-loss clutter scene with a veil of points between part and floor: point-to-plane L2 on the
whole scan, on the filtered scan, and Tukey alone on the whole scan (pose errors against the ground truth).  Prints one JSON line.

    python tools/bench_outlier.py [--repeats 9] [--buys]
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
    rng = np.random.default_rng(1)
    z[rng.integers(0, H, 400), rng.integers(0, W, 400)] -= rng.uniform(0.1, 0.4, 400)
    return np.round(z * SCALE).astype(np.uint16)


def buys(ctx, synth):
    """ICP on the clutter scene plus a veil: 300 points spread between the part's bottom face and the floor under it."""
    import icp_loss_restatement as IL
    S = IL.SCENE
    src, tgt, nrm, T0, T_gt = IL.clutter_scene(synth)
    rng = np.random.default_rng(5)
    veil = np.stack([rng.uniform(-0.13, 0.13, 300), rng.uniform(-0.08, 0.08, 300), rng.uniform(-0.03 - S["floor_gap"], -0.03, 300)], 1)
    Ti = np.linalg.inv(T_gt.astype(np.float64))
    src = np.concatenate([src, (veil @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)])
    out = {}

    def err(name, cloud):
        r = ctx.icp(cloud, tgt, nrm, T0, S["thr"], S["iterations"], True)
        a, t = synth.pose_error(r.transformation, T_gt)
        out[name] = dict(n=len(cloud), rad=float(a), m=float(t))
    err("l2_whole", src)
    for k, ratio in ((20, 2.0), (20, 1.0)):
        kept, _ = ctx.remove_statistical_outlier(src, k, ratio)
        err("l2_statistical_%d_%g" % (k, ratio), kept)
    kept, _ = ctx.remove_radius_outlier(src, 5, 0.008)
    err("l2_radius_5_8mm", kept)
    ctx.set_icp_loss("tukey", S["tukey_scale"])
    err("tukey_whole", src)
    ctx.set_icp_loss("l2")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--buys", action="store_true", help="also measure ICP on the clutter scene with and without the filter")
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
    clouds["scene"] = (d_rest, n_rest, 0.010)
    d_raw = torch.from_numpy(frame().reshape(-1).view(np.int16).copy()).to(dev)
    d_xyz = torch.zeros(W * H * 3, dtype=torch.float32, device=dev)
    n = ctx.depth_to_cloud_dev(d_raw.data_ptr(), None, None, W, H, SCALE, FX, FY, CX, CY, ZMAX, d_xyz.data_ptr(), None, W * H)
    clouds["frame"] = (d_xyz, n, 0.003)
    torch.cuda.synchronize()

    K, RATIO, NB = 20, 2.0, 10
    n_max = max(c[1] for c in clouds.values())
    d_mask = torch.zeros(n_max, dtype=torch.uint8, device=dev)
    d_ind = torch.zeros(n_max, dtype=torch.int32, device=dev)
    d_out = torch.zeros(3 * n_max, dtype=torch.float32, device=dev)
    d_nrm = torch.zeros(3 * n_max, dtype=torch.float32, device=dev)
    d_knn = torch.zeros(K * n_max, dtype=torch.int32, device=dev)

    def statistical(d, m, eps):
        return ctx.remove_statistical_outlier_dev(d.data_ptr(), m, K, RATIO, d_mask=d_mask.data_ptr(), d_index=d_ind.data_ptr(), d_out_xyz=d_out.data_ptr())

    def normals(d, m, eps):
        ctx.estimate_normals_dev(d.data_ptr(), m, K, d_nrm.data_ptr(), d_knn.data_ptr())

    def radius(d, m, eps):
        return ctx.remove_radius_outlier_dev(d.data_ptr(), m, NB, eps, d_mask=d_mask.data_ptr(), d_index=d_ind.data_ptr(), d_out_xyz=d_out.data_ptr())

    def dbscan(d, m, eps):
        return ctx.cluster_dbscan_dev(d.data_ptr(), m, eps, NB + 1, d_labels=d_ind.data_ptr())[0]

    ops = dict(statistical=statistical, normals=normals, radius=radius, dbscan=dbscan)
    configs = [(c, o) for c in clouds for o in ops]
    info = {}
    for _ in range(2):                                           # warm-up (arena growth, code load) and the counts
        for c, o in configs:
            info[(c, o)] = ops[o](*clouds[c])
    torch.cuda.synchronize()
    times = {k: [] for k in configs}
    for _ in range(args.repeats):
        for k in configs:                                        # alternating, so that a slow phase of the machine hits every one
            t = time.perf_counter()
            ops[k[1]](*clouds[k[0]])
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    out = dict(tool="bench_outlier", repeats=args.repeats, nb_neighbors=K, std_ratio=RATIO, nb_points=NB,
               n_points={k: v[1] for k, v in clouds.items()}, eps={k: v[2] for k, v in clouds.items()})
    for c in clouds:
        med = {o: 1e3 * float(np.median(times[(c, o)])) for o in ops}
        out[c] = {o: dict(ms=round(med[o], 4), min_ms=round(1e3 * float(np.min(times[(c, o)])), 4), max_ms=round(1e3 * float(np.max(times[(c, o)])), 4))
                  for o in ops}
        out[c]["statistical"]["result"] = info[(c, "statistical")]
        out[c]["radius"]["result"] = info[(c, "radius")]
        out[c]["statistical_over_normals"] = round(med["statistical"] / med["normals"], 3)
        out[c]["radius_over_dbscan"] = round(med["radius"] / med["dbscan"], 3)
    if args.buys:
        out["buys"] = buys(ctx, synth)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
