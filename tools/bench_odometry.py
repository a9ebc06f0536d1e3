#!/usr/bin/env python3
"""Depth odometry (tdv_depth_maps_dev / tdv_depth_odometry_dev / tdv_depth_odometry_sequence_dev, include/tdv_hip.h): what the maps, a
pair and a sequence cost, beside the route the library had for the same pair before, and what the poses buy a fusion.  Prints one JSON
line per step.  Without --step every step runs in a child process of its own under its own time limit, in order, and the first that
fails ends the run: nothing is tried again.

  maps      tdv_depth_maps_dev at 640 x 480 and 1280 x 720: maps only (no read-back) and maps + rows + count.
  pair      one pair at both sizes, default params, from the identity: the whole call, and per applied iteration; beside it the route of
            the library without odometry - tdv_depth_to_cloud_dev x 2, tdv_estimate_normals_dev (k = 30) on the target's cloud,
            tdv_icp_dev point-to-plane with the same start, threshold = depth_diff and the same iteration budget (35) - and both
            routes' pose errors against the render's ground truth.
  sequence  8 frames of 640 x 480 and 64 frames of 160 x 120 in one call against the same pairs as single calls; same bytes or not.
  fusion    tests/tsdf_cases.py's relief part from 0.4 m, eleven views in steps of 2.5 degrees about x, fused (volume in camera 0's
            frame, pose_direction source_onto_target) with the true poses, with poses perturbed by 1 degree / 5 mm, and with
            tdv_depth_odometry_sequence_dev's h_poses started from the perturbed ones, handed to tdv_tsdf_integrate_dev unchanged: the
            crossings' distance to the true surface for each.

Every timed call is timed on the host up to a synchronise, alternating between the variants of a step, median / min / max over
--repeats rounds after a warm-up.  The scene of maps and pair: a 360 x 260 mm relief plate from 0.6 m, the second view turned by 1
degree about (0.3, 1, 0.2).

    python tools/bench_odometry.py [--repeats 9] [--step maps|pair|sequence|fusion]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32
STEPS = (("maps", 240), ("pair", 300), ("sequence", 300), ("fusion", 300))      # (step, its time limit in seconds)
SIZES = {(640, 480): 750.0, (1280, 720): 1500.0}
AXIS = [0.3, 1.0, 0.2]


def _median_ms(torch, runs, repeats):
    for f in runs.values():           # warm-up: arena growth, code load
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, f in runs.items():     # alternating, so that a slow phase of the machine hits every one
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t))
    return {k: dict(median_ms=round(float(np.median(v)), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in times.items()}


def plate_pair(size):
    """Two views of the plate, 1 degree apart: dict(frames, intr, T_gt)."""
    import odometry_cases as K
    import tsdf_cases as Cs
    part = Cs.synth.ReliefPart(seed=3, L=0.36, W=0.26)
    poses = Cs.view_poses(0.6, [(AXIS, 0.0), (AXIS, 1.0)])
    frames, intr = Cs.render(part.surface_points(0.0003 if size[0] <= 640 else 0.0002), poses, SIZES[size], *size)
    return dict(frames=frames, intr=intr, T_gt=K.truth(poses[1], poses[0]))


def up(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def step_maps(tdv, torch, ctx, repeats):
    out = {}
    for size in SIZES:
        s = plate_pair(size)
        w, h = size
        d = up(torch, s["frames"][0])
        buf = torch.zeros((4, w * h, 3), dtype=torch.float32, device=d.device)
        torch.cuda.synchronize()
        n, _ = ctx.depth_maps_dev(d.data_ptr(), w, h, *s["intr"])
        t = _median_ms(torch, {
            "maps_only": lambda: ctx.depth_maps_dev(d.data_ptr(), w, h, *s["intr"], buf[0].data_ptr(), buf[1].data_ptr(), want_count=False),
            "maps_rows_count": lambda: ctx.depth_maps_dev(d.data_ptr(), w, h, *s["intr"], buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(),
                                                          buf[3].data_ptr(), w * h)}, repeats)
        out["%dx%d" % size] = dict(rows=n, bytes_in=2 * w * h, bytes_out_maps=24 * w * h, bytes_out_rows=24 * n, **t)
    return out


def step_pair(tdv, torch, ctx, repeats):
    import odometry_cases as K
    out = {}
    for size in SIZES:
        s = plate_pair(size)
        w, h = size
        scale, fx, fy, cx, cy = s["intr"]
        d_src, d_tgt = up(torch, s["frames"][1]), up(torch, s["frames"][0])
        prm = tdv.odometry_params()
        budget = sum(prm.max_iterations)
        clouds = torch.zeros((3, w * h, 3), dtype=torch.float32, device=d_src.device)
        torch.cuda.synchronize()
        state = {}

        def odometry():
            state["odo"] = ctx.depth_odometry_dev(d_src.data_ptr(), d_tgt.data_ptr(), w, h, *s["intr"])

        def cloud_route():
            ns = ctx.depth_to_cloud_dev(d_src.data_ptr(), None, None, w, h, scale, fx, fy, cx, cy, prm.zmax, clouds[0].data_ptr(), None, w * h)
            nt = ctx.depth_to_cloud_dev(d_tgt.data_ptr(), None, None, w, h, scale, fx, fy, cx, cy, prm.zmax, clouds[1].data_ptr(), None, w * h)
            ctx.estimate_normals_dev(clouds[1].data_ptr(), nt, 30, clouds[2].data_ptr(), None)
            state["icp"] = ctx.icp_dev(clouds[0].data_ptr(), ns, clouds[1].data_ptr(), clouds[2].data_ptr(), nt, np.eye(4, dtype=F), prm.depth_diff,
                                       budget, True)
            state["n"] = (ns, nt)

        t = _median_ms(torch, {"odometry": odometry, "cloud_normals_icp": cloud_route}, repeats)
        odo, icp = state["odo"], state["icp"]
        its = sum(odo["iterations"])
        e0, eo, ei = K.errors(np.eye(4), s["T_gt"]), K.errors(odo["T"], s["T_gt"]), K.errors(icp.transformation, s["T_gt"])
        out["%dx%d" % size] = dict(
            odometry=dict(t["odometry"], iterations=odo["iterations"], n_corr_level=odo["n_corr_level"],
                          median_ms_per_applied_iteration=round(t["odometry"]["median_ms"] / max(its, 1), 4),
                          rotation_error_deg=round(eo[0], 5), translation_error_mm=round(1e3 * eo[1], 4)),
            cloud_normals_icp=dict(t["cloud_normals_icp"], points=state["n"], iterations=int(icp.iterations), iteration_budget=budget,
                                   rotation_error_deg=round(ei[0], 5), translation_error_mm=round(1e3 * ei[1], 4)),
            identity=dict(rotation_error_deg=round(e0[0], 5), translation_error_mm=round(1e3 * e0[1], 4)))
    return out


def step_sequence(tdv, torch, ctx, repeats):
    import odometry_cases as K
    import tsdf_cases as Cs
    out = {}
    plate = Cs.synth.ReliefPart(seed=3, L=0.36, W=0.26).surface_points(0.0003)
    small = Cs.synth.ReliefPart(seed=3, L=0.06, W=0.03, feature=0.006).surface_points(0.0002)
    for name, pts, size, f, dist, n, step in (("8x640x480", plate, (640, 480), 750.0, 0.6, 8, 0.5), ("64x160x120", small, (160, 120), 420.0, 0.3, 64, 0.25)):
        poses = Cs.view_poses(dist, [(AXIS, step * k) for k in range(n)])
        frames, intr = Cs.render(pts, poses, f, *size)
        w, h = size
        d = up(torch, frames)
        kw = dict(depth_diff=0.01)
        state = {}

        def one_call():
            state["seq"] = ctx.depth_odometry_sequence_dev(d.data_ptr(), n, w, h, *intr, **kw)

        def single_calls():
            state["single"] = [ctx.depth_odometry_dev(d.data_ptr() + 2 * w * h * k, d.data_ptr() + 2 * w * h * (k - 1), w, h, *intr, **kw)
                               for k in range(1, n)]

        t = _median_ms(torch, {"one_call": one_call, "single_calls": single_calls}, repeats)
        pairs = state["seq"][1]
        same = all(pairs[k]["T"].tobytes() == state["single"][k - 1]["T"].tobytes() and pairs[k]["iterations"] == state["single"][k - 1]["iterations"]
                   for k in range(1, n))
        err = [K.errors(state["seq"][0][k], K.truth(poses[k], poses[0])) for k in range(1, n)]
        out[name] = dict(t, pairs=n - 1, same_bytes_as_single_calls=bool(same), iterations_total=int(sum(sum(p["iterations"]) for p in pairs)),
                         one_call_faster_by_more_than_the_spread=bool(t["single_calls"]["min_ms"] > t["one_call"]["max_ms"]),
                         last_pose_rotation_error_deg=round(err[-1][0], 4), last_pose_translation_error_mm=round(1e3 * err[-1][1], 3),
                         last_pose_motion_deg=step * (n - 1))
    return out


def step_fusion(tdv, torch, ctx, repeats):
    import odometry_cases as K
    import tsdf_cases as Cs
    sc = Cs.relief_scene()
    part = sc["part"]
    n = 11
    views = Cs.view_poses(0.4, [([1.0, 0.0, 0.0], 2.5 * k) for k in range(n)])
    frames, intr = Cs.render(part.surface_points(0.0003), views, 1400.0, 640, 480)
    true = np.stack([K.truth(views[k], views[0]) for k in range(n)])                 # camera k in camera 0's frame
    pert = np.stack([true[0]] + [Cs.synth.perturb(true[k], seed=k, angle_deg=1.0, trans=0.005) for k in range(1, n)]).astype(np.float64)
    init = np.stack([np.eye(4)] + [np.linalg.inv(pert[k - 1]) @ pert[k] for k in range(1, n)]).astype(F)
    d = up(torch, frames)
    poses, pairs = ctx.depth_odometry_sequence_dev(d.data_ptr(), n, 640, 480, *intr, init=init, depth_diff=0.01)
    to_part = np.linalg.inv(np.asarray(views[0], np.float64))                         # camera 0 -> the part's frame
    out = dict(frames=n, step_deg=2.5)
    for name, P in (("true_poses", true.astype(F)), ("perturbed_poses", pert.astype(F)), ("odometry_poses", poses)):
        vol = ctx.tsdf_volume((-0.068, -0.048, 0.376), 0.001, (136, 96, 40))
        ctx.tsdf_integrate_dev(vol[0], vol[1].data_ptr(), d.data_ptr(), P, 640, 480, *intr, want_counts=False, pose_direction="source_onto_target")
        xyz, _ = ctx.tsdf_extract(vol)
        p = xyz.astype(np.float64) @ to_part[:3, :3].T + to_part[:3, 3]
        inside = (np.abs(p[:, 0]) < part.L / 2 - 0.002) & (np.abs(p[:, 1]) < part.W / 2 - 0.002)
        hgt, _ = Cs.true_surface(part, p[inside])
        dist = np.abs(p[inside, 2] - hgt)
        errs = [K.errors(P[k], true[k]) for k in range(1, n)]
        out[name] = dict(crossings=int(len(xyz)), mean_distance_mm=round(1e3 * float(dist.mean()), 4), median_distance_mm=round(1e3 * float(np.median(dist)), 4),
                         p90_distance_mm=round(1e3 * float(np.quantile(dist, 0.9)), 4),
                         worst_rotation_error_deg=round(max(e[0] for e in errs), 4), worst_translation_error_mm=round(1e3 * max(e[1] for e in errs), 4))
    out["pairs_iterations"] = [p["iterations"] for p in pairs[1:]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--step", type=str, default="")
    args = ap.parse_args()
    if not args.step:
        for step, limit in STEPS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--repeats", str(args.repeats)], timeout=limit)
            if r.returncode != 0:
                raise SystemExit("bench_odometry.py: step %s ended with status %d; the later steps were not run" % (step, r.returncode))
        return
    import torch
    tdv = importlib.import_module("3dvision_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_odometry.py measures on the GPU: no device")
    ctx = tdv.Context(0)
    res = {"maps": step_maps, "pair": step_pair, "sequence": step_sequence, "fusion": step_fusion}[args.step](tdv, torch, ctx, args.repeats)
    ctx.close()
    print(json.dumps(dict(tool="bench_odometry", step=args.step, repeats=args.repeats, **{args.step: res})), flush=True)


if __name__ == "__main__":
    main()
