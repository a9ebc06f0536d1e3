#!/usr/bin/env python3
"""ISS keypoints (tdv_iss_keypoints_dev), device-resident, in two parts.  Prints one JSON line.

cost   the call at the default radii (mask, index and the keypoints' rows asked for) on the two clouds of tools/bench_ops.py - the instance
       cloud of one 1280x720 frame of the relief part in pixel order, and the 200,000-point cuboid in random order - beside the yardstick
       run in the same process on the same cloud: tdv_compute_fpfh_dev at radius = the salient radius the call reported (the same kind of
       radius walk; it writes 33 floats per point).  Also the call at those radii GIVEN (no resolution pass).  Median, minimum and maximum
       of --repeats alternating rounds, in ms per call.  The split per kernel comes from a kernel trace of this script (--cost-only keeps
       the trace short).
buys   one instance of tools/bench_batch.py's scene (config C4's shapes: the relief part in its own frame against the model scan): depth ->
       cloud -> voxel -> normals + FPFH on the FULL cloud, then descriptor match + RANSAC + ICP from all source points (`all`), from
       the source's keypoint rows against the whole model (`key`), and from the keypoint rows of both clouds (`both`); FPFH is gathered
       through attr, and ICP refines the full cloud against the full model in every variant.  Per variant: points handed to the match,
       ms of ISS, of the match, of RANSAC and of ICP, RANSAC's fitness over the points it was given, and the pose error against the ground
       truth before and after ICP.  --instances poses, each reported.

    python tools/bench_iss.py [--repeats 9] [--instances 4] [--hyps 10000] [--clouds frame,cuboid] [--cost-only | --buys-only]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _stats(ts):
    return dict(ms=round(1e3 * float(np.median(ts)), 4), min_ms=round(1e3 * float(np.min(ts)), 4), max_ms=round(1e3 * float(np.max(ts)), 4))


def _timed(torch, ops, repeats):
    """Median / min / max seconds of every op over alternating rounds (a slow phase of the machine hits every one), after two warm-ups."""
    info = {}
    for _ in range(2):
        for k, f in ops.items():
            info[k] = f()
    torch.cuda.synchronize()
    times = {k: [] for k in ops}
    for _ in range(repeats):
        for k, f in ops.items():
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    return {k: _stats(v) for k, v in times.items()}, info


def frame_cloud(ctx, synth, torch, dev):
    """tools/opbench.py's voxel_image_order cloud: instance 0 of the relief part, unprojected in row-major pixel order."""
    bb = importlib.import_module("bench_batch")
    px = bb.DIST / bb.F
    part = synth.ReliefPart(3, L=448 * px, W=448 * px, feature=6.0 * 1.2 * px, density=0.09)
    dense = torch.from_numpy(part.surface_points(px / 2.5)).to(dev)
    d_depth, d_mask = synth.render_depth_torch(dense, synth.instance_pose(0, bb.DIST, 30.0), bb.F, bb.F, bb.CX, bb.CY, bb.W, bb.H, bb.SCALE)
    n_px = int((d_mask > 0).sum())
    d_xyz = torch.empty((n_px, 3), dtype=torch.float32, device=dev)
    n = ctx.depth_to_cloud_dev(d_depth.data_ptr(), d_mask.data_ptr(), None, bb.W, bb.H, bb.SCALE, bb.F, bb.F, bb.CX, bb.CY, bb.ZMAX, d_xyz.data_ptr(), None, n_px)
    return d_xyz, n


def cost(ctx, tdv, synth, torch, dev, repeats, which):
    opbench = importlib.import_module("opbench")
    clouds = {}
    if "frame" in which:
        clouds["frame"] = frame_cloud(ctx, synth, torch, dev)
    if "cuboid" in which:
        cam = opbench.cuboid_scene(synth, 200000)[0]
        clouds["cuboid"] = (torch.from_numpy(cam).to(dev), len(cam))
    out = {}
    for name, (d_xyz, n) in clouds.items():
        d_mask = torch.zeros(n, dtype=torch.uint8, device=dev); d_ind = torch.zeros(n, dtype=torch.int32, device=dev)
        d_out = torch.zeros(3 * n, dtype=torch.float32, device=dev); d_nrm = torch.zeros(3 * n, dtype=torch.float32, device=dev)
        d_desc = torch.zeros(33 * n, dtype=torch.float32, device=dev)
        ctx.estimate_normals_dev(d_xyz.data_ptr(), n, 30, d_nrm.data_ptr())

        def iss(**kw):
            return ctx.iss_keypoints_dev(d_xyz.data_ptr(), n, d_mask=d_mask.data_ptr(), d_index=d_ind.data_ptr(), d_out_xyz=d_out.data_ptr(), **kw)
        first = iss()
        radii = dict(salient_radius=first["salient_radius"], non_max_radius=first["non_max_radius"])
        ops = dict(iss_default_radii=iss, iss_given_radii=lambda: iss(**radii),
                   fpfh_at_salient_radius=lambda: ctx.compute_fpfh_dev(d_xyz.data_ptr(), d_nrm.data_ptr(), n, radii["salient_radius"], d_desc.data_ptr(), None, None))
        t, info = _timed(torch, ops, repeats)
        out[name] = dict(n_points=n, result=info["iss_default_radii"], **t)
        out[name]["iss_over_fpfh"] = round(t["iss_default_radii"]["ms"] / t["fpfh_at_salient_radius"]["ms"], 3)
    return out


def buys(ctx, tdv, synth, torch, dev, instances, hyps, repeats):
    bb = importlib.import_module("bench_batch")
    order = tdv.TDV_VOXEL_ORDER_FIRST
    wl = bb.build_workload(tdv, synth, ctx, instances, 1.2, 448, 3, order, dev)
    d_mx, d_mn, d_mf, nm = wl["model"]
    voxel = wl["voxel"]
    rows = []
    for b in range(instances):
        n_px = wl["mask_px"][b]
        d_raw = torch.empty((n_px, 3), dtype=torch.float32, device=dev)
        n_raw = ctx.depth_to_cloud_dev(wl["depth"][b].data_ptr(), wl["masks"][b].data_ptr(), None, bb.W, bb.H, bb.SCALE, bb.F, bb.F, bb.CX, bb.CY, bb.ZMAX,
                                       d_raw.data_ptr(), None, n_px)
        d_src = torch.empty_like(d_raw)
        n = ctx.voxel_downsample_dev(d_raw.data_ptr(), None, n_raw, voxel, d_src.data_ptr(), None, n_raw, order)
        d_nrm = torch.empty((n, 3), dtype=torch.float32, device=dev); d_fs = torch.empty((n, 33), dtype=torch.float32, device=dev)
        ctx.normals_fpfh_dev(d_src.data_ptr(), n, 30, 5.0 * voxel, d_nrm.data_ptr(), d_fs.data_ptr())
        d_kx = torch.empty((n, 3), dtype=torch.float32, device=dev); d_kf = torch.empty((n, 33), dtype=torch.float32, device=dev)
        d_corr = torch.empty(n, dtype=torch.int32, device=dev)
        state = {}

        def iss():
            state["iss"] = ctx.iss_keypoints_dev(d_src.data_ptr(), n, d_fs.data_ptr(), 33, d_out_xyz=d_kx.data_ptr(), d_out_attr=d_kf.data_ptr())
            return state["iss"]
        iss()
        m = state["iss"]["n_keypoints"]

        # the model's keypoints too (what a caller who reduces both clouds hands to the match): computed once, outside the timings
        d_mkx = torch.empty((nm, 3), dtype=torch.float32, device=dev); d_mkf = torch.empty((nm, 33), dtype=torch.float32, device=dev)
        mk = ctx.iss_keypoints_dev(d_mx.data_ptr(), nm, d_mf.data_ptr(), 33, d_out_xyz=d_mkx.data_ptr(), d_out_attr=d_mkf.data_ptr())["n_keypoints"]
        variants = dict(all=(d_src, n, d_fs, d_mx, nm, d_mf), key=(d_kx, m, d_kf, d_mx, nm, d_mf), both=(d_kx, m, d_kf, d_mkx, mk, d_mkf))

        def match(key):
            d_pts, count, d_feat, d_t, nt, d_tf = variants[key]
            return lambda: ctx.feature_match_dev(d_feat.data_ptr(), count, d_tf.data_ptr(), nt, d_corr.data_ptr())

        def ransac(key):
            d_pts, count, d_feat, d_t, nt, d_tf = variants[key]

            def f():
                match(key)()                                     # d_corr is shared: each variant's own matches, outside ITS timing below
                torch.cuda.synchronize(); t = time.perf_counter()
                state[key] = ctx.ransac_dev(d_pts.data_ptr(), count, d_t.data_ptr(), nt, None, None, d_corr.data_ptr(), voxel, hyps, 0.999, 42)
                torch.cuda.synchronize()
                state.setdefault(key + "_ransac_s", []).append(time.perf_counter() - t)
                return state[key]
            return f

        def refine(key):
            def f():
                state[key + "_icp"] = ctx.icp_dev(d_src.data_ptr(), n, d_mx.data_ptr(), d_mn.data_ptr(), nm, state[key].transformation, 0.4 * voxel, 50, True)
                return state[key + "_icp"]
            return f
        ops = dict(iss=iss)
        for key in variants:
            ops[key + "_match"] = match(key)
            ops[key + "_match_ransac"] = ransac(key)
        t, _ = _timed(torch, ops, repeats)
        t2, _ = _timed(torch, {key + "_icp": refine(key) for key in variants}, repeats)
        t.update(t2)
        ms = {k: v["ms"] for k, v in t.items()}
        for key in variants:
            ms[key + "_ransac"] = round(1e3 * float(np.median(state[key + "_ransac_s"][2:])), 4)      # (the two warm-ups dropped)
        row = dict(instance=b, n_voxels=n, n_keypoints=m, model_keypoints=mk, iss_result=state["iss"], ms=ms)
        for key, v in variants.items():
            c, r = state[key], state[key + "_icp"]
            a0, t0 = synth.pose_error(c.transformation, wl["T_gt"][b])
            a1, t1 = synth.pose_error(r.transformation, wl["T_gt"][b])
            row[key] = dict(points=v[1], targets=v[4], coarse_fitness=float(c.fitness), coarse_inliers=int(c.inliers), iterations_run=int(c.iterations_run),
                            coarse_rad=float(a0), coarse_m=float(t0), icp_fitness=float(r.fitness), icp_rad=float(a1), icp_m=float(t1),
                            icp_iterations=int(r.iterations))
        rows.append(row)
    return dict(voxel_m=voxel, model_points=nm, hyps=hyps, instances=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--instances", type=int, default=4)
    ap.add_argument("--hyps", type=int, default=10000)
    ap.add_argument("--clouds", default="frame,cuboid", help="the clouds of the cost part (a kernel trace of one cloud at a time splits the call per kernel)")
    ap.add_argument("--cost-only", action="store_true")
    ap.add_argument("--buys-only", action="store_true")
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)
    out = dict(tool="bench_iss", repeats=args.repeats)
    if not args.buys_only:
        out["cost"] = cost(ctx, tdv, synth, torch, dev, args.repeats, args.clouds.split(","))
    if not args.cost_only:
        out["buys"] = buys(ctx, tdv, synth, torch, dev, args.instances, args.hyps, args.repeats)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
