#!/usr/bin/env python3
"""TSDF ray casting and frame-to-model tracking (tdv_tsdf_raycast_dev / tdv_tsdf_track_dev / tdv_tsdf_track_sequence_dev,
include/tdv_hip.h): what a view of the volume costs beside the route the library had for the same image before, what tracking a frame
against the volume costs beside frame-to-frame odometry, and what it does to a sequence's drift.  Prints one JSON line per step.
Without --step every step runs in a child process of its own under its own time limit, in order, and the first that fails ends the run:
nothing is tried again.

  raycast   profiles/r24/tsdf.md's volume - 400 x 300 x 200 voxels of 1 mm around a 360 x 260 mm relief plate - fused from four 1280 x 720
            views a degree apart, seen from the pose of a fifth: depth only (no read-back), all three maps, and the earlier route to a
            depth image, tdv_tsdf_extract_dev followed by tdv_render_depth_dev (splat 1 and splat 3).  zmax is 1 m: the plate sits at
            0.6 m, and a ray that misses walks to zmax.  Samples per ray, and the share of rays that end at the step cap or beyond zmax,
            come from the restatement on a 320 x 180 view of the same field (tests/tsdf_raycast_restatement.py; the device's image of that
            view is compared with it byte for byte).  The bytes per second are the bytes the samples ask for - 64 per sample, eight
            pairs - over the call's median: requests, most of them served by the caches, not HBM traffic; beside bench.py's HBM_PEAK_GBPS.
  track     the fifth frame against that volume from the fourth's pose (tdv_tsdf_track_dev) beside tdv_depth_odometry_dev on frames
            five and four, and both routes' pose errors against the render's ground truth.
  sequence  64 frames of 160 x 120 of the small part, a quarter of a degree apart, into 80 x 48 x 32 voxels:
            tdv_tsdf_track_sequence_dev beside tdv_depth_odometry_sequence_dev plus one tdv_tsdf_integrate_dev call with all frames.
  drift     tools/bench_odometry.py's eleven views of the relief part, 2.5 degrees apart: the final pose's error and the fused surface's
            distance to the true one for the true poses, the frame-to-frame chain and frame-to-model tracking, both from the identity.

Every timed call is timed on the host up to a synchronise, alternating between the variants of a step, median / min / max over
--repeats rounds after a warm-up.

    python tools/bench_tsdf_raycast.py [--repeats 7] [--step raycast|track|sequence|drift]
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
STEPS = (("raycast", 420), ("track", 300), ("sequence", 300), ("drift", 300))      # (step, its time limit in seconds)
DIMS, VOXEL, ORIGIN = (400, 300, 200), 0.001, (-0.2, -0.15, -0.08)
SIZE, FOCAL, DISTANCE = (1280, 720), 1500.0, 0.6
AXIS = [0.3, 1.0, 0.2]
ZMAX = 1.0
SOT = "source_onto_target"


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


def up(torch, a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def camera_poses(views):
    """MODEL_TO_CAMERA view poses as the cameras' poses in the model's frame (float64)."""
    return np.stack([np.linalg.inv(np.asarray(P, np.float64)) for P in views])


def plate_scene(ctx, torch, n=5):
    """n views of the plate a degree apart, the first n - 1 fused at their true poses: dict(frames, d_raw, intr, cam, vol, poses)."""
    import tsdf_cases as Cs
    part = Cs.synth.ReliefPart(seed=3, L=0.36, W=0.26)
    views = Cs.view_poses(DISTANCE, [(AXIS, float(k)) for k in range(n)])
    frames, intr = Cs.render(part.surface_points(0.0002), views, FOCAL, *SIZE)
    cam = camera_poses(views)
    d_raw = up(torch, frames)
    vol = ctx.tsdf_volume(ORIGIN, VOXEL, DIMS)
    ctx.tsdf_integrate_dev(vol[0], vol[1].data_ptr(), d_raw.data_ptr(), cam[:n - 1].astype(F), *SIZE, *intr, want_counts=False, pose_direction=SOT)
    ctx.synchronize()
    return dict(frames=frames, d_raw=d_raw, intr=intr, cam=cam, vol=vol)


def step_raycast(tdv, torch, ctx, repeats):
    import bench
    import tsdf_raycast_restatement as R
    import tsdf_restatement as Ts
    s = plate_scene(ctx, torch)
    (cvol, d_vol), intr = s["vol"], s["intr"]
    w, h = SIZE
    pose = s["cam"][4].astype(F)
    kw = dict(zmax=ZMAX, pose_direction=SOT)
    out = torch.zeros((7, w * h), dtype=torch.float32, device=d_vol.device)
    m, _ = ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), None, None, 0)
    rows = torch.zeros((max(m, 1), 3), dtype=torch.float32, device=d_vol.device)
    torch.cuda.synchronize()
    to_camera = np.linalg.inv(s["cam"][4]).astype(F)                                # the splat takes the model to the camera
    state = {}

    def splat(k):
        def run():
            n, _ = ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), rows.data_ptr(), None, m)
            state["rendered_%d" % k] = ctx.render_depth_dev(rows.data_ptr(), n, to_camera, w, h, *intr[1:], out[0].data_ptr(), splat=k, zmax=ZMAX,
                                                            pose_direction="model_to_camera")
        return run

    def count():
        state["n_hit"] = ctx.tsdf_raycast_dev(cvol, d_vol.data_ptr(), pose, w, h, *intr[1:], out[0].data_ptr(), **kw)

    t = _median_ms(torch, {
        "raycast_depth": lambda: ctx.tsdf_raycast_dev(cvol, d_vol.data_ptr(), pose, w, h, *intr[1:], out[0].data_ptr(), want_count=False, **kw),
        "raycast_depth_count": count,
        "raycast_three_maps": lambda: ctx.tsdf_raycast_dev(cvol, d_vol.data_ptr(), pose, w, h, *intr[1:], out[0].data_ptr(), out[1].data_ptr(),
                                                           out[4].data_ptr(), want_count=False, **kw),
        "extract_then_splat_1": splat(1), "extract_then_splat_3": splat(3)}, repeats)
    # samples per ray from the restatement, on a quarter-size view of the same field; the device's image of that view, byte for byte
    qs, qcam = (w // 4, h // 4), (intr[1] / 4, intr[2] / 4, (intr[3] - 1.5) / 4, (intr[4] - 1.5) / 4)
    buf = d_vol.cpu().numpy().reshape(DIMS[2], DIMS[1], DIMS[0], 2)
    ref = R.raycast(Ts.Volume(ORIGIN, VOXEL, DIMS), buf, pose, qs, qcam, normals=False, zmax=ZMAX, pose_direction=Ts.SOURCE_ONTO_TARGET)
    small = torch.zeros(qs[0] * qs[1], dtype=torch.float32, device=d_vol.device)
    torch.cuda.synchronize()
    ctx.tsdf_raycast_dev(cvol, d_vol.data_ptr(), pose, *qs, *qcam, small.data_ptr(), want_count=False, **kw)
    ctx.synchronize()
    mean = float(ref["samples"].mean())
    asked = 64.0 * mean * w * h
    return dict(volume=dict(dims=DIMS, voxel_mm=1e3 * VOXEL, bytes=8 * DIMS[0] * DIMS[1] * DIMS[2]), image=SIZE, zmax=ZMAX, crossings=m,
                n_hit=state["n_hit"], rendered_splat_1=state["rendered_1"], rendered_splat_3=state["rendered_3"], **t,
                quarter_view=dict(size=qs, same_bytes_as_restatement=bool(small.cpu().numpy().tobytes() == ref["depth"].tobytes()),
                                  mean_samples_per_ray=round(mean, 2), mean_samples_of_hits=round(float(ref["samples"][ref["depth"] > 0].mean()), 2),
                                  share_hit=round(float((ref["depth"] > 0).mean()), 4), share_ended_at_cap=round(float(ref["capped"].mean()), 4),
                                  share_ended_beyond_zmax=round(float(ref["far"].mean()), 4)),
                bytes_asked_for=asked, asked_gbps_depth_only=round(asked / (1e-3 * t["raycast_depth"]["median_ms"]) / 1e9, 1),
                hbm_peak_gbps=bench.HBM_PEAK_GBPS)


def step_track(tdv, torch, ctx, repeats):
    import odometry_cases as K
    s = plate_scene(ctx, torch)
    (cvol, d_vol), intr, cam = s["vol"], s["intr"], s["cam"]
    w, h = SIZE
    fb = 2 * w * h
    d4, d3 = s["d_raw"].data_ptr() + 4 * fb, s["d_raw"].data_ptr() + 3 * fb
    guess = cam[3].astype(F)
    state = {}

    def track():
        state["track"] = ctx.tsdf_track_dev(cvol, d_vol.data_ptr(), d4, guess, w, h, *intr, tsdf=dict(zmax=ZMAX))

    def pair():
        state["pair"] = ctx.depth_odometry_dev(d4, d3, w, h, *intr)

    t = _median_ms(torch, {"track_against_volume": track, "odometry_frame_to_frame": pair}, repeats)
    tr, pr = state["track"], state["pair"]
    e0, et = K.errors(guess, cam[4]), K.errors(tr["pose"], cam[4])
    ep = K.errors(cam[3] @ np.asarray(pr["T"], np.float64), cam[4])
    return dict(image=SIZE, **t,
                track=dict(n_hit=tr["n_hit"], iterations=tr["odom"]["iterations"], n_corr=tr["odom"]["n_corr"], rotation_error_deg=round(et[0], 5),
                           translation_error_mm=round(1e3 * et[1], 4)),
                frame_to_frame=dict(iterations=pr["iterations"], n_corr=pr["n_corr"], rotation_error_deg=round(ep[0], 5),
                                    translation_error_mm=round(1e3 * ep[1], 4)),
                guess=dict(rotation_error_deg=round(e0[0], 5), translation_error_mm=round(1e3 * e0[1], 4)))


def step_sequence(tdv, torch, ctx, repeats):
    import odometry_cases as K
    import tsdf_cases as Cs
    n, size, f, step = 64, (160, 120), 420.0, 0.25
    pts = Cs.synth.ReliefPart(seed=3, L=0.06, W=0.03, feature=0.006).surface_points(0.0002)
    views = Cs.view_poses(0.3, [(AXIS, step * k) for k in range(n)])
    frames, intr = Cs.render(pts, views, f, *size)
    cam = camera_poses(views)
    w, h = size
    d = up(torch, frames)
    vol_args = ((-0.04, -0.024, -0.0096), 0.001, (80, 48, 32))
    va, vb = ctx.tsdf_volume(*vol_args), ctx.tsdf_volume(*vol_args)
    kw = dict(depth_diff=0.01)
    state = {}

    def tracked():
        ctx.tsdf_reset_dev(va[0], va[1].data_ptr())
        state["track"] = ctx.tsdf_track_sequence_dev(va[0], va[1].data_ptr(), d.data_ptr(), n, w, h, *intr, pose0=cam[0].astype(F),
                                                     tsdf=dict(zmax=ZMAX), odom=kw)

    def chained():
        ctx.tsdf_reset_dev(vb[0], vb[1].data_ptr())
        poses, _ = ctx.depth_odometry_sequence_dev(d.data_ptr(), n, w, h, *intr, **kw)
        world = np.stack([cam[0] @ P.astype(np.float64) for P in poses]).astype(F)
        ctx.tsdf_integrate_dev(vb[0], vb[1].data_ptr(), d.data_ptr(), world, w, h, *intr, want_counts=False, zmax=ZMAX, pose_direction=SOT)
        state["chain"] = world

    t = _median_ms(torch, {"track_sequence": tracked, "odometry_sequence_then_integrate": chained}, repeats)
    et, ec = K.errors(state["track"][0][-1], cam[-1]), K.errors(state["chain"][-1], cam[-1])
    return dict(frames=n, image=size, volume=vol_args[2], **t, ms_per_frame_tracked=round(t["track_sequence"]["median_ms"] / n, 4),
                last_pose_motion_deg=step * (n - 1),
                track_sequence_last_pose=dict(rotation_error_deg=round(et[0], 4), translation_error_mm=round(1e3 * et[1], 3)),
                chain_last_pose=dict(rotation_error_deg=round(ec[0], 4), translation_error_mm=round(1e3 * ec[1], 3)),
                hits_per_frame_min=int(min(r["n_hit"] for r in state["track"][1][1:])))


def step_drift(tdv, torch, ctx, repeats):
    import odometry_cases as K
    import tsdf_cases as Cs
    sc = Cs.relief_scene()
    part = sc["part"]
    n = 11
    views = Cs.view_poses(0.4, [([1.0, 0.0, 0.0], 2.5 * k) for k in range(n)])
    frames, intr = Cs.render(part.surface_points(0.0003), views, 1400.0, 640, 480)
    true = np.stack([K.truth(views[k], views[0]) for k in range(n)])                 # camera k in camera 0's frame
    d = up(torch, frames)
    vol_args = ((-0.068, -0.048, 0.376), 0.001, (136, 96, 40))
    kw = dict(depth_diff=0.01)
    chain, _ = ctx.depth_odometry_sequence_dev(d.data_ptr(), n, 640, 480, *intr, **kw)
    vt = ctx.tsdf_volume(*vol_args)
    tracked, res = ctx.tsdf_track_sequence_dev(vt[0], vt[1].data_ptr(), d.data_ptr(), n, 640, 480, *intr, tsdf=dict(zmax=ZMAX), odom=kw)
    to_part = np.linalg.inv(np.asarray(views[0], np.float64))                         # camera 0 -> the part's frame
    out = dict(frames=n, step_deg=2.5, start="identity", hits_per_frame=[r["n_hit"] for r in res[1:]],
               track_iterations=[r["odom"]["iterations"] for r in res[1:]])
    for name, P in (("true_poses", true.astype(F)), ("frame_to_frame_chain", chain), ("frame_to_model_tracking", tracked)):
        if name == "frame_to_model_tracking":
            vol = vt                                                                # the volume the tracked sequence fused itself
        else:
            vol = ctx.tsdf_volume(*vol_args)
            ctx.tsdf_integrate_dev(vol[0], vol[1].data_ptr(), d.data_ptr(), P, 640, 480, *intr, want_counts=False, zmax=ZMAX, pose_direction=SOT)
        xyz, _ = ctx.tsdf_extract(vol)
        p = xyz.astype(np.float64) @ to_part[:3, :3].T + to_part[:3, 3]
        inside = (np.abs(p[:, 0]) < part.L / 2 - 0.002) & (np.abs(p[:, 1]) < part.W / 2 - 0.002)
        hgt, _ = Cs.true_surface(part, p[inside])
        dist = np.abs(p[inside, 2] - hgt)
        errs = [K.errors(P[k], true[k]) for k in range(1, n)]
        out[name] = dict(crossings=int(len(xyz)), mean_distance_mm=round(1e3 * float(dist.mean()), 4), median_distance_mm=round(1e3 * float(np.median(dist)), 4),
                         p90_distance_mm=round(1e3 * float(np.quantile(dist, 0.9)), 4),
                         final_rotation_error_deg=round(errs[-1][0], 4), final_translation_error_mm=round(1e3 * errs[-1][1], 4),
                         worst_rotation_error_deg=round(max(e[0] for e in errs), 4), worst_translation_error_mm=round(1e3 * max(e[1] for e in errs), 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step", type=str, default="")
    args = ap.parse_args()
    if not args.step:
        for step, limit in STEPS:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--repeats", str(args.repeats)], timeout=limit)
            if r.returncode != 0:
                raise SystemExit("bench_tsdf_raycast.py: step %s ended with status %d; the later steps were not run" % (step, r.returncode))
        return
    import torch
    tdv = importlib.import_module("3dvision_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_raycast.py measures on the GPU: no device")
    ctx = tdv.Context(0)
    res = {"raycast": step_raycast, "track": step_track, "sequence": step_sequence, "drift": step_drift}[args.step](tdv, torch, ctx, args.repeats)
    ctx.close()
    print(json.dumps(dict(tool="bench_tsdf_raycast", step=args.step, repeats=args.repeats, **{args.step: res})), flush=True)


if __name__ == "__main__":
    main()
