#!/usr/bin/env python3
"""TSDF fusion (tdv_tsdf_integrate_dev / tdv_tsdf_extract_dev, include/tdv_hip.h): what a pass over a working-size volume costs, what the
frames of a call share, and what the fused cloud holds.  Prints one JSON line.

The scene: a 360 x 260 mm relief plate (synth.ReliefPart, bumps of 11 mm) in a volume of 400 x 300 x 200 voxels of 1 mm (24 M voxels,
192 MB), seen in eight 1280 x 720 frames from 0.6 m at f = 1500: the scan pose and seven tilts of up to 25 degrees about x and y.

  integrate  1, 4 and 8 frames in one call against the same frames as single-frame calls, alternating, every call timed on the host up to
             a synchronise (no read-back in the call: want_counts=False).  Per count: median, minimum and maximum in ms over --repeats
             rounds after a warm-up; the voxels at least one of the frames updates (counted on a fresh volume) and the bytes per second
             that 16 bytes - one load and one store of the pair - per such voxel over the median amount to, beside bench.py's
             HBM_PEAK_GBPS.  The call is an upload of the poses, a memset and one launch: the rate is the call's, the kernel's own time
             comes from a `rocprofv3 --kernel-trace --stats` run of this tool.
  ab         with TDV_LIB_VARIANT=study: the same calls with one voxel row per wave (csrc/tsdf.hip: k_tsdf_integrate<1>, the A/B that lost)
             alternating with the product's eight rows per wave, and whether both leave the same bytes.
  extract    the crossings of the eight-frame volume with and without normals: the whole call (count pass, scan, one read-back, rows).
  host       the numpy restatement (tests/tsdf_restatement.py) of the eight-frame call and of the extraction on the host, and whether
             the device wrote the same bytes (volume, counts, points, normals).
  views      crossings from 1, 4 and 8 views.

    python tools/bench_tsdf.py [--repeats 9] [--skip host]
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
F = np.float32
DIMS, VOXEL = (400, 300, 200), 0.001
SIZE, FOCAL, DISTANCE = (1280, 720), 1500.0, 0.6
TILTS = (([1.0, 0.0, 0.0], 0.0), ([1.0, 0.0, 0.0], 25.0), ([1.0, 0.0, 0.0], -25.0), ([0.0, 1.0, 0.0], 25.0), ([0.0, 1.0, 0.0], -25.0),
         ([1.0, 1.0, 0.0], 15.0), ([1.0, -1.0, 0.0], 15.0), ([1.0, 1.0, 0.0], -15.0))


def build_scene():
    import tsdf_cases as Cs
    import tsdf_restatement as R
    part = Cs.synth.ReliefPart(seed=3, L=0.36, W=0.26)
    poses = Cs.view_poses(DISTANCE, TILTS)
    frames, intr = Cs.render(part.surface_points(0.0002), poses, FOCAL, *SIZE)
    vol = R.Volume((-0.2, -0.15, -0.08), VOXEL, DIMS)
    return dict(part=part, vol=vol, frames=frames, poses=poses, intr=intr)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--skip", type=str, default="")
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf.py measures on the GPU: no device")
    import bench
    import tsdf_restatement as R
    skip = set(args.skip.split(",")) if args.skip else set()
    s = build_scene()
    vol, frames, poses, intr = s["vol"], s["frames"], s["poses"], s["intr"]
    h, w = frames.shape[1:]
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)
    cvol, d_vol = ctx.tsdf_volume(*vol.args())
    d_raw = torch.from_numpy(frames.view(np.int16).copy()).to(dev)
    torch.cuda.synchronize()
    frame_bytes = w * h * 2

    def integrate(a, e, counts=False):
        return ctx.tsdf_integrate_dev(cvol, d_vol.data_ptr(), d_raw.data_ptr() + a * frame_bytes, poses[a:e], w, h, *intr, want_counts=counts)

    def fused(n):
        integrate(0, n)
        ctx.synchronize()

    def single(n):
        for k in range(n):
            integrate(k, k + 1)
        ctx.synchronize()

    res = dict(volume=dict(dims=DIMS, voxel_mm=1e3 * VOXEL, voxels=vol.voxels, bytes=vol.voxels * 8), frames=dict(size=SIZE, f=FOCAL, count=len(frames)))
    runs = {}
    def one_row(n):
        os.environ["TDV_TSDF_ONE_ROW"] = "1"
        try:
            fused(n)
        finally:
            os.environ.pop("TDV_TSDF_ONE_ROW", None)

    for n in (1, 4, 8):
        runs[("one_call", n)] = lambda n=n: fused(n)
        runs[("single_frame_calls", n)] = lambda n=n: single(n)
        if tdv.STUDY_BUILD:
            runs[("one_row_per_wave", n)] = lambda n=n: one_row(n)
    t = _median_ms(torch, runs, args.repeats)
    rows, crossings, device_out = [], {}, {}
    for n in (1, 4, 8):
        ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
        counts = integrate(0, n, counts=True)
        touched = int((d_vol[:, 1] > 0).sum().item())
        one = t[("one_call", n)]
        rows.append(dict(frames=n, one_call=one, single_frame_calls=t[("single_frame_calls", n)], updated_per_frame=counts.tolist(),
                         voxels_updated=touched, floor_bytes=16 * touched, achieved_gbps=round(16 * touched / (1e-3 * one["median_ms"]) / 1e9, 1),
                         one_call_faster_by_more_than_the_spread=bool(t[("single_frame_calls", n)]["min_ms"] > one["max_ms"])))
        if tdv.STUDY_BUILD:
            ab = t[("one_row_per_wave", n)]
            rows[-1]["one_row_per_wave"] = dict(ab, product_faster_by_more_than_the_spread=bool(ab["min_ms"] > one["max_ms"]))
        xyz, nrm = ctx.tsdf_extract((cvol, d_vol))
        crossings[n] = len(xyz)
        if n == 8:
            device_out = dict(volume=d_vol.cpu().numpy().reshape(vol.nz, vol.ny, vol.nx, 2), counts=counts, xyz=xyz, normals=nrm)
    res["integrate"] = dict(hbm_peak_gbps=bench.HBM_PEAK_GBPS, rows=rows)
    if tdv.STUDY_BUILD:
        ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
        one_row(8)
        res["integrate"]["one_row_per_wave_same_bytes"] = bool(d_vol.cpu().numpy().tobytes() == device_out["volume"].tobytes())
        ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
        fused(8)
    res["views"] = {"crossings_from_%d" % n: c for n, c in crossings.items()}
    # extraction of the eight-frame volume (the volume holds it now)
    m = crossings[8]
    out = torch.zeros((2, max(m, 1), 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ex = _median_ms(torch, {"with_normals": lambda: ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), m),
                            "without_normals": lambda: ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), out[0].data_ptr(), None, m)}, args.repeats)
    res["extract"] = dict(crossings=m, volume_bytes=vol.voxels * 8, **ex)
    if "host" not in skip:
        t0 = time.perf_counter()
        buf, counts = R.integrate(vol, R.reset(vol), frames, poses, intr)
        t1 = time.perf_counter()
        xyz, nrm, _ = R.extract(vol, buf)
        t2 = time.perf_counter()
        same = (buf.tobytes() == device_out["volume"].tobytes() and np.array_equal(counts, device_out["counts"])
                and xyz.tobytes() == device_out["xyz"].tobytes() and nrm.tobytes() == device_out["normals"].tobytes())
        res["host"] = dict(restatement_integrate_8_frames_ms=round(1e3 * (t1 - t0), 1), restatement_extract_ms=round(1e3 * (t2 - t1), 1),
                           same_bytes_as_restatement=bool(same))
    ctx.close()
    print(json.dumps(dict(tool="bench_tsdf", repeats=args.repeats, **res)))


if __name__ == "__main__":
    main()
