#!/usr/bin/env python3
"""The mesh of a fused volume (tdv_tsdf_extract_mesh_dev, include/tdv_hip.h rules T9 to T12) beside the cloud of the same volume
(tdv_tsdf_extract_dev with normals, whose code this feature leaves as it was), on tools/bench_tsdf.py's scene: 400 x 300 x 200 voxels of
1 mm, eight 1280 x 720 frames.  Prints one JSON line.

  mesh     the vertex and triangle counts; the whole mesh call and the whole cloud call, alternating in one process, each timed on the
           host up to a synchronise: median, minimum and maximum in ms over --repeats rounds after a warm-up, and their ratio.  The
           kernels' own times - the share of the mesh call spent in the triangle pass among them - come from a
           `rocprofv3 --kernel-trace --stats` run of this tool (tools/prof_kernels.sh).
  host     the numpy restatement (tests/tsdf_mesh_restatement.py) of the same mesh on the host, and whether the device wrote the same
           bytes (vertices, normals, triangles).
  relief   the CPU suite's relief scene (tests/tsdf_cases.py: 136 x 96 x 40 voxels, four 640 x 480 views with holes): its fused mesh under
           tdv_verify_poses_mesh with back faces culled at each of the four view poses against that view's frame - the consistent,
           violating, occluded and unknown shares of the rendered pixels.

    python tools/bench_tsdf_mesh.py [--repeats 9] [--skip host,relief]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32


def relief_scores(ctx):
    import tsdf_cases as Cs
    s = Cs.relief_scene()
    xyz, _, tri = ctx.tsdf_fuse_mesh(s["frames"], s["poses"], s["intr"], s["vol"].args(), trunc=0.004)
    views = []
    for frame, pose in zip(s["frames"], s["poses"]):
        r = ctx.verify_poses_mesh(xyz, tri, pose[None], frame, *s["intr"], pose_direction="model_to_camera", cull="back")[0][0]
        n = max(r["n_rendered"], 1)
        views.append(dict(rendered=r["n_rendered"], **{k: round(100.0 * r["n_" + k] / n, 2) for k in ("consistent", "violating", "occluded", "unknown")}))
    return dict(vertices=len(xyz), triangles=len(tri), share_of_rendered_percent=views)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--skip", type=str, default="")
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_mesh.py measures on the GPU: no device")
    import bench_tsdf
    skip = set(args.skip.split(",")) if args.skip else set()
    s = bench_tsdf.build_scene()
    vol, frames, poses, intr = s["vol"], s["frames"], s["poses"], s["intr"]
    h, w = frames.shape[1:]
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)
    cvol, d_vol = ctx.tsdf_volume(*vol.args())
    d_raw = torch.from_numpy(frames.view(np.int16).copy()).to(dev)
    torch.cuda.synchronize()
    ctx.tsdf_integrate_dev(cvol, d_vol.data_ptr(), d_raw.data_ptr(), poses, w, h, *intr, want_counts=False)
    nv, nt, _ = ctx.tsdf_extract_mesh_dev(cvol, d_vol.data_ptr(), None, None, 0, None, 0)
    out = torch.zeros((2, max(nv, 1), 3), dtype=torch.float32, device=dev)
    tri = torch.zeros((max(nt, 1), 3), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    runs = {"mesh": lambda: ctx.tsdf_extract_mesh_dev(cvol, d_vol.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), nv, tri.data_ptr(), nt),
            "cloud_with_normals": lambda: ctx.tsdf_extract_dev(cvol, d_vol.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), nv)}
    t = bench_tsdf._median_ms(torch, runs, args.repeats)
    res = dict(volume=dict(dims=bench_tsdf.DIMS, voxels=vol.voxels, bytes=vol.voxels * 8), vertices=nv, triangles=nt, **t,
               mesh_over_cloud=round(t["mesh"]["median_ms"] / t["cloud_with_normals"]["median_ms"], 3))
    runs["mesh"]()
    ctx.synchronize()
    got = out.cpu().numpy()[:, :nv].copy(), tri.cpu().numpy()[:nt].copy()
    referenced = int(len(np.unique(got[1])))
    res["vertices_in_no_triangle"] = nv - referenced
    if "host" not in skip:
        import tsdf_mesh_restatement as M
        buf = d_vol.cpu().numpy().reshape(vol.nz, vol.ny, vol.nx, 2)
        t0 = time.perf_counter()
        xyz, nrm, _, rt = M.mesh(vol, buf)
        t1 = time.perf_counter()
        res["host"] = dict(restatement_mesh_ms=round(1e3 * (t1 - t0), 1),
                           same_bytes_as_restatement=bool(xyz.tobytes() == got[0][0].tobytes() and nrm.tobytes() == got[0][1].tobytes()
                                                          and rt.tobytes() == got[1].tobytes()))
    if "relief" not in skip:
        res["relief"] = relief_scores(ctx)
    ctx.close()
    print(json.dumps(dict(tool="bench_tsdf_mesh", repeats=args.repeats, **res)))


if __name__ == "__main__":
    main()
