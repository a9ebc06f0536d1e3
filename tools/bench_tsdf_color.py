#!/usr/bin/env python3
"""Coloured TSDF fusion (tdv_tsdf_integrate_color_dev / tdv_tsdf_extract_color_dev / tdv_tsdf_extract_mesh_color_dev /
tdv_tsdf_raycast_color_dev, include/tdv_hip.h) beside the plain calls, on tools/bench_tsdf.py's scene: a 360 x 260 mm relief plate in
400 x 300 x 200 voxels of 1 mm (24 M voxels: 192 MB of pairs, 384 MB of colour quads), eight 1280 x 720 frames from 0.6 m with seeded
random BGR images.  Prints one JSON line.

  integrate  1, 4 and 8 frames in one call, plain and coloured alternating, every call timed on the host up to a synchronise (no
             read-back in the call).  Per count: median, minimum and maximum in ms over --repeats rounds after a warm-up; the voxels at
             least one frame updates, and the bytes per second that 16 bytes per such voxel (the pair's load and store) amount to for the
             plain call and 48 (the pair's and the quad's) for the coloured one, beside bench.py's HBM_PEAK_GBPS.
  ab         with TDV_LIB_VARIANT=study: the coloured call with two and with eight voxel rows per wave (csrc/tsdf.hip:
             TDV_TSDF_COLOR_ROWS), alternating with the product's four, and whether all leave the same bytes.
  extract    the crossings of the eight-frame volume, plain and coloured, with normals: the whole call.
  mesh       the mesh of the same volume, plain and coloured.
  raycast    a 1280 x 720 view from the scan pose, depth and both maps, plain and with the colour map.
  same       whether the coloured calls left the plain calls' bytes (pair volume, points, normals, triangles, maps).

    python tools/bench_tsdf_color.py [--repeats 9]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32
ZMAX = 1.0
OTHER_ROWS = (2, 8)                                        # the study library's sides of the rows-per-wave A/B; the product has four


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_color.py measures on the GPU: no device")
    import bench
    import bench_tsdf
    import tsdf_color_cases as Cc
    s = bench_tsdf.build_scene()
    vol, frames, poses, intr = s["vol"], s["frames"], s["poses"], s["intr"]
    images = Cc.random_images(frames)
    h, w = frames.shape[1:]
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)
    cvol, d_vol = ctx.tsdf_volume(*vol.args())
    d_col = ctx.tsdf_color_volume(cvol)
    d_raw = torch.from_numpy(frames.view(np.int16).copy()).to(dev)
    d_bgr = torch.from_numpy(images).to(dev)
    torch.cuda.synchronize()

    def plain(n):
        ctx.tsdf_integrate_dev(cvol, d_vol.data_ptr(), d_raw.data_ptr(), poses[:n], w, h, *intr, want_counts=False)
        ctx.synchronize()

    def coloured(n):
        ctx.tsdf_integrate_color_dev(cvol, d_vol.data_ptr(), d_col.data_ptr(), d_raw.data_ptr(), d_bgr.data_ptr(), poses[:n], w, h, *intr, want_counts=False)
        ctx.synchronize()

    def other_rows(n, rows):
        os.environ["TDV_TSDF_COLOR_ROWS"] = str(rows)
        try:
            coloured(n)
        finally:
            os.environ.pop("TDV_TSDF_COLOR_ROWS", None)

    def fresh():
        ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
        ctx.tsdf_color_reset_dev(cvol, d_col.data_ptr())

    res = dict(volume=dict(dims=bench_tsdf.DIMS, voxels=vol.voxels, pair_bytes=vol.voxels * 8, colour_bytes=vol.voxels * 16),
               frames=dict(size=bench_tsdf.SIZE, count=len(frames)), study_build=bool(tdv.STUDY_BUILD))
    runs = {}
    for n in (1, 4, 8):
        runs[("plain", n)] = lambda n=n: plain(n)
        runs[("coloured", n)] = lambda n=n: coloured(n)
        if tdv.STUDY_BUILD:
            for rows in OTHER_ROWS:
                runs[("coloured_%d_rows_per_wave" % rows, n)] = lambda n=n, rows=rows: other_rows(n, rows)
    t = bench_tsdf._median_ms(torch, runs, args.repeats)
    rows = []
    for n in (1, 4, 8):
        fresh()
        coloured(n)
        touched = int((d_vol[:, 1] > 0).sum().item())
        p, c = t[("plain", n)], t[("coloured", n)]
        rows.append(dict(frames=n, voxels_updated=touched, plain=p, coloured=c, coloured_over_plain=round(c["median_ms"] / p["median_ms"], 3),
                         plain_gbps_at_16_bytes=round(16 * touched / (1e-3 * p["median_ms"]) / 1e9, 1),
                         coloured_gbps_at_48_bytes=round(48 * touched / (1e-3 * c["median_ms"]) / 1e9, 1)))
        if tdv.STUDY_BUILD:
            for k in OTHER_ROWS:
                rows[-1]["coloured_%d_rows_per_wave" % k] = t[("coloured_%d_rows_per_wave" % k, n)]
    res["integrate"] = dict(hbm_peak_gbps=bench.HBM_PEAK_GBPS, rows=rows)
    same = {}
    if tdv.STUDY_BUILD:
        kept = d_col.cpu().numpy().tobytes(), d_vol.cpu().numpy().tobytes()
        for k in OTHER_ROWS:
            fresh()
            other_rows(8, k)
            same["%d_rows_per_wave" % k] = bool(kept == (d_col.cpu().numpy().tobytes(), d_vol.cpu().numpy().tobytes()))
    # the plain call's pair volume
    pair = d_vol.cpu().numpy().tobytes()
    ctx.tsdf_reset_dev(cvol, d_vol.data_ptr())
    plain(8)
    same["pair_volume"] = bool(d_vol.cpu().numpy().tobytes() == pair)
    # extraction and mesh of the eight-frame volumes
    nv, nt, _ = ctx.tsdf_extract_mesh_dev(cvol, d_vol.data_ptr(), None, None, 0, None, 0)
    out = torch.zeros((5, max(nv, 1), 3), dtype=torch.float32, device=dev)
    tri = torch.zeros((2, max(nt, 1), 3), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pv, pc = d_vol.data_ptr(), d_col.data_ptr()
    o = [out[k].data_ptr() for k in range(5)]
    ex = bench_tsdf._median_ms(torch, {
        "extract_plain": lambda: ctx.tsdf_extract_dev(cvol, pv, o[0], o[1], nv),
        "extract_coloured": lambda: ctx.tsdf_extract_color_dev(cvol, pv, pc, o[2], o[3], o[4], nv),
        "mesh_plain": lambda: ctx.tsdf_extract_mesh_dev(cvol, pv, o[0], o[1], nv, tri[0].data_ptr(), nt),
        "mesh_coloured": lambda: ctx.tsdf_extract_mesh_color_dev(cvol, pv, pc, o[2], o[3], o[4], nv, tri[1].data_ptr(), nt)}, args.repeats)
    ctx.synchronize()
    same["points_normals_triangles"] = bool(torch.equal(out[0], out[2]) and torch.equal(out[1], out[3]) and torch.equal(tri[0], tri[1]))
    rgb = out[4, :nv]
    res["extract"] = dict(crossings=nv, triangles=nt, coloured_rows=int((rgb != 0).any(1).sum().item()), rgb_min=float(rgb.min().item()) if nv else 0.0,
                          rgb_max=float(rgb.max().item()) if nv else 0.0, **ex)
    # the ray cast
    maps = torch.zeros((7, w * h, 3), dtype=torch.float32, device=dev)
    dd = torch.zeros((2, w * h), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m = [maps[k].data_ptr() for k in range(7)]
    pose, cam = poses[0], intr[1:]
    rc = bench_tsdf._median_ms(torch, {
        "raycast_plain": lambda: ctx.tsdf_raycast_dev(cvol, pv, pose, w, h, *cam, dd[0].data_ptr(), m[0], m[1], want_count=False, zmax=ZMAX),
        "raycast_coloured": lambda: ctx.tsdf_raycast_color_dev(cvol, pv, pc, pose, w, h, *cam, dd[1].data_ptr(), m[2], m[3], m[4], want_count=False,
                                                              zmax=ZMAX)}, args.repeats)
    ctx.synchronize()
    same["depth_and_maps"] = bool(torch.equal(dd[0], dd[1]) and torch.equal(maps[0], maps[2]) and torch.equal(maps[1], maps[3]))
    res["raycast"] = dict(image=bench_tsdf.SIZE, hits=int((dd[1] != 0).sum().item()), coloured_pixels=int((maps[4] != 0).any(1).sum().item()), **rc)
    res["same_bytes_as_plain"] = same
    ctx.close()
    print(json.dumps(dict(tool="bench_tsdf_color", repeats=args.repeats, **res)))


if __name__ == "__main__":
    main()
