#!/usr/bin/env python3
"""Pose verification from a mesh (tdv_verify_poses_mesh_dev, include/tdv_hip.h) against the point splat (tdv_verify_poses_dev) in the same
run: what a call costs, how much of the frame agrees with the ground-truth pose under either renderer, and how either order ranks the
candidates.  Prints one JSON line.  The scenes, the candidates, the timing and the ranking are tools/bench_verify.py's:

  ppf    the PPF batch tests' eight instances of the relief part, a 320 x 240 frame each, eight calls of eight poses.  The splat's model is
         the part's surface at 2 mm (splat 1), the mesh is the part's height grid at 2 mm triangulated (tests/mesh_cases.py: relief), both
         in the model's frame, which is the part's.  tau the default 2 mm.
  tray   --tray-instances parts of the tray scene in ONE 1280 x 720 frame, one call for every candidate of every instance.  The splat's
         model is the scan of the part, the mesh is the disc part's height grid at one pixel footprint, moved into the model's frame (the
         scan camera's).  tau is the voxel size.
  box    tests/mesh_cases.py's box (12 faces of thousands of pixels: the kernel's cooperative path) at --box-poses poses around one pose in
         a 1280 x 720 frame rendered from the mesh itself, against a splat of 20,000 samples of the same surface; with and without culling.
  Timed, warmed, --repeats alternating rounds on the host clock around a whole call (every call ends in its own read-back), everything
  resident on the device.

    python tools/bench_verify_mesh.py [--repeats 7] [--tray-instances 64] [--box-poses 64] [--skip ppf,tray,box]
    python tools/bench_verify_mesh.py --registers   # the compiler's register / LDS report of csrc/verify_mesh.hip for gfx950 (no GPU needed)
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, _p)
import bench_verify as BV  # noqa: E402
import mesh_cases  # noqa: E402

F = np.float32


def registers():
    """kernel-resource-usage of every kernel in csrc/verify_mesh.hip, compiled with the library's flags."""
    src = os.path.join(ROOT, "3dvision_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-I", os.path.join(ROOT, "include"), "-I", src, "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(src, "verify_mesh.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            t = re.search(r"k_mesh_tilesILb(\d)E", name)
            cur = "k_mesh_tiles<%s>" % ("render" if t.group(1) == "1" else "classify") if t else re.search(r"k_mesh_[a-z]+", name).group(0)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1)] = int(m.group(2))
    return out


def _share(r):
    return dict(n_rendered=r["n_rendered"], consistent=round(r["n_consistent"] / max(r["n_rendered"], 1), 4),
                violating=round(r["n_violating"] / max(r["n_rendered"], 1), 4))


def _truth(shares):
    return dict(consistent_min=min(x["consistent"] for x in shares), violating_max=max(x["violating"] for x in shares),
                consistent_median=float(np.median([x["consistent"] for x in shares])))


def _first_errors(synth, per_instance, results):
    """Median rotation error (rad) against the ground truth of each order's first candidate: by fitness, and by each renderer's score."""
    out = {k: [] for k in ["fitness"] + list(results)}
    for b, (poses, T_gt) in enumerate(per_instance):
        if not poses:
            continue
        out["fitness"].append(synth.pose_error(poses[BV._first_by_fitness(poses)].transformation, T_gt)[0])
        for k, res in results.items():
            score = [r["n_consistent"] - r["n_violating"] for r in res[b]]
            out[k].append(synth.pose_error(poses[min(range(len(poses)), key=lambda i: (-score[i], i))].transformation, T_gt)[0])
    return {k: float("%.3g" % np.median(v)) for k, v in out.items() if v}


def _rank(synth, cands, res, T_gts):
    r = BV._ranking(synth, [(c[0], x, T) for c, x, T in zip(cands, res, T_gts)])
    r.pop("detail")
    return r


def ppf_scene(torch, tdv, ctx, synth, args):
    import ppf_batch_cases as B
    import ppf_scene as S
    dev = torch.device("cuda", 0)
    W, H, f, scale = 320, 240, 500.0, 10000.0
    cam = (f, f, W / 2.0, H / 2.0)
    sprm, mprm = dict(splat=1, tau=0.002, zmax=2.0), dict(tau=0.002, zmax=2.0)
    part = synth.ReliefPart(3)
    dense = part.surface_points(0.0004)
    g = np.arange(-0.1, 0.1 + 1e-9, 0.0004)
    FX, FY = (a.ravel() for a in np.meshgrid(g, g))
    keep = ((np.abs(FX) > part.L / 2) | (np.abs(FY) > part.W / 2)) & (np.abs(FX) <= part.L / 2 + 0.03) & (np.abs(FY) <= part.W / 2 + 0.03)
    dense = np.concatenate([dense, np.stack([FX[keep], FY[keep], np.full(int(keep.sum()), -0.004)], 1)])
    vmodel = S._surface(part, 0.002)[0].astype(F)
    verts, tris = mesh_cases.relief(part, 0.002)
    scenes = [B.scene(synth, k) for k in B.EIGHT]
    sc0 = scenes[0]
    cands = ctx.ppf_match_batch([s["scene"] for s in scenes], [s["scene_normals"] for s in scenes], sc0["model"], sc0["model_normals"], S.THR)
    frames = [synth.render_depth(dense, synth.instance_pose(k, 0.5, 30.0), *cam, W, H, scale)[0] for k in B.EIGHT]
    d_frames = [torch.from_numpy(fr.view(np.int16)).to(dev) for fr in frames]
    d_model, d_verts, d_tris = torch.from_numpy(vmodel).to(dev), torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    torch.cuda.synchronize()
    poses = [[p.transformation for p in res] for res, _ in cands]

    def splat(P=poses):
        return [ctx.verify_poses_dev(d_model.data_ptr(), len(vmodel), T, d.data_ptr(), W, H, scale, *cam, **sprm)[0] if len(T) else []
                for T, d in zip(P, d_frames)]

    def mesh(P=poses):
        return [ctx.verify_poses_mesh_dev(d_verts.data_ptr(), len(verts), d_tris.data_ptr(), len(tris), T, d.data_ptr(), W, H, scale, *cam, **mprm)[0]
                if len(T) else [] for T, d in zip(P, d_frames)]

    res = dict(splat=splat(), mesh=mesh())
    t = BV._median_ms(torch, dict(mesh=mesh, splat=splat), args.repeats)
    gt = [[s["T_gt"]] for s in scenes]
    truth = {k: _truth([_share(r[0]) for r in fn(gt)]) for k, fn in (("splat", splat), ("mesh", mesh))}
    T_gts = [s["T_gt"] for s in scenes]
    return dict(frame=[W, H], frames=len(frames), splat_points=len(vmodel), mesh=dict(vertices=len(verts), triangles=len(tris)),
                params=dict(splat=sprm, mesh=mprm), candidates=sum(len(T) for T in poses), calls=len(frames), time=t, true_pose=truth,
                ranking={k: _rank(synth, cands, res[k], T_gts) for k in res},
                first_candidate_err_rad=_first_errors(synth, [(c[0], T) for c, T in zip(cands, T_gts)], res))


def tray(torch, tdv, ctx, synth, args):
    dev = torch.device("cuda", 0)
    n_inst = args.tray_instances
    seed, feature_voxels, distance, f, part_px, voxel_px = 7, 3.0, 0.45, 1500.0, 25, 1.2        # tray_scene's arguments and defaults
    sc = synth.tray_scene(n_inst, seed=seed, feature_voxels=feature_voxels)
    W, H, scale, voxel = sc["width"], sc["height"], sc["scale"], sc["voxel"]
    cam = (sc["fx"], sc["fy"], sc["cx"], sc["cy"])
    sprm, mprm = dict(splat=1, tau=voxel, zmax=sc["zmax"]), dict(tau=voxel, zmax=sc["zmax"])
    thr = 1.5 * voxel

    def cloud(depth, select):
        v, u = np.nonzero(select)
        z = depth[v, u].astype(F) * F(1.0 / scale)
        return np.stack([(u.astype(F) - F(cam[2])) * z / F(cam[0]), (v.astype(F) - F(cam[3])) * z / F(cam[1]), z], 1).astype(F)

    model = cloud(sc["model_depth"], sc["model_mask"] > 0)
    px = distance / f
    part = synth.DiscPart(seed, part_px * px, feature_voxels * voxel_px * px)      # the part tray_scene drew
    assert len(part.bumps) == sc["bumps"]
    verts, tris = mesh_cases.relief(part, px, keep=lambda x, y: x * x + y * y <= (part.D / 2) ** 2, transform=synth.scan_pose(distance))
    model_n = ctx.estimate_normals(model, 12)
    clouds = [cloud(sc["depth"], sc["label"] == b + 1) for b in range(n_inst)]
    normals = [ctx.estimate_normals(c, 12) for c in clouds]
    cands = ctx.ppf_match_batch(clouds, normals, model, model_n, thr)
    poses = [[p.transformation for p in res] for res, _ in cands]
    flat = np.array([t for T in poses for t in T], F).reshape(-1, 4, 4)
    off = np.concatenate([[0], np.cumsum([len(T) for T in poses])])
    d_raw = torch.from_numpy(sc["depth"].view(np.int16)).to(dev)
    d_model, d_verts, d_tris = torch.from_numpy(model).to(dev), torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    torch.cuda.synchronize()

    def splat(P=flat):
        return ctx.verify_poses_dev(d_model.data_ptr(), len(model), P, d_raw.data_ptr(), W, H, scale, *cam, **sprm)[0]

    def mesh(P=flat):
        return ctx.verify_poses_mesh_dev(d_verts.data_ptr(), len(verts), d_tris.data_ptr(), len(tris), P, d_raw.data_ptr(), W, H, scale, *cam, **mprm)[0]

    flat_res = dict(splat=splat(), mesh=mesh())
    t = BV._median_ms(torch, dict(mesh=mesh, splat=splat), args.repeats)
    gt = np.array(sc["T_gt"][:n_inst], F)
    truth = {k: _truth([_share(r) for r in fn(gt)]) for k, fn in (("splat", splat), ("mesh", mesh))}
    res = {k: [v[off[b]:off[b + 1]] for b in range(n_inst)] for k, v in flat_res.items()}
    T_gts = sc["T_gt"][:n_inst]
    return dict(frame=[W, H], instances=n_inst, splat_points=len(model), mesh=dict(vertices=len(verts), triangles=len(tris)),
                params=dict(splat=dict(sprm, tau=round(float(voxel), 6)), mesh=dict(mprm, tau=round(float(voxel), 6))), candidates=len(flat),
                calls=1, time=t, true_pose=truth, ranking={k: _rank(synth, cands, res[k], T_gts) for k in res},
                first_candidate_err_rad=_first_errors(synth, [(c[0], T) for c, T in zip(cands, T_gts)], res))


def box(torch, tdv, ctx, synth, args):
    dev = torch.device("cuda", 0)
    W, H, f, scale = 1280, 720, 1500.0, 10000.0
    cam = (f, f, W / 2.0, H / 2.0)
    verts, tris = mesh_cases.box()
    true = synth.make_transform([1.0, 0.4, 0.1], 140.0, (0.01, 0.0, 0.7)).astype(F)    # model -> camera: 430 pixels across, 4 x 3 tiles
    rng = np.random.default_rng(5)
    poses = np.stack([true] * args.box_poses)
    poses[1:, :3, 3] += rng.uniform(-0.01, 0.01, (args.box_poses - 1, 3)).astype(F)
    pts = synth.sample_object(20000, 1)[0]                                         # (the boss of that object aside, the same box)
    samples = pts[np.abs(pts[:, 2]) <= 0.03 + 1e-6]
    d_verts, d_tris, d_pts = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev), torch.from_numpy(samples.copy()).to(dev)
    img = ctx.render_depth_mesh(verts, tris, true, W, H, *cam, pose_direction="model_to_camera")
    raw = np.rint(np.where(img != 0, img, F(1.0)).astype(np.float64) * scale).astype(np.uint16)
    d_raw = torch.from_numpy(raw.view(np.int16)).to(dev)
    torch.cuda.synchronize()
    m2c = dict(pose_direction="model_to_camera", tau=0.002, zmax=2.0)

    def mesh(cull="none"):
        return ctx.verify_poses_mesh_dev(d_verts.data_ptr(), 8, d_tris.data_ptr(), 12, poses, d_raw.data_ptr(), W, H, scale, *cam, cull=cull, **m2c)[0]

    def splat():
        return ctx.verify_poses_dev(d_pts.data_ptr(), len(samples), poses, d_raw.data_ptr(), W, H, scale, *cam, splat=1, **m2c)[0]

    r, rs = mesh()[0], splat()[0]
    t = BV._median_ms(torch, dict(mesh=mesh, mesh_cull_back=lambda: mesh("back"), splat=splat), args.repeats)
    return dict(frame=[W, H], poses=len(poses), mesh=dict(vertices=8, triangles=12), splat_points=len(samples), pixels_on_the_box=int((img != 0).sum()),
                time=t, true_pose=dict(mesh=_share(r), splat=_share(rs)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--registers", action="store_true", help="print the compiler's resource report of csrc/verify_mesh.hip and exit")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tray-instances", type=int, default=64)
    ap.add_argument("--box-poses", type=int, default=64)
    ap.add_argument("--skip", type=str, default="")
    args = ap.parse_args()
    if args.registers:
        print(json.dumps(dict(tool="bench_verify_mesh", registers=registers())))
        return
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify_mesh.py measures on the GPU: no device")
    skip = set(args.skip.split(",")) if args.skip else set()
    ctx = tdv.Context(0)
    res = {}
    for name, fn in (("ppf", ppf_scene), ("tray", tray), ("box", box)):
        if name not in skip:
            res[name] = fn(torch, tdv, ctx, synth, args)
    ctx.close()
    print(json.dumps(dict(tool="bench_verify_mesh", repeats=args.repeats, **res)))


if __name__ == "__main__":
    main()
