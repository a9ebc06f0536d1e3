#!/usr/bin/env python3
"""Pose verification (tdv_verify_poses_dev, include/tdv_hip.h): what it costs to score a frame's candidate poses by rendering, against
scoring them one by one with tdv_icp_correspondences, and whether the two rank the candidates alike.  Prints one JSON line.

  ppf    the PPF batch tests' scene (tests/ppf_batch_cases.py: eight instances of the relief part, each a cloud of its own at its own pose,
         ~1,450 points with the floor patch and 10 % clutter).  Each instance gets the depth frame its camera would have seen: the dense part
         and its floor patch rendered at the instance's pose (synth.render_depth, 320 x 240, f = 500, 0.1 mm units), so eight frames and
         eight verification calls, one per frame with all of its candidates.  The verification model is the part's surface at 2 mm (splat 1
         at 1 mm pixels), tau the default 2 mm.
  tray   --tray-instances parts of the tray scene (synth.tray_scene: ONE 1280 x 720 frame, parts of 25 pixels): the instances' clouds are
         the pixels of their labels, the model is the scan of the part, and ONE verification call scores every candidate of every instance.
         The parts are 7.5 mm across, so tau is the voxel size (0.36 mm) and not the default.
  Candidates are what tdv_ppf_match_batch_dev returns (up to max_poses = 8 per instance), the threshold 1.5 voxels resp. the PPF tests' own.
  Timed, warmed, --repeats alternating rounds, each on the host around a whole call (every call ends in its own read-back): `verify` with
  the model and the frame resident on the device, `fitness` = tdv_icp_correspondences once per candidate on host arrays, the existing way
  to score a pose.  Ranking: per instance the first candidate by n_consistent - n_violating against the first by (fitness, then lower
  rmse); where they differ, which of the two is nearer the ground truth (rotation angle, then translation).

    python tools/bench_verify.py [--repeats 7] [--tray-instances 64] [--skip ppf,tray]
    python tools/bench_verify.py --registers      # the compiler's register / LDS report of csrc/verify.hip for gfx950 (no GPU needed)
"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32


def registers():
    """kernel-resource-usage of every kernel in csrc/verify.hip, compiled with the library's flags."""
    src = os.path.join(ROOT, "3dvision_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-I", os.path.join(ROOT, "include"), "-I", src, "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(src, "verify.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            t = re.search(r"k_verify_tilesILb(\d)E", name)
            cur = "k_verify_tiles<%s>" % ("render" if t.group(1) == "1" else "classify") if t else re.search(r"k_verify_[a-z]+", name).group(0)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1)] = int(m.group(2))
    return out


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


def _first_by_fitness(poses):
    return min(range(len(poses)), key=lambda i: (-float(poses[i].fitness), float(poses[i].rmse), i))


def _ranking(synth, per_instance):
    """per_instance: (poses, their verification results, T_gt).  The first candidate by either order, and who is nearer where they differ."""
    out = dict(instances=0, without_candidates=0, candidates=0, disagree=0, verify_nearer=0, fitness_nearer=0, tie=0, detail=[])
    for b, (poses, res, T_gt) in enumerate(per_instance):
        out["instances"] += 1
        if not poses:
            out["without_candidates"] += 1
            continue
        out["candidates"] += len(poses)
        score = [r["n_consistent"] - r["n_violating"] for r in res]
        iv = min(range(len(poses)), key=lambda i: (-score[i], i))
        ifit = _first_by_fitness(poses)
        if iv == ifit:
            continue
        out["disagree"] += 1
        ev, ef = synth.pose_error(poses[iv].transformation, T_gt), synth.pose_error(poses[ifit].transformation, T_gt)
        who = "verify_nearer" if ev < ef else "fitness_nearer" if ef < ev else "tie"
        out[who] += 1
        out["detail"].append(dict(instance=b, verify=dict(index=iv, score=score[iv], fitness=round(float(poses[iv].fitness), 4), err_rad=float("%.3g" % ev[0]),
                                                          err_mm=float("%.3g" % (1e3 * ev[1]))),
                                  fitness=dict(index=ifit, score=score[ifit], fitness=round(float(poses[ifit].fitness), 4), err_rad=float("%.3g" % ef[0]),
                                               err_mm=float("%.3g" % (1e3 * ef[1])))))
    return out


def _true_pose_check(ctx, d_model, n_model, T_gt, d_raw, w, h, scale, cam, prm):
    """The ground-truth pose through the verification: how much of it the frame agrees with."""
    r = ctx.verify_poses_dev(d_model, n_model, [T_gt], d_raw, w, h, scale, *cam, **prm)[0][0]
    return dict(n_rendered=r["n_rendered"], consistent=round(r["n_consistent"] / max(r["n_rendered"], 1), 4),
                violating=round(r["n_violating"] / max(r["n_rendered"], 1), 4))


def ppf_scene(torch, tdv, ctx, synth, args):
    import ppf_batch_cases as B
    import ppf_scene as S
    dev = torch.device("cuda", 0)
    W, H, f, scale = 320, 240, 500.0, 10000.0
    cam = (f, f, W / 2.0, H / 2.0)
    prm = dict(splat=1, tau=0.002, zmax=2.0)
    part = synth.ReliefPart(3)
    dense = part.surface_points(0.0004)
    g = np.arange(-0.1, 0.1 + 1e-9, 0.0004)
    FX, FY = (a.ravel() for a in np.meshgrid(g, g))
    keep = ((np.abs(FX) > part.L / 2) | (np.abs(FY) > part.W / 2)) & (np.abs(FX) <= part.L / 2 + 0.03) & (np.abs(FY) <= part.W / 2 + 0.03)
    dense = np.concatenate([dense, np.stack([FX[keep], FY[keep], np.full(int(keep.sum()), -0.004)], 1)])
    vmodel = S._surface(part, 0.002)[0].astype(F)
    scenes = [B.scene(synth, k) for k in B.EIGHT]
    sc0 = scenes[0]
    cands = ctx.ppf_match_batch([s["scene"] for s in scenes], [s["scene_normals"] for s in scenes], sc0["model"], sc0["model_normals"], S.THR)
    frames = [synth.render_depth(dense, synth.instance_pose(k, 0.5, 30.0), *cam, W, H, scale)[0] for k in B.EIGHT]
    d_frames = [torch.from_numpy(fr.view(np.int16)).to(dev) for fr in frames]
    d_model = torch.from_numpy(vmodel).to(dev)
    torch.cuda.synchronize()
    poses = [[p.transformation for p in res] for res, _ in cands]

    def verify():
        return [ctx.verify_poses_dev(d_model.data_ptr(), len(vmodel), T, d.data_ptr(), W, H, scale, *cam, **prm)[0] if len(T) else []
                for T, d in zip(poses, d_frames)]

    def fitness():
        for s, T in zip(scenes, poses):
            for t in T:
                ctx.icp_correspondences(s["scene"], sc0["model"], t, S.THR)

    res = verify()
    t = _median_ms(torch, dict(verify=verify, fitness=fitness), args.repeats)
    truth = [_true_pose_check(ctx, d_model.data_ptr(), len(vmodel), s["T_gt"], d.data_ptr(), W, H, scale, cam, prm) for s, d in zip(scenes, d_frames)]
    return dict(frame=[W, H], frames=len(frames), model_points=len(vmodel), scene_points=[len(s["scene"]) for s in scenes], params=prm,
                candidates=sum(len(T) for T in poses), calls=dict(verify=len(frames), fitness=sum(len(T) for T in poses)), time=t,
                true_pose=dict(consistent_min=min(x["consistent"] for x in truth), violating_max=max(x["violating"] for x in truth)),
                ranking=_ranking(synth, [(c[0], r, s["T_gt"]) for c, r, s in zip(cands, res, scenes)]))


def tray(torch, tdv, ctx, synth, args):
    dev = torch.device("cuda", 0)
    n_inst = args.tray_instances
    sc = synth.tray_scene(n_inst, seed=7, feature_voxels=3.0)
    W, H, scale, voxel = sc["width"], sc["height"], sc["scale"], sc["voxel"]
    cam = (sc["fx"], sc["fy"], sc["cx"], sc["cy"])
    prm = dict(splat=1, tau=voxel, zmax=sc["zmax"])
    thr = 1.5 * voxel

    def cloud(depth, select):
        v, u = np.nonzero(select)
        z = depth[v, u].astype(F) * F(1.0 / scale)
        return np.stack([(u.astype(F) - F(cam[2])) * z / F(cam[0]), (v.astype(F) - F(cam[3])) * z / F(cam[1]), z], 1).astype(F)

    model = cloud(sc["model_depth"], sc["model_mask"] > 0)
    model_n = ctx.estimate_normals(model, 12)
    clouds = [cloud(sc["depth"], sc["label"] == b + 1) for b in range(n_inst)]
    normals = [ctx.estimate_normals(c, 12) for c in clouds]
    cands = ctx.ppf_match_batch(clouds, normals, model, model_n, thr)
    poses = [[p.transformation for p in res] for res, _ in cands]
    flat = np.array([t for T in poses for t in T], F).reshape(-1, 4, 4)
    off = np.concatenate([[0], np.cumsum([len(T) for T in poses])])
    d_raw = torch.from_numpy(sc["depth"].view(np.int16)).to(dev)
    d_model = torch.from_numpy(model).to(dev)
    torch.cuda.synchronize()

    def verify():
        return ctx.verify_poses_dev(d_model.data_ptr(), len(model), flat, d_raw.data_ptr(), W, H, scale, *cam, **prm)[0]

    def fitness():
        for c, T in zip(clouds, poses):
            for t in T:
                ctx.icp_correspondences(c, model, t, thr)

    res = verify()
    t = _median_ms(torch, dict(verify=verify, fitness=fitness), args.repeats)
    truth = [_true_pose_check(ctx, d_model.data_ptr(), len(model), sc["T_gt"][b], d_raw.data_ptr(), W, H, scale, cam, prm) for b in range(min(n_inst, 16))]
    per = [(cands[b][0], res[off[b]:off[b + 1]], sc["T_gt"][b]) for b in range(n_inst)]
    return dict(frame=[W, H], instances=n_inst, model_points=len(model), scene_points=int(sum(len(c) for c in clouds)),
                params=dict(prm, tau=round(float(voxel), 6)), candidates=len(flat), calls=dict(verify=1, fitness=len(flat)), time=t,
                true_pose=dict(consistent_min=min(x["consistent"] for x in truth), violating_max=max(x["violating"] for x in truth)),
                ranking=_ranking(synth, per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--registers", action="store_true", help="print the compiler's resource report of csrc/verify.hip and exit")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--tray-instances", type=int, default=64)
    ap.add_argument("--skip", type=str, default="")
    args = ap.parse_args()
    if args.registers:
        print(json.dumps(dict(tool="bench_verify", registers=registers())))
        return
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    if not torch.cuda.is_available():
        raise SystemExit("bench_verify.py measures on the GPU: no device")
    skip = set(args.skip.split(",")) if args.skip else set()
    ctx = tdv.Context(0)
    res = {}
    if "ppf" not in skip:
        res["ppf"] = ppf_scene(torch, tdv, ctx, synth, args)
    if "tray" not in skip:
        res["tray"] = tray(torch, tdv, ctx, synth, args)
    ctx.close()
    print(json.dumps(dict(tool="bench_verify", repeats=args.repeats, **res)))


if __name__ == "__main__":
    main()
