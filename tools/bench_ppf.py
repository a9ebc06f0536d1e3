#!/usr/bin/env python3
"""PPF matching (tdv_ppf_model_dev + tdv_ppf_match_dev) against the descriptor chain (normals + FPFH of the scene, then tdv_ransac_dev with
its descriptor match, --hyps hypotheses) on the same clouds.

  c4     instance 0 of tools/bench_refine.py's scene (tools/bench_batch.py's workload, C4's voxel size: ~150 k points a side): voxels,
         normals and FPFH made on the device.  PPF votes on clouds sampled at about the distance step: model and scene are downsampled
         again at --ppf-voxel-factor x the voxel size (raised in steps of 10 % until the model has at most TDV_PPF_MODEL_MAX points) and get normals of their own
         (tdv_estimate_normals_dev, k = 12); `ppf_scene_prep` times that for the scene.  The PPF pose goes through ICP on the coarse
         clouds (threshold 2 coarse voxels) before the fine ICP both poses get.
  scene  the scene of the PPF tests (tests/ppf_scene.py: the part, its floor patch and 10 % clutter against a 330-point model), normals as
         given there; the descriptor chain computes its own normals and FPFH on both clouds.
Per scene: the median time of --repeats alternating rounds of the table build, the match, the scene's normals alone (what PPF needs), the
scene's normals + FPFH and RANSAC (what the descriptor chain needs), and the pose error against the ground truth before and after the same
tdv_icp_dev refinement for the best-fitness PPF pose and for RANSAC's.  Prints one JSON line.

    python tools/bench_ppf.py [--repeats 7] [--hyps 10000] [--icp-iters 50]

With --instances B[,B...] it measures the batch instead: the test scene's instances (tests/ppf_scene.py: build(synth, seed, k), k = 1..B, one
model) back to back on the device, the table built once; one tdv_ppf_match_batch_dev call against a loop of B tdv_ppf_match_dev calls, both
warmed, alternating, --repeats rounds: median, minimum and maximum of each in ms, and whether both returned the same poses.

    python tools/bench_ppf.py --instances 64,256 [--repeats 7]
"""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _timed(torch, runs, repeats):
    for f in runs.values():           # warm-up: arena growth, code load
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, f in runs.items():     # alternating, so that a slow phase of the machine hits every one
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t)
    return {k + "_ms": round(1e3 * float(np.median(v)), 4) for k, v in times.items()}


def compare(torch, ctx, synth, d, T_gt, voxel, score_thr, icp_thr, args, ppf_kw):
    """d: device tensors src, tgt, tn (the scene and the model of RANSAC and the fine ICP), fs, ft, ps, psn, pm, pn (PPF's scene and model
    with normals); optional prep (callable: what makes ps and psn from src) and coarse_thr (ICP on PPF's clouds before the fine one)."""
    dev = d["src"].device
    ns, nt, npm, nps = int(d["src"].shape[0]), int(d["tgt"].shape[0]), int(d["pm"].shape[0]), int(d["ps"].shape[0])
    p = lambda k: d[k].data_ptr()   # noqa: E731
    nbytes = ctx.ppf_model_bytes(npm, **ppf_kw)
    table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    nrm = torch.empty((ns, 3), dtype=torch.float32, device=dev); fs = torch.empty((ns, 33), dtype=torch.float32, device=dev)
    info = ctx.ppf_model_dev(p("pm"), p("pn"), npm, table.data_ptr(), nbytes, **ppf_kw)
    runs = dict(ppf_model=lambda: ctx.ppf_model_dev(p("pm"), p("pn"), npm, table.data_ptr(), nbytes, **ppf_kw),
                ppf_match=lambda: ctx.ppf_match_dev(p("ps"), p("psn"), nps, p("pm"), p("pn"), npm, table.data_ptr(), info, score_thr, **ppf_kw),
                scene_normals=lambda: ctx.estimate_normals_dev(p("src"), ns, 30, nrm.data_ptr()),
                scene_normals_fpfh=lambda: ctx.normals_fpfh_dev(p("src"), ns, 30, voxel * 5.0, nrm.data_ptr(), fs.data_ptr()),
                ransac=lambda: ctx.ransac_dev(p("src"), ns, p("tgt"), nt, p("fs"), p("ft"), None, voxel, args.hyps, 0.999, 42))
    if d.get("prep"):
        runs["ppf_scene_prep"] = d["prep"]
    out = _timed(torch, runs, args.repeats)
    poses, more, n_ref = runs["ppf_match"]()
    r = runs["ransac"]()
    best = max(range(len(poses)), key=lambda k: poses[k].fitness) if poses else None
    for name, T in (("ppf", poses[best].transformation if poses else np.eye(4, dtype=np.float32)), ("ransac", r.transformation)):
        T_first = T
        if name == "ppf" and d.get("coarse_thr"):
            T = ctx.icp_dev(p("ps"), nps, p("pm"), p("pn"), npm, T, d["coarse_thr"], args.icp_iters).transformation
            a, t = synth.pose_error(T, T_gt)
            out["ppf_coarse_icp"] = dict(rad=float("%.3g" % a), m=float("%.3g" % t))
        fine = ctx.icp_dev(p("src"), ns, p("tgt"), p("tn"), nt, T, icp_thr, args.icp_iters)
        a0, t0 = synth.pose_error(T_first, T_gt)
        a1, t1 = synth.pose_error(fine.transformation, T_gt)
        out[name] = dict(rad=float("%.3g" % a0), m=float("%.3g" % t0), icp_rad=float("%.3g" % a1), icp_m=float("%.3g" % t1),
                         fitness=round(float(fine.fitness), 4))
    out["ppf"].update(n_poses=len(poses), best_rank=best, n_ref=n_ref, n_pairs=info["n_pairs"], table_mib=round(nbytes / 2 ** 20, 1),
                      votes=[m["votes"] for m in more])
    out["ransac"].update(inliers=r.inliers)
    out.update(ns=ns, nt=nt, n_ppf_model=npm, n_ppf_scene=nps)
    return out


def batch_against_loop(torch, tdv, ctx, synth, S, n_inst, args):
    """One batch call against n_inst single calls on the same device buffers and table."""
    dev = torch.device("cuda", 0)
    scenes = [S.build(synth, args.seed, k) for k in range(1, n_inst + 1)]
    off = np.zeros(n_inst + 1, np.int32)
    off[1:] = np.cumsum([len(sc["scene"]) for sc in scenes])
    up = lambda a: torch.from_numpy(np.array(a, np.float32)).to(dev)   # noqa: E731
    d_src, d_sn = up(np.concatenate([sc["scene"] for sc in scenes])), up(np.concatenate([sc["scene_normals"] for sc in scenes]))
    d_tgt, d_tn = up(scenes[0]["model"]), up(scenes[0]["model_normals"])
    nt = int(d_tgt.shape[0])
    nbytes = ctx.ppf_model_bytes(nt)
    table = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    info = ctx.ppf_model_dev(d_tgt.data_ptr(), d_tn.data_ptr(), nt, table.data_ptr(), nbytes)
    ps, pn, pt, ptn, ptab = d_src.data_ptr(), d_sn.data_ptr(), d_tgt.data_ptr(), d_tn.data_ptr(), table.data_ptr()
    # (through ctypes directly: the Python wrappers' result objects would be timed with the calls)
    lib, C = tdv.lib(), tdv.C
    prm = tdv.ppf_params()
    ci = tdv.PpfModelInfoC(**{k: info[k] for k, _ in tdv.PpfModelInfoC._fields_})
    b_poses = (tdv.PpfPoseC * (n_inst * prm.max_poses))(); b_n = (C.c_int * n_inst)()
    l_poses = (tdv.PpfPoseC * (n_inst * prm.max_poses))(); l_n = (C.c_int * n_inst)()
    h_off = (C.c_int * (n_inst + 1))(*[int(v) for v in off])
    V = C.c_void_p

    def batch():
        st = lib.tdv_ppf_match_batch_dev(ctx._h, V(ps), V(pn), h_off, n_inst, V(pt), V(ptn), nt, V(ptab), C.byref(ci), C.c_float(S.THR), C.byref(prm),
                                         b_poses, b_n, None, None)
        assert st == 0, st

    def loop():
        one = C.sizeof(tdv.PpfPoseC) * prm.max_poses
        for b in range(n_inst):
            st = lib.tdv_ppf_match_dev(ctx._h, V(ps + 12 * int(off[b])), V(pn + 12 * int(off[b])), int(off[b + 1] - off[b]), V(pt), V(ptn), nt, V(ptab),
                                       C.byref(ci), C.c_float(S.THR), C.byref(prm), C.byref(l_poses, b * one), C.byref(l_n, 4 * b), None, None)
            assert st == 0, st

    runs = dict(batch=batch, loop=loop)
    for f in runs.values():
        f()
    torch.cuda.synchronize()
    same = list(b_n) == list(l_n) and all(bytes(b_poses[b * prm.max_poses + k]) == bytes(l_poses[b * prm.max_poses + k])
                                          for b in range(n_inst) for k in range(b_n[b]))
    times = {k: [] for k in runs}
    for _ in range(args.repeats):
        for k, f in runs.items():
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t))
    out = dict(instances=n_inst, points=int(off[-1]), nt=nt, poses=int(sum(b_n)), same_bytes=bool(same))
    for k, v in times.items():
        out[k] = dict(median_ms=round(float(np.median(v)), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
    out["batch_below_loop_by_more_than_its_spread"] = bool(out["loop"]["median_ms"] - out["batch"]["median_ms"] > out["loop"]["max_ms"] - out["loop"]["min_ms"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=str, default="", help="B[,B...]: time one batch call against B single calls, nothing else")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hyps", type=int, default=10000)
    ap.add_argument("--icp-iters", type=int, default=50)
    ap.add_argument("--ppf-voxel-factor", type=float, default=9.0)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    import ppf_scene as S
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)
    if args.instances:
        res = [batch_against_loop(torch, tdv, ctx, synth, S, int(b), args) for b in args.instances.split(",")]
        ctx.close()
        print(json.dumps(dict(tool="bench_ppf", batch=res)))
        return
    res = {}

    # C4: instance 0 of bench_refine.py's scene, prepared on the device
    bb = _tool("bench_batch")
    wl = bb.build_workload(tdv, synth, ctx, 1, 1.2, 448, args.seed, tdv.TDV_VOXEL_ORDER_REFERENCE, dev)
    d_mx, d_mn, d_mf, nm = wl["model"]
    voxel = wl["voxel"]
    cap = int(sum(wl["mask_px"]))
    d_xyz = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    off = ctx.depth_to_cloud_batch_dev(wl["depth"].data_ptr(), wl["masks"].data_ptr(), None, 1, bb.W, bb.H, bb.SCALE, bb.F, bb.F, bb.CX,
                                       bb.CY, bb.ZMAX, d_xyz.data_ptr(), None, cap, n_frames=1)
    d_vox = torch.empty_like(d_xyz)
    n = ctx.voxel_downsample_dev(d_xyz.data_ptr(), None, int(off[1]), voxel, d_vox.data_ptr(), None, int(off[1]),
                                 order=tdv.TDV_VOXEL_ORDER_REFERENCE)
    d_nrm = torch.empty((n, 3), dtype=torch.float32, device=dev); d_fs = torch.empty((n, 33), dtype=torch.float32, device=dev)
    ctx.normals_fpfh_dev(d_vox.data_ptr(), n, 30, voxel * 5.0, d_nrm.data_ptr(), d_fs.data_ptr())
    factor = args.ppf_voxel_factor
    d_pm = torch.empty((nm, 3), dtype=torch.float32, device=dev)
    while True:                                                      # the coarsest of factor, 1.1 factor, ... that fits a PPF model
        pv = voxel * factor
        npm = ctx.voxel_downsample_dev(d_mx.data_ptr(), None, nm, pv, d_pm.data_ptr(), None, nm, order=tdv.TDV_VOXEL_ORDER_FIRST)
        if npm <= tdv.TDV_PPF_MODEL_MAX:
            break
        factor *= 1.1
    d_pn = torch.empty((npm, 3), dtype=torch.float32, device=dev)
    ctx.estimate_normals_dev(d_pm.data_ptr(), npm, 12, d_pn.data_ptr())
    d_ps = torch.empty((n, 3), dtype=torch.float32, device=dev); d_psn = torch.empty((n, 3), dtype=torch.float32, device=dev)
    nps = [0]

    def prep():
        nps[0] = ctx.voxel_downsample_dev(d_vox.data_ptr(), None, n, pv, d_ps.data_ptr(), None, n, order=tdv.TDV_VOXEL_ORDER_FIRST)
        ctx.estimate_normals_dev(d_ps.data_ptr(), nps[0], 12, d_psn.data_ptr())
    prep()
    d = dict(src=d_vox[:n].contiguous(), tgt=d_mx[:nm].contiguous(), tn=d_mn[:nm].contiguous(), fs=d_fs, ft=d_mf[:nm].contiguous(),
             ps=d_ps[:nps[0]], psn=d_psn[:nps[0]], pm=d_pm[:npm].contiguous(), pn=d_pn, prep=prep, coarse_thr=2.0 * pv)
    res["c4"] = dict(compare(torch, ctx, synth, d, wl["T_gt"][0], voxel, pv, voxel * 0.4, args, {}), ppf_voxel_factor=round(factor, 3))

    # the PPF tests' scene; the descriptor chain gets normals and FPFH of its own on both clouds
    sc = S.build(synth)
    up = lambda a: torch.from_numpy(np.array(a, np.float32)).to(dev)   # noqa: E731
    d = dict(src=up(sc["scene"]), psn=up(sc["scene_normals"]), tgt=up(sc["model"]), tn=up(sc["model_normals"]))
    d.update(ps=d["src"], pm=d["tgt"], pn=d["tn"])
    for cloud, key in (("src", "fs"), ("tgt", "ft")):
        m = int(d[cloud].shape[0])
        nr = torch.empty((m, 3), dtype=torch.float32, device=dev); d[key] = torch.empty((m, 33), dtype=torch.float32, device=dev)
        ctx.normals_fpfh_dev(d[cloud].data_ptr(), m, 30, S.MODEL_STEP * 5.0, nr.data_ptr(), d[key].data_ptr())
    res["scene"] = compare(torch, ctx, synth, d, sc["T_gt"], S.MODEL_STEP, S.THR, S.THR, args, {})
    ctx.close()
    print(json.dumps(dict(tool="bench_ppf", hyps=args.hyps, **res)))


if __name__ == "__main__":
    main()
