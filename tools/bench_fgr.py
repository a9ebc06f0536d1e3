#!/usr/bin/env python3
"""Fast Global Registration (tdv_fgr_dev) against RANSAC (tdv_ransac_dev, --hyps hypotheses, the reference's settings) on the same clouds
and descriptors.

  c4     instance 0 of tools/bench_refine.py's scene (tools/bench_batch.py's workload: the relief part in a 1280x720 frame against one
         shared model, C4's voxel size): voxels, normals and FPFH made on the device;
  chain  the three instances of tests/chain_scene.py (the full-chain tests' scene), prepared by the CPU oracle as those tests do.
Per scene: the median time of --repeats alternating rounds of FGR, FGR with iteration_number 0 (the difference is the optimisation
loop) and RANSAC, the two descriptor matches FGR runs (tdv_feature_match_dev each way), the pose error against the ground truth before
and after the same tdv_icp_dev refinement, and n_mutual, n_tuple and trials_run.  Prints one JSON line.

    python tools/bench_fgr.py [--repeats 7] [--hyps 10000] [--icp-iters 50]
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


def compare(torch, ctx, synth, src, tgt, d, T_gt, voxel, args):
    """d: device tensors src, tgt, tgt normals, fs, ft."""
    ns, nt = int(src.shape[0]), int(tgt.shape[0])
    p = lambda k: d[k].data_ptr()   # noqa: E731
    corr = torch.zeros(max(ns, nt), dtype=torch.int32, device=d["src"].device)
    runs = dict(fgr=lambda: ctx.fgr_dev(p("src"), ns, p("tgt"), nt, p("fs"), p("ft"), voxel),
                fgr_iter0=lambda: ctx.fgr_dev(p("src"), ns, p("tgt"), nt, p("fs"), p("ft"), voxel, iteration_number=0),
                ransac=lambda: ctx.ransac_dev(p("src"), ns, p("tgt"), nt, p("fs"), p("ft"), None, voxel, args.hyps, 0.999, 42),
                match_st=lambda: ctx.feature_match_dev(p("fs"), ns, p("ft"), nt, corr.data_ptr()),
                match_ts=lambda: ctx.feature_match_dev(p("ft"), nt, p("fs"), ns, corr.data_ptr()))
    out = _timed(torch, runs, args.repeats)
    g, info = runs["fgr"]()
    r = runs["ransac"]()
    thr = voxel * 0.4
    for name, T in (("fgr", g.transformation), ("ransac", r.transformation)):
        fine = ctx.icp_dev(p("src"), ns, p("tgt"), p("tn"), nt, T, thr, args.icp_iters)
        a0, t0 = synth.pose_error(T, T_gt)
        a1, t1 = synth.pose_error(fine.transformation, T_gt)
        out[name] = dict(rad=float("%.3g" % a0), m=float("%.3g" % t0), icp_rad=float("%.3g" % a1), icp_m=float("%.3g" % t1),
                         fitness=round(float(fine.fitness), 4))
    out["fgr"].update(n_mutual=info["n_mutual"], n_tuple=info["n_tuple"], trials_run=info["trials_run"], degenerate=info["degenerate"],
                      inliers=g.inliers)
    out["ransac"].update(inliers=r.inliers)
    out.update(ns=ns, nt=nt)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--hyps", type=int, default=10000)
    ap.add_argument("--icp-iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    from oracle import pyoracle as orc
    import chain_scene as cs
    dev = torch.device("cuda", 0)
    ctx = tdv.Context(0)
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
    d = dict(src=d_vox[:n].contiguous(), tgt=d_mx[:nm].contiguous(), tn=d_mn[:nm].contiguous(), fs=d_fs, ft=d_mf[:nm].contiguous())
    res["c4"] = compare(torch, ctx, synth, d["src"], d["tgt"], d, wl["T_gt"][0], voxel, args)

    # the chain scene, prepared by the oracle as tests/test_oracle_chain.py does
    orc.lib()
    sc = cs.build(synth, n_instances=3)
    model = cs.oracle_model(orc, sc)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)   # noqa: E731
    for b in range(3):
        dp = orc.depth_preprocess(sc["depth"][b], sc["masks"][b], cs.SCALE)
        xyz, _ = orc.unproject(dp, None, cs.F, cs.F, cs.CX, cs.CY, cs.ZMAX)
        src, _, _ = orc.voxel_downsample(xyz, None, cs.VOXEL)
        fs = orc.compute_fpfh(src, orc.estimate_normals(src, 30), cs.VOXEL * 5.0)
        d = dict(src=up(src), tgt=up(model["xyz"]), tn=up(model["normals"]), fs=up(fs), ft=up(model["fpfh"]))
        res["chain%d" % b] = compare(torch, ctx, synth, d["src"], d["tgt"], d, sc["T_gt"][b], cs.VOXEL, args)
    ctx.close()
    print(json.dumps(dict(tool="bench_fgr", hyps=args.hyps, **res)))


if __name__ == "__main__":
    main()
