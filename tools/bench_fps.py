#!/usr/bin/env python3
"""Farthest point sampling (tdv_farthest_point_down_sample_dev, include/tdv_hip.h): what a sample costs on either kernel family, the batch
against a loop of single calls, and what an exact count buys a PPF model.  Prints one JSON line.

  cost   a random cloud of n points on the device, num_samples = 512 and 2,048 (--samples), the whole `_dev` call timed on the host (it ends
         in its own read-back): the workgroup kernels at n = 2,048, 8,192 and TDV_FPS_WORKGROUP_MAX, the grid kernels at
         TDV_FPS_WORKGROUP_MAX + 1, 50,000 and 200,000 and, forced, at 8,192 and TDV_FPS_WORKGROUP_MAX - the sizes both families take, so
         that AUTO's size rule is checked against a number.  Per row: the median call in ms, microseconds per sample (call / samples), and
         the marginal microseconds per sample between the two sample counts (the fixed cost of a call drops out).  Warmed, --repeats
         alternating rounds; every timed output is compared with the other family's bytes where both ran.
  batch  --instances 64,256: that many instances of the PPF tests' scene (tests/ppf_scene.py, ~1,450 points each) back to back, 256
         samples of each: one tdv_farthest_point_down_sample_batch_dev call against a loop of `_dev` calls on the same buffers; median,
         minimum and maximum in ms, and whether both wrote the same bytes.
  buys   a dense model (~20 k points with normals) brought under TDV_PPF_MODEL_MAX twice: by FPS to exactly 2,048 points (the normals as
         the companion rows), and by the voxel downsample at the smallest voxel size whose count fits (the normals averaged per voxel
         and renormalised).  Each goes through tdv_ppf_match on the PPF tests' scene; reported: the count reached and the best pose's
         fitness, rmse and error against the ground truth.  Two models: `relief`, the part the scene shows, sampled at 0.7 mm; and
         `object`, synth.sample_object(20000) - another part than the scene's, so its poses say nothing about registration (kept as the
         control: what the scoring gives a model that is not there).

    python tools/bench_fps.py [--repeats 7] [--samples 512,2048] [--instances 64,256] [--skip cost,batch,buys]
    python tools/bench_fps.py --registers      # the compiler's register / LDS report of csrc/fps.hip for gfx950 (no GPU needed)
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
    """kernel-resource-usage of every kernel in csrc/fps.hip, compiled with the library's flags."""
    src = os.path.join(ROOT, "3dvision_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-I", os.path.join(ROOT, "include"), "-I", src, "-Rpass-analysis=kernel-resource-usage",
           "-c", os.path.join(src, "fps.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            t = re.search(r"k_fps_workgroupILi(\d+)E", name)
            cur = "k_fps_workgroup<%s>" % t.group(1) if t else re.search(r"k_fps_[a-z_]+?(?=E[A-Z])|k_fps_[a-z_]+", name).group(0)
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
    return {k: (float(np.median(v)), min(v), max(v)) for k, v in times.items()}


def cost(torch, tdv, ctx, args):
    dev = torch.device("cuda", 0)
    cap = tdv.TDV_FPS_WORKGROUP_MAX
    ks = [int(v) for v in args.samples.split(",")]
    rows = [("workgroup", 2048), ("workgroup", 8192), ("workgroup", cap), ("grid", 8192), ("grid", cap), ("grid", cap + 1), ("grid", 50000), ("grid", 200000)]
    pts = torch.from_numpy(np.random.default_rng(1).random((200000, 3)).astype(F)).to(dev)
    kmax = max(ks)
    oi = {p: torch.zeros(kmax, dtype=torch.int32, device=dev) for p in ("workgroup", "grid")}
    od = {p: torch.zeros(kmax, dtype=torch.float32, device=dev) for p in ("workgroup", "grid")}
    torch.cuda.synchronize()
    runs = {}
    for path, n in rows:
        for k in ks:
            def f(path=path, n=n, k=k):
                ctx.set_fps_path(path)
                r = ctx.fps_dev(pts.data_ptr(), n, k, 0, None, 0, oi[path].data_ptr(), od[path].data_ptr())
                assert r["n_selected"] == min(k, n), r
            runs[(path, n, k)] = f
    t = _median_ms(torch, runs, args.repeats)
    same = {}
    for n in (8192, cap):             # both families on one size: the same bytes
        for k in ks:
            runs[("workgroup", n, k)](); runs[("grid", n, k)]()
            torch.cuda.synchronize()
            same["%d/%d" % (n, k)] = bool(torch.equal(oi["workgroup"][:k], oi["grid"][:k]) and torch.equal(od["workgroup"][:k], od["grid"][:k]))
    ctx.set_fps_path("auto")
    out = []
    for path, n in rows:
        row = dict(path=path, n=n)
        for k in ks:
            med, lo, hi = t[(path, n, k)]
            row["k%d" % k] = dict(call_ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), us_per_sample=round(1e3 * med / min(k, n), 3))
        if len(ks) >= 2 and min(ks[-1], n) > min(ks[0], n):
            row["marginal_us_per_sample"] = round(1e3 * (t[(path, n, ks[-1])][0] - t[(path, n, ks[0])][0]) / (min(ks[-1], n) - min(ks[0], n)), 3)
        out.append(row)
    return dict(rows=out, both_families_same_bytes=same)


def batch_against_loop(torch, tdv, ctx, synth, S, n_inst, args):
    """One batch call against n_inst single calls on the same device buffers."""
    dev = torch.device("cuda", 0)
    k = 256
    scenes = [S.build(synth, args.seed, b)["scene"] for b in range(1, n_inst + 1)]
    off = np.zeros(n_inst + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in scenes])
    d_xyz = torch.from_numpy(np.concatenate(scenes).astype(F)).to(dev)
    cap = int(np.minimum(np.diff(off), k).sum())
    out = {w: (torch.zeros(cap, dtype=torch.int32, device=dev), torch.zeros(cap, dtype=torch.float32, device=dev),
               torch.zeros((cap, 3), dtype=torch.float32, device=dev)) for w in ("batch", "loop")}
    torch.cuda.synchronize()
    lib, C = tdv.lib(), tdv.C           # (through ctypes directly: the Python wrappers' result objects would be timed with the calls)
    V = C.c_void_p
    h_off = (C.c_int * (n_inst + 1))(*[int(v) for v in off])
    h_out = (C.c_int * (n_inst + 1))()
    b_res, l_res = (tdv.FpsResultC * n_inst)(), (tdv.FpsResultC * n_inst)()
    px = d_xyz.data_ptr()

    def batch():
        i, d, x = out["batch"]
        st = lib.tdv_farthest_point_down_sample_batch_dev(ctx._h, V(px), None, 0, h_off, n_inst, k, b_res, h_out, V(i.data_ptr()), V(d.data_ptr()),
                                                          V(x.data_ptr()), None)
        assert st == 0, st

    def loop():
        i, d, x = out["loop"]
        o = 0
        for b in range(n_inst):
            st = lib.tdv_farthest_point_down_sample_dev(ctx._h, V(px + 12 * int(off[b])), int(off[b + 1] - off[b]), k, 0, None, 0,
                                                        C.byref(l_res, 16 * b), V(i.data_ptr() + 4 * o), V(d.data_ptr() + 4 * o), V(x.data_ptr() + 12 * o),
                                                        None)
            assert st == 0, st
            o += l_res[b].n_selected

    t = _median_ms(torch, dict(batch=batch, loop=loop), args.repeats)
    same = bytes(b_res) == bytes(l_res) and all(torch.equal(a, b) for a, b in zip(out["batch"], out["loop"])) and h_out[n_inst] == cap
    res = dict(instances=n_inst, points=int(off[-1]), samples_each=k, same_bytes=bool(same))
    for w, (med, lo, hi) in t.items():
        res[w] = dict(median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3))
    res["batch_below_loop_by_more_than_its_spread"] = bool(res["loop"]["median_ms"] - res["batch"]["median_ms"] > res["loop"]["max_ms"] - res["loop"]["min_ms"])
    return res


def _unit(v):
    return (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)).astype(F)


def buys(tdv, ctx, synth, S):
    sc = S.build(synth)
    part = synth.ReliefPart(3)
    dense = S._surface(part, 0.0007)
    models = dict(relief=(dense[0].astype(F), dense[1].astype(F)), object=synth.sample_object(20000, 7))
    res = {}
    for name, (pts, nrm) in models.items():
        row = dict(n_dense=len(pts))
        r = ctx.fps(pts, tdv.TDV_PPF_MODEL_MAX, 0, nrm)
        cands = dict(fps=(r["xyz"], _unit(r["attr"]), dict(cover_mm=round(1e3 * float(np.sqrt(r["cover_d2"])), 3))))
        lo, hi = 1e-4, 2e-2                                  # the smallest voxel size whose count fits: bisection (the count falls as the size grows)
        for _ in range(24):
            mid = 0.5 * (lo + hi)
            if len(ctx.voxel_downsample(pts, nrm, mid)[0]) <= tdv.TDV_PPF_MODEL_MAX:
                hi = mid
            else:
                lo = mid
        vx, vn = ctx.voxel_downsample(pts, nrm, hi)
        cands["voxel"] = (vx, _unit(vn), dict(voxel_mm=round(1e3 * hi, 4)))
        for how, (mx, mn, extra) in cands.items():
            poses, more = ctx.ppf_match(sc["scene"], sc["scene_normals"], mx, mn, S.THR)
            best = max(poses, key=lambda p: p.fitness) if poses else None
            e = synth.pose_error(best.transformation, sc["T_gt"]) if best else (float("nan"), float("nan"))
            row[how] = dict(extra, count=len(mx), n_poses=len(poses), fitness=None if best is None else round(float(best.fitness), 4),
                            rmse_mm=None if best is None else round(1e3 * float(best.rmse), 4), err_rad=float("%.3g" % e[0]), err_mm=float("%.3g" % (1e3 * e[1])))
        res[name] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--registers", action="store_true", help="print the compiler's resource report of csrc/fps.hip and exit")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--samples", type=str, default="512,2048")
    ap.add_argument("--instances", type=str, default="64,256")
    ap.add_argument("--skip", type=str, default="")
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()
    if args.registers:
        print(json.dumps(dict(tool="bench_fps", registers=registers())))
        return
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    import ppf_scene as S
    if not torch.cuda.is_available():
        raise SystemExit("bench_fps.py measures on the GPU: no device")
    skip = set(args.skip.split(",")) if args.skip else set()
    ctx = tdv.Context(0)
    res = {}
    if "cost" not in skip:
        res["cost"] = cost(torch, tdv, ctx, args)
    if "batch" not in skip:
        res["batch"] = [batch_against_loop(torch, tdv, ctx, synth, S, int(b), args) for b in args.instances.split(",")]
    if "buys" not in skip:
        res["buys"] = buys(tdv, ctx, synth, S)
    ctx.close()
    print(json.dumps(dict(tool="bench_fps", repeats=args.repeats, **res)))


if __name__ == "__main__":
    main()
