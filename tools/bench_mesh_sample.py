#!/usr/bin/env python3
"""Mesh sampling (tdv_mesh_sample_points_dev, include/tdv_hip.h): what a million samples cost, what the even-spread model costs, and what
the model buys PPF matching.  Prints one JSON line.

  cost   1,000,000 samples with every output but attr (36 bytes per sample) from the 4,800-face relief (tests/mesh_cases.py) and from a
         2^20-face jittered grid (tests/mesh_sample_cases.py), the whole `_dev` call timed on the host (it ends in its own read-back).
         Per shape: the median, minimum and maximum call in ms over --repeats alternating rounds after a warm-up, and two yardsticks: the
         numpy restatement of the same call on the host (what it replaces), and the sample kernel's floor - 36 bytes x 1,000,000 over the
         HBM bandwidth of bench.py's roofline block (HBM_PEAK_GBPS) - with the call's multiple of it.  The call is five launches and a
         read-back, so the multiple is the call's, not the kernel's: the kernel's own time comes from a `rocprofv3 --kernel-trace --stats`
         run of this tool.
  ab     the same two calls with every step of the search in global memory (csrc/mesh_sample.hip: k_ms_sample_global, the A/B that lost),
         alternating with the product's LDS-staged search, and whether both wrote the same bytes.  That kernel exists in the study
         library only: run with TDV_LIB_VARIANT=study.
  model  Context.mesh_model_dev for 2,048 points at oversample 8 on the relief: the median call, and the restatement's time on the host.
  ppf    tdv_ppf_match on the PPF tests' scene (tests/ppf_scene.py, the scene tools/bench_ppf.py reports as `scene`) with three models of the
         part: the surface grid at 5.7 mm that scene ships with (what bench_ppf.py uses today), and Context.mesh_model of the relief
         mesh at the grid's count and at TDV_PPF_MODEL_MAX.  Per model: the count and the best pose's fitness, rmse and error against the
         ground truth.

    python tools/bench_mesh_sample.py [--repeats 9] [--samples 1000000] [--skip cost,ab,model,ppf]
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
ROW_BYTES = 36                                      # xyz, normals, triangle, bary


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


def _shapes(synth):
    import mesh_cases
    import mesh_sample_cases
    return dict(relief_4800=mesh_cases.relief(synth.ReliefPart(seed=3), 0.002), grid_2p20=mesh_sample_cases.grid_mesh(1 << 20, seed=1))


class Call:
    """One shape on the device with its outputs; run() is the timed call."""

    def __init__(self, torch, ctx, v, t, n):
        dev = torch.device("cuda", 0)
        self.ctx, self.n, self.nv, self.nt = ctx, n, len(v), len(t)
        self.v, self.t = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
        self.out = dict(xyz=torch.zeros((n, 3), dtype=torch.float32, device=dev), normals=torch.zeros((n, 3), dtype=torch.float32, device=dev),
                        triangle=torch.zeros(n, dtype=torch.int32, device=dev), bary=torch.zeros((n, 2), dtype=torch.float32, device=dev))
        torch.cuda.synchronize()

    def run(self, global_search=False):
        if global_search:
            os.environ["TDV_MESH_SAMPLE_GLOBAL"] = "1"
        try:
            r = self.ctx.mesh_sample_dev(self.v.data_ptr(), self.nv, self.t.data_ptr(), self.nt, self.n, seed=1,
                                         **{"d_out_" + k: b.data_ptr() for k, b in self.out.items()})
        finally:
            os.environ.pop("TDV_MESH_SAMPLE_GLOBAL", None)
        assert r["n_sampled"] == self.n, r
        return r

    def bytes(self):
        return tuple(b.cpu().numpy().tobytes() for b in self.out.values())


def cost(torch, tdv, ctx, synth, args, want_ab):
    import bench
    import mesh_sample_restatement as R
    n = args.samples
    floor_us = 1e6 * ROW_BYTES * n / (bench.HBM_PEAK_GBPS * 1e9)
    shapes = _shapes(synth)
    calls = {name: Call(torch, ctx, v, t, n) for name, (v, t) in shapes.items()}
    runs = {(name, "product"): c.run for name, c in calls.items()}
    if want_ab:
        runs.update({(name, "global"): (lambda c=c: c.run(global_search=True)) for name, c in calls.items()})
    t = _median_ms(torch, runs, args.repeats)
    rows = []
    for name, (v, tri) in shapes.items():
        c = calls[name]
        c.run()
        ctx.synchronize()
        ref_bytes = c.bytes()
        t0 = time.perf_counter()
        ref = R.sample(v, tri, n, seed=1)
        host_ms = 1e3 * (time.perf_counter() - t0)
        row = dict(shape=name, triangles=len(tri), samples=n, bytes_per_sample=ROW_BYTES, **t[(name, "product")],
                   restatement_on_the_host_ms=round(host_ms, 1), floor_us=round(floor_us, 2),
                   call_over_floor=round(1e3 * t[(name, "product")]["median_ms"] / floor_us, 1),
                   same_bytes_as_restatement=bool(ref_bytes == tuple(ref[k].tobytes() for k in ("xyz", "normals", "triangle", "bary"))))
        if want_ab:
            c.run(global_search=True)
            ctx.synchronize()
            row["global_search"] = dict(t[(name, "global")], same_bytes=bool(c.bytes() == ref_bytes),
                                        product_faster_in_the_median=bool(t[(name, "product")]["median_ms"] < t[(name, "global")]["median_ms"]),
                                        product_faster_by_more_than_the_spread=bool(t[(name, "global")]["min_ms"] > t[(name, "product")]["max_ms"]))
        rows.append(row)
    return dict(hbm_peak_gbps=bench.HBM_PEAK_GBPS, rows=rows)


def model(torch, tdv, ctx, synth, args):
    import mesh_cases
    import mesh_sample_restatement as R
    dev = torch.device("cuda", 0)
    v, t = mesh_cases.relief(synth.ReliefPart(seed=3), 0.002)
    n_points, over = tdv.TDV_PPF_MODEL_MAX, 8
    d_v, d_t = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
    ox, on = torch.zeros((n_points, 3), dtype=torch.float32, device=dev), torch.zeros((n_points, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def run():
        r = ctx.mesh_model_dev(d_v.data_ptr(), len(v), d_t.data_ptr(), len(t), n_points, ox.data_ptr(), on.data_ptr(), over, 1)
        assert r["n_selected"] == n_points, r
    tm = _median_ms(torch, dict(model=run), args.repeats)["model"]
    t0 = time.perf_counter()
    px, pn, _ = R.mesh_model(v, t, n_points, over, 1)
    host_ms = 1e3 * (time.perf_counter() - t0)
    same = ox.cpu().numpy().tobytes() == px.tobytes() and on.cpu().numpy().tobytes() == pn.tobytes()
    return dict(triangles=len(t), n_points=n_points, oversample=over, **tm, restatement_on_the_host_ms=round(host_ms, 1), same_bytes_as_restatement=bool(same))


def ppf(tdv, ctx, synth):
    import mesh_cases
    import ppf_scene as S
    sc = S.build(synth)
    v, t = mesh_cases.relief(synth.ReliefPart(seed=3), 0.002)
    models = {"grid_5.7mm (today)": (sc["model"], sc["model_normals"])}
    for n in (len(sc["model"]), tdv.TDV_PPF_MODEL_MAX):
        px, pn, r = ctx.mesh_model(v, t, n, 8, 1)
        models["mesh_model_%d" % n] = (px, pn)
    out = {}
    for name, (mx, mn) in models.items():
        poses, _ = ctx.ppf_match(sc["scene"], sc["scene_normals"], mx, mn, S.THR)
        best = max(poses, key=lambda p: p.fitness) if poses else None
        e = synth.pose_error(best.transformation, sc["T_gt"]) if best else (float("nan"), float("nan"))
        out[name] = dict(count=len(mx), n_poses=len(poses), fitness=None if best is None else round(float(best.fitness), 4),
                         rmse_mm=None if best is None else round(1e3 * float(best.rmse), 4), err_rad=float("%.3g" % e[0]), err_mm=float("%.3g" % (1e3 * e[1])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--samples", type=int, default=1000000)
    ap.add_argument("--skip", type=str, default="")
    args = ap.parse_args()
    import torch
    tdv = importlib.import_module("3dvision_amd")
    synth = importlib.import_module("3dvision_amd.synth")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_sample.py measures on the GPU: no device")
    skip = set(args.skip.split(",")) if args.skip else set()
    ctx = tdv.Context(0)
    res = {}
    if "cost" not in skip:
        res["cost"] = cost(torch, tdv, ctx, synth, args, tdv.STUDY_BUILD and "ab" not in skip)
    if "model" not in skip:
        res["model"] = model(torch, tdv, ctx, synth, args)
    if "ppf" not in skip:
        res["ppf"] = ppf(tdv, ctx, synth)
    ctx.close()
    print(json.dumps(dict(tool="bench_mesh_sample", repeats=args.repeats, library="study" if tdv.STUDY_BUILD else "product", **res)))


if __name__ == "__main__":
    main()
