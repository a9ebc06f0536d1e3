"""One ICP iteration on the hash-grid path against the number of source points (same 200k-point target): the fixed and the per-point
part of the whole iteration, of the search launch, and - from a kernel trace - of every ICP kernel.

    python tools/studies/icp_grid_scaling.py [--forms auto|two|one,...] [--cache auto|off|on,...] [--rounds R] [--sizes N,N,...]
                                             [--iters K] [--trans T,T,...] [--no-timer]
        per source count, form (tdv_ctx_set_icp_launches) and probe-cache setting (tdv_ctx_set_icp_probe_cache; all alternated, R rounds):
        iteration_us is a K-iteration fixed run (default 100) between two events with timing off, nn_kernel_us is TDV_TIMER_ICP_NN per
        launch (with ONE launch that is the whole fused kernel), probe_misses what the cache reports for that run.  --trans: the start
        pose's translation error(s) instead of 0.0005 (with --iters: calls whose pose moves by cells per iteration - the cache misses
        everywhere).  On a library without the probe cache only --cache auto runs.
        TDV_LIB_VARIANT=study TDV_ICP_PROBE_STUDY=heads|probe (with --cache on): the iteration without its probe loop resp. without its
        list walk (csrc/icp.hip: grid_nearest's PROBE 2 and 3), the bound on what the cache can save.
    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/studies/icp_grid_scaling.py ...
    python tools/studies/icp_grid_scaling.py --trace <kernel_trace.csv>
        the trace of such a run split by kernel and workgroup count (one workgroup count per source count): mean us per launch of
        k_icp_nn_grid, k_icp_accumulate and k_icp_iterate.  k_icp_accumulate at 12,500 sources is that kernel's fixed part."""
import argparse, csv, importlib, os, sys, json

SIZES = (12500, 25000, 50000, 100000, 200000, 400000, 800000)
ap = argparse.ArgumentParser()
ap.add_argument("--forms", default="auto")
ap.add_argument("--cache", default="auto")
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--trans", default="0.0005")
ap.add_argument("--no-timer", action="store_true", help="skip the timed run (TDV_TIMER_ICP_NN)")
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--sizes", help="source counts instead of the standard seven (with --trace: the counts of the traced run)")
ap.add_argument("--trace")
args = ap.parse_args()
if args.sizes: SIZES = tuple(int(n) for n in args.sizes.split(","))

if args.trace:
    acc = {}
    for r in csv.DictReader(open(args.trace)):
        name = r["Kernel_Name"].split("(")[0]
        kern = next((k for k in ("k_icp_nn_grid", "k_icp_accumulate", "k_icp_iterate") if k in name and "_multi" not in name), None)
        if not kern: continue
        wgs = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
        acc.setdefault((kern, wgs), []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    pts = {"k_icp_nn_grid": 256, "k_icp_accumulate": 1024, "k_icp_iterate": 1024}
    for (kern, wgs), d in sorted(acc.items()):
        ns = [n for n in SIZES if (n + pts[kern] - 1) // pts[kern] == wgs]
        d = sorted(d)[: max(1, len(d) * 9 // 10)]      # without the slowest tenth: first launches of a call
        print(json.dumps({"kernel": kern, "workgroups": wgs, "ns": ns[0] if ns else None, "launches": len(d), "mean_us": sum(d) / len(d) / 1e3, "min_us": d[0] / 1e3}))
    sys.exit(0)

import numpy as np
import torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
tdv = importlib.import_module("3dvision_amd")
synth = importlib.import_module("3dvision_amd.synth")
nt = 200000
ctx = tdv.Context(0); dev = torch.device("cuda", 0)
tgt, nrm = synth.sample_object(nt, 42)
voxel = float(np.float32(synth.mean_spacing(nt)))
d_tgt = torch.from_numpy(tgt).to(dev); d_nrm = torch.from_numpy(nrm).to(dev)
ctx.set_icp_search("grid")
K = args.iters
for ns in SIZES:
  for trans in (float(t) for t in args.trans.split(",")):
    src, T_gt = synth.make_scene(ns, 42)
    T0 = synth.perturb(T_gt, 42, angle_deg=0.3, trans=trans)
    d_src = torch.from_numpy(src).to(dev)
    run = lambda n: ctx.icp_dev(d_src.data_ptr(), ns, d_tgt.data_ptr(), d_nrm.data_ptr(), nt, T0, voxel * 0.4, n, True, fixed_iterations=True)
    for rnd in range(args.rounds):
        for form in args.forms.split(","):
          for cache in args.cache.split(","):
            if form != "auto": ctx.set_icp_launches(form)
            if cache != "auto": ctx.set_icp_probe_cache(cache)
            run(min(K, 10))
            reps = max(1, 100 // K)            # short calls: several between the two events
            e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): r = run(K)
            e1.record(); e1.synchronize()
            out = {"ns": ns, "form": form, "cache": cache, "trans": trans, "iters": K, "round": rnd, "search": ctx.last_icp_search(),
                   "iteration_us": e0.elapsed_time(e1) * 1e3 / (K * reps), "n_corr": r.n_corr}
            if hasattr(ctx, "last_icp_probe_misses"): out["probe_misses"] = ctx.last_icp_probe_misses()
            if not args.no_timer:
                ctx.timing_enable(True); ctx.timing_read(tdv.TIMER_ICP_NN)
                run(K)
                ms, launches = ctx.timing_read(tdv.TIMER_ICP_NN); ctx.timing_enable(False)
                out.update({"nn_kernel_us": ms / launches * 1e3, "ns_per_point": ms / launches * 1e6 / ns})
            if form != "auto": out["ran"] = ctx.last_icp_launches()
            print(json.dumps(out), flush=True)
