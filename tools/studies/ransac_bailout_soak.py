"""One-off soak (GPU box): 150 random RANSAC calls (sizes, inlier shares, thresholds, 16k-140k iterations, stopping confidences incl. 0) -
the default run without a trace (exact bail-out) against the exact scoring kernel.  Result at the end of round 2: 0 mismatches."""
import importlib, os, sys, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
tdv = importlib.import_module("3dvision_amd"); synth = importlib.import_module("3dvision_amd.synth")
import test_gpu_ransac as T
ctx = tdv.Context(0)
bad = 0
for seed in range(1000, 1150):
    rng = np.random.default_rng(seed)
    ns = int(rng.integers(20, 9000)); nt = int(rng.integers(10, 5000))
    good = float(rng.choice([0.0, 0.02, 0.2, 0.5, 0.9, 1.0]))
    src, tgt, corr, _ = T._case(synth, ns, nt, seed=seed, good_frac=good)
    voxel = float(rng.choice([0.001, 0.002, 0.004, 0.02, 0.1]))
    iters = int(rng.choice([16385, 17000, 40000, 65537, 66000, 131072, 140000]))
    conf = float(rng.choice([2.0, 2.0, 0.9, 0.5, 0.2, 0.05, 0.0]))
    ctx.set_ransac_score("exact"); e = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=conf)
    ctx.set_ransac_score("fast"); f = ctx.ransac(src, tgt, corr=corr, voxel=voxel, max_iterations=iters, confidence=conf)
    ok = (f.best_iteration, f.iterations_run, f.inliers, f.fitness, f.rmse) == (e.best_iteration, e.iterations_run, e.inliers, e.fitness, e.rmse) and f.transformation.tobytes() == e.transformation.tobytes()
    if not ok:
        bad += 1; print("MISMATCH seed", seed, ns, nt, good, voxel, iters, conf, (f.best_iteration, f.inliers), (e.best_iteration, e.inliers))
print("soak: 150 cases, mismatches:", bad)
