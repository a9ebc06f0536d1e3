#!/usr/bin/env python3
"""Study (CPU only, no GPU): what the order of the scored points does to RANSAC's exact bail-out.

The bail-out (RansacPlan) scores a hypothesis over a prefix of P = N - cut * best points and drops it when
count(prefix) + (N - P) <= best.  Counts do not depend on the order of the points, the survivors do.  On bench.py's inputs (synth
seed 42, half of the correspondences true) this script draws random triples, solves each pose with a numpy Kabsch, scores every
hypothesis with an inlier rate over 2 % in full, and reports, per order and cut, how many of those survive the prefix and the share
of their tests that is evaluated, tests / (good hypotheses x N):
    natural   the points as they come
    best      the outliers of the best hypothesis first, its inliers behind them (stable)
    stale     the same partition made from the best of the first eighth of the triples, the rule against the true best
and, for the `best` order, the ideal of a check every 1,000 points (a hypothesis stops at the first check that drops it).
    python tools/studies/ransac_point_order_study.py [--points 200000] [--triples 16384]"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
synth = importlib.import_module("3dvision_amd.synth")


def nearest(p, tgt):
    """index of the nearest target per point: a k-d tree where scipy is installed, a cell grid otherwise"""
    try:
        from scipy.spatial import cKDTree
        return cKDTree(tgt).query(p)[1].astype(np.int64)
    except ImportError:
        pass
    lo = tgt.min(0); cell = float(np.prod(tgt.max(0) - lo + 1e-9) / max(len(tgt) / 8.0, 1.0)) ** (1.0 / 3.0)
    dims = np.floor((tgt.max(0) - lo) / cell).astype(np.int64) + 1
    key = lambda c: (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    ct = np.floor((tgt - lo) / cell).astype(np.int64); kt = key(ct); order = np.argsort(kt, kind="stable"); ks = kt[order]
    cp = np.clip(np.floor((p - lo) / cell).astype(np.int64), 0, dims - 1)
    best = np.zeros(len(p), np.int64); bd = np.full(len(p), np.inf)
    for dx in range(-1, 2):
        for dy in range(-1, 2):
            for dz in range(-1, 2):
                c = cp + (dx, dy, dz); ok = ((c >= 0) & (c < dims)).all(1)
                k = key(c); a = np.searchsorted(ks, k, "left"); b = np.searchsorted(ks, k, "right")
                for j in range(int((b - a)[ok].max(initial=0))):
                    sel = ok & (a + j < b); t = order[np.minimum(a + j, len(order) - 1)]
                    d = ((p - tgt[t]) ** 2).sum(1); d[~sel] = np.inf
                    up = d < bd; bd[up] = d[up]; best[up] = t[up]
    return best


def kabsch(P, Q):
    """rotation and translation per triple: P, Q [H, 3, 3] (three points each)"""
    pc, qc = P.mean(1, keepdims=True), Q.mean(1, keepdims=True)
    H = np.einsum("hki,hkj->hij", P - pc, Q - qc)
    U, _, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(np.einsum("hji,hkj->hik", Vt, U)))
    D = np.zeros_like(H); D[:, 0, 0] = 1; D[:, 1, 1] = 1; D[:, 2, 2] = d
    R = np.einsum("hji,hjk,hlk->hil", Vt, D, U)
    return R, qc[:, 0] - np.einsum("hij,hj->hi", R, pc[:, 0])


def inlier_masks(R, t, p, q, tau, block=16):
    out = np.empty((len(R), len(p)), bool)
    for a in range(0, len(R), block):
        x = np.einsum("hij,nj->hni", R[a:a + block], p) + t[a:a + block, None, :] - q[None]
        out[a:a + block] = (x * x).sum(2) < tau
    return out


def report(name, masks, order, best, cuts, n):
    for cut in cuts:
        P = n - int(cut * best)
        prefix = masks[:, order[:P]].sum(1)
        keep = prefix + (n - P) > best
        tests = len(masks) * P + int(keep.sum()) * (n - P)
        print("  %-8s cut %.2f  prefix %6d  survivors %5d of %5d  tests share %.3f" % (name, cut, P, keep.sum(), len(masks), tests / (len(masks) * float(n))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--triples", type=int, default=16384)
    args = ap.parse_args()
    n = args.points
    tgt, _ = synth.sample_object(n, 42)
    src, T = synth.make_scene(n, 42)
    T = np.asarray(T, np.float64).reshape(4, 4)
    nn = nearest(src.astype(np.float64) @ T[:3, :3].T + T[:3, 3], tgt.astype(np.float64))
    rng = np.random.Generator(np.random.PCG64(1234))
    corr = np.where(rng.random(n) < 0.5, nn, rng.integers(0, n, n))
    p = src.astype(np.float64); q = tgt[corr].astype(np.float64)
    tau = (float(np.float32(synth.mean_spacing(n))) * 1.5) ** 2
    tri = rng.integers(0, n, (args.triples, 3))
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    R, t = kabsch(p[tri], q[tri])
    sub = rng.choice(n, min(n, 4000), replace=False)                      # a cheap first look: who is worth a full count
    good = np.nonzero(inlier_masks(R, t, p[sub], q[sub], tau).mean(1) > 0.01)[0]
    masks = inlier_masks(R[good], t[good], p, q, tau)
    counts = masks.sum(1)
    sel = counts > 0.02 * n
    good, masks, counts = good[sel], masks[sel], counts[sel]
    best_i = int(np.argmax(counts)); best = int(counts[best_i])
    early = good < len(tri) // 8
    stale_i = int(np.nonzero(early)[0][np.argmax(counts[early])]) if early.any() else best_i
    print("%d points, %d valid triples, %d hypotheses with a rate over 2 %%, best count %d, stale best %d" % (n, len(tri), len(good), best, counts[stale_i]))
    cuts = (0.85, 0.90, 0.95, 0.97, 0.99)
    natural = np.arange(n)
    part = lambda m: np.concatenate([np.nonzero(~m)[0], np.nonzero(m)[0]])       # outliers first, stable
    report("natural", masks, natural, best, cuts, n)
    report("best", masks, part(masks[best_i]), best, cuts, n)
    report("stale", masks, part(masks[stale_i]), best, cuts, n)
    # the ideal with many checkpoints, best-first order: a hypothesis stops at the first multiple of 1,000 points where it is dropped
    m = n // 1000
    marks = np.arange(1, m + 1) * 1000
    cum = masks[:, part(masks[best_i])[:m * 1000]].reshape(len(masks), m, 1000).sum(2).cumsum(1)
    dropped = cum + (n - marks)[None] <= best
    stop = np.where(dropped.any(1), marks[np.argmax(dropped, 1)], n)
    print("  best, a check every 1,000 points: tests share %.3f" % (stop.sum() / (len(masks) * float(n))))


if __name__ == "__main__":
    main()
