#!/usr/bin/env python3
"""Study (CPU only, no GPU): how many of a live RANSAC hypothesis' tests fall on pairs that a bound from the best pose already rules
out (csrc/ransac.hip, RansacFarBound; profiles/r13/ransac_far_outliers.md).

Inputs as tools/studies/ransac_leaf_bound_study.py: synth seed 42, 200k pairs, half of them true, threshold 1.5 spacings.  The best B of
a first batch of 8,192 triples splits the pairs into its inliers I and outliers O; d_B(i) = |R_B p_i + t_B - q_i|.  The all-true triples
of a further 6,000 stand in for a bounded batch's live list.  For each of them Delta_h = max over the corners of the sources' box of
|(R_h - R_B) c + (t_h - t_B)|, and only the pairs with d_B < thr + Delta_h can be its inliers.  The script prints the table of d_B over O,
the quantiles of Delta_h, and a single-checkpoint model of the present scheme (phase 1 over the first N - 0.95 best points of [O | I],
survivors score the rest) against the proposed one: O split at r_F into F (far) and M, order [F | M | I]; a hypothesis with
UB_F(h) = #{i in F : d_B(i) < thr + Delta_h} <= U_cut skips F in phase 1, scores M and the first a points of I, and survives on
prefix + (|I| - a) + UB_F(h) > best; a survivor scores everything else.
    python tools/studies/ransac_far_outliers_study.py [--points 200000]"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from ransac_point_order_study import inlier_masks, kabsch, nearest       # noqa: E402

synth = importlib.import_module("3dvision_amd.synth")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200000)
    args = ap.parse_args()
    n = args.points
    tgt, _ = synth.sample_object(n, 42)
    src, T = synth.make_scene(n, 42)
    T = np.asarray(T, np.float64).reshape(4, 4)
    nn = nearest(src.astype(np.float64) @ T[:3, :3].T + T[:3, 3], tgt.astype(np.float64))
    rng = np.random.default_rng(1234)
    true = rng.random(n) < 0.5
    corr = np.where(true, nn, rng.integers(0, n, n))
    true = corr == nn
    p = src.astype(np.float64); q = tgt[corr].astype(np.float64)
    sp = float(np.float32(synth.mean_spacing(n))); thr = 1.5 * sp; tau = thr * thr

    def triples(k):
        tri = rng.integers(0, n, (k, 3))
        return tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]

    # the first batch's best
    tri = triples(8192)
    R, t = kabsch(p[tri], q[tri])
    sub = rng.choice(n, 4000, replace=False)
    rate = inlier_masks(R, t, p[sub], q[sub], tau).mean(1)
    cand = np.argsort(rate)[-64:]
    counts = inlier_masks(R[cand], t[cand], p, q, tau).sum(1)
    b = cand[int(np.argmax(counts))]; best = int(counts.max())
    RB, tB = R[b], t[b]
    dB = np.linalg.norm(p @ RB.T + tB - q, axis=1)
    inl = dB < thr
    O = ~inl
    print("%d pairs, spacing %.5f; best of %d triples: %d inliers; |O| %d with %d true pairs, false pairs in I: %d"
          % (n, sp, len(tri), best, O.sum(), (O & true).sum(), (inl & ~true).sum()))
    print("pairs of O with d_B below (spacings): " + "  ".join("%g: %d" % (r, (O & (dB < r * sp)).sum()) for r in (2, 3, 6, 10, 20, 50, 100)))

    # the stand-in for a live list: all-true triples of a further 6,000
    tri = triples(6000)
    tri = tri[true[tri].all(1)]
    R, t = kabsch(p[tri], q[tri])
    lo, hi = p.min(0), p.max(0)
    corners = np.array([[hi[a] if (k >> a) & 1 else lo[a] for a in range(3)] for k in range(8)])
    delta = np.linalg.norm(np.einsum("hij,kj->hki", R - RB, corners) + (t - tB)[:, None, :], axis=2).max(1)
    print("%d all-true triples; Delta_h in spacings at 10/25/50/75/90 %%: %s" % (len(tri), "  ".join("%.1f" % v for v in np.percentile(delta, (10, 25, 50, 75, 90)) / sp)))
    masks = inlier_masks(R, t, p, q, tau)
    full = masks.sum(1)
    print("their inlier counts: median %d, 75 %% %d; over O: median %d, max %d" % (np.median(full), np.percentile(full, 75), np.median(masks[:, O].sum(1)), masks[:, O].sum(1).max()))
    # the triangle inequality, checked: no inlier of h outside d_B < thr + Delta_h
    assert not (masks & (dB[None, :] >= thr + delta[:, None])).any()

    # the present scheme: order [O | I], phase 1 over the first N - 0.95 best points
    nO = int(O.sum()); H = len(tri)
    order = np.concatenate([np.nonzero(O)[0], np.nonzero(inl)[0]])
    P1 = n - int(0.95 * best)
    keep = masks[:, order[:P1]].sum(1) + (n - P1) > best
    present = H * P1 + int(keep.sum()) * (n - P1)
    print("present: phase 1 over %d points, survivors %.3f, tests %.3e" % (P1, keep.mean(), present))
    dO = np.sort(dB[O])
    print("| r_F (sp) | a | U_cut | near share | tests, new / present | survivors, new |")
    for rF, a, ucut in ((6, 4500, 900), (6, 10000, 2000), (6, 20000, 4000), (4, 20000, 1000), (3, 10000, 500)):
        F = O & (dB >= rF * sp); M = O & ~F
        nF, nM = int(F.sum()), int(M.sum())
        ubf = np.searchsorted(dO, thr + delta, side="left") - np.searchsorted(dO, rF * sp, side="left")     # pairs of F with d_B < thr + Delta_h
        ubf = np.maximum(ubf, 0)
        near = ubf <= ucut
        idxI = np.nonzero(inl)[0]
        pre_near = masks[:, M].sum(1) + masks[:, idxI[:a]].sum(1)
        keep_near = pre_near + (len(idxI) - a) + ubf > best
        surv = np.where(near, keep_near, keep)
        tests = (near * (nM + a)).sum() + (~near * P1).sum() + (surv & near).sum() * (n - nM - a) + (surv & ~near).sum() * (n - P1)
        print("| %g | %d | %d | %.2f | %.2f | %.3f |" % (rF, a, ucut, near.mean(), tests / present, surv.mean()))


if __name__ == "__main__":
    main()
