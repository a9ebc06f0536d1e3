"""Study (CPU): what is on the lists of RANSAC's two-level leaf-box bound (csrc/ransac.hip, RansacBoundLists), on the
inputs of ransac_leaf_bound_study.py: 200k pairs, half of them true, B = the best of the first 8,192 triples, 4,000 further random
triples as one bounded batch, the kernel's box test on coarse leaves of 128 pairs and fine leaves of 32, in float64.
  1. the present 6-D Morton leaves: the shares of the batch that are undecided after the coarse level, live after the fine level and
     killed by it, and Delta_h - the largest displacement between pose h and B over the 8 corners of the sources' bounding box - of
     the live ones and of the ones the fine level kills;
  2. the same shares with class-major leaves: B's outliers first, then its inliers, each class along its own Morton curve;
  3. class-major leaves plus "Delta_h <= c thresholds goes live without a walk": how much goes live unwalked, how much of that the
     walk would have killed, and the lengths of the fine list and of the live list.
Needs scipy.  python tools/studies/ransac_bound_lists_study.py"""
import os, sys, importlib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
synth = importlib.import_module('3dvision_amd.synth')
from scipy.spatial import cKDTree
n = 200000
tgt, _ = synth.sample_object(n, 42)
src, T_gt = synth.make_scene(n, 42)
vox = float(np.float32(synth.mean_spacing(n))); thr = 1.5 * vox
nn = cKDTree(tgt).query(src @ T_gt[:3, :3].T + T_gt[:3, 3])[1]
rng = np.random.default_rng(1234)
corr = np.where(rng.random(n) < 0.5, nn, rng.integers(0, n, n))
P = src.astype(np.float64); Q = tgt[corr].astype(np.float64)

def morton(X, bits):
    lo, hi = X.min(0), X.max(0)
    q = np.clip(((X - lo) / (hi - lo + 1e-12) * (1 << bits)).astype(np.int64), 0, (1 << bits) - 1)
    key = np.zeros(len(X), np.int64); D = X.shape[1]
    for b in range(bits):
        for d in range(D):
            key |= ((q[:, d] >> b) & 1) << (D * b + d)
    return key

def kabsch(ps, qs):
    cp, cq = ps.mean(0), qs.mean(0)
    H = (ps - cp).T @ (qs - cq)
    U, S, Vt = np.linalg.svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt[2] *= -1; R = Vt.T @ U.T
    return R, cq - R @ cp

def count(R, t):
    return int((np.linalg.norm(P @ R.T + t - Q, axis=1) < thr).sum())

# B: the best of the first batch (only an all-true triple can win; 200 of them are scored)
tri = rng.integers(0, n, (8192, 3))
best = -1
for k in np.nonzero((corr[tri] == nn[tri]).all(1))[0][:200]:
    R, t = kabsch(P[tri[k]], Q[tri[k]])
    c = count(R, t)
    if c > best: best, RB, tB = c, R, t
print("%d pairs, spacing %.5f; B = the best of the first 8192 triples: %d inliers" % (n, vox, best))
H = 4000
hyps = [kabsch(P[t_], Q[t_]) for t_ in rng.integers(0, n, (H, 3))]

def leaves(LEAF, key):
    order = np.argsort(key, kind='stable')
    nl = -(-n // LEAF); pad = nl * LEAF - n
    Ps = np.concatenate([P[order], np.repeat(P[order[-1:]], pad, 0)]).reshape(nl, LEAF, 3)
    Qs = np.concatenate([Q[order], np.repeat(Q[order[-1:]], pad, 0)]).reshape(nl, LEAF, 3)
    sz = np.full(nl, LEAF); sz[-1] = LEAF - pad
    return Ps.min(1), Ps.max(1), Qs.min(1), Qs.max(1), sz

def bounds(L):
    Pmin, Pmax, Qmin, Qmax, sz = L
    c = (Pmin + Pmax) / 2; e = (Pmax - Pmin) / 2
    out = []
    for R, t in hyps:
        xc = c @ R.T + t; xe = e @ np.abs(R).T
        gap = np.maximum(0, np.maximum((xc - xe) - Qmax, Qmin - (xc + xe)))
        out.append(sz[(gap ** 2).sum(1) < thr * thr].sum())
    return np.array(out)

k6 = morton(np.concatenate([P, Q], 1), 5)
inl = np.linalg.norm(P @ RB.T + tB - Q, axis=1) < thr
lo, hi = P.min(0), P.max(0)
corners = np.array([[(hi if (k >> d) & 1 else lo)[d] for d in range(3)] for k in range(8)])
delta = np.array([np.linalg.norm(corners @ (R - RB).T + (t - tB), axis=1).max() for R, t in hyps])      # Delta_h, in metres
cnt = np.array([count(R, t) for R, t in hyps[:1500]])
print("true counts of the first 1500 hypotheses: max %d (best %d)" % (cnt.max(), best))

def lists(key):
    uc = bounds(leaves(128, key)); uf = bounds(leaves(32, key))
    und = uc > best
    return und, und & (uf > best)

print("\n1. present: 6-D Morton leaves")
und, live = lists(k6)
print("   undecided after the coarse level %.4f, live after the fine level %.4f, killed by the fine level %.4f" % (und.mean(), live.mean(), (und & ~live).mean()))
print("   Delta_h of the live ones, spacings: median %.1f, 90 %% %.1f, 99 %% %.1f" % tuple(np.percentile(delta[live] / vox, (50, 90, 99))))
print("   Delta_h of the ones the fine level kills, spacings: 1 %% %.1f, 5 %% %.1f, median %.1f" % tuple(np.percentile(delta[und & ~live] / vox, (1, 5, 50))))
print("   hypotheses with a true count above the best that are not live: %d" % int(((cnt > best) & ~live[:1500]).sum()))

print("\n2. class-major leaves: B's outliers, then its inliers, 6-D Morton inside each class")
und, live = lists(k6 + (inl.astype(np.int64) << 30))
print("   undecided after the coarse level %.4f, live after the fine level %.4f, killed by the fine level %.4f" % (und.mean(), live.mean(), (und & ~live).mean()))
print("   hypotheses with a true count above the best that are not live: %d" % int(((cnt > best) & ~live[:1500]).sum()))

print("\n3. class-major leaves, Delta_h <= c thresholds live without a walk (shares of the batch)")
print("| c (thresholds) | pre-live | of them coarse-dead / fine-dead | fine list | live list |")
for c in (6, 9, 13, 20, 27):
    pre = delta <= c * thr
    print("| %d | %.4f | %.4f / %.4f | %.4f | %.4f |" % (c, pre.mean(), (pre & ~und).mean(), (pre & und & ~live).mean(), (und & ~pre).mean(), (pre | live).mean()))
    assert not ((cnt > best) & ~(pre | live)[:1500]).any()
