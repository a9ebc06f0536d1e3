"""Study (CPU): how tight a leaf-box upper bound of a RANSAC hypothesis' inlier count is on bench.py's workload (200k pairs, half
true nearest neighbours, threshold 1.5 voxel), for several orderings of the pairs and leaf sizes: the share of hypotheses whose bound
exceeds the best (ground-truth pose) count, i.e. the ones the bound cannot rule out.  Basis of RansacLeafBound (csrc/ransac.hip,
DESIGN.md 4): 6-D Morton order, 5 bits per coordinate, leaves of 32 pairs.  Needs scipy."""
import os, sys, importlib, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
synth = importlib.import_module('3dvision_amd.synth')
from scipy.spatial import cKDTree
n = 200000
tgt, _ = synth.sample_object(n, 42)
src, T_gt = synth.make_scene(n, 42)
vox = float(np.float32(synth.mean_spacing(n))); thr = 1.5 * vox
tree = cKDTree(tgt)
p_t = src @ T_gt[:3, :3].T + T_gt[:3, 3]
nn = tree.query(p_t)[1]
rng = np.random.default_rng(1234)
corr = np.where(rng.random(n) < 0.5, nn, rng.integers(0, n, n))
P = src.astype(np.float64); Q = tgt[corr].astype(np.float64)
print("vox", vox, "extent P", P.max(0)-P.min(0), "Q", Q.max(0)-Q.min(0))

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

R0, t0 = T_gt[:3, :3].astype(np.float64), T_gt[:3, 3].astype(np.float64)
best = int((np.linalg.norm(P @ R0.T + t0 - Q, axis=1) < thr).sum())
print("best (true pose) inliers", best)
H = 400
hyps = []; ntrue = []
for h in range(H):
    tri = rng.integers(0, n, 3)
    hyps.append(kabsch(P[tri], Q[tri])); ntrue.append(int((corr[tri] == nn[tri]).sum()))
ntrue = np.array(ntrue)
cnt = np.array([(np.linalg.norm(P @ R.T + t - Q, axis=1) < thr).sum() for R, t in hyps])
print("hyp inlier counts: all-true median %d, others max %d" % (np.median(cnt[ntrue == 3]) if (ntrue==3).any() else -1, cnt[ntrue < 3].max()))
orders = {
  '6d b3': lambda: morton(np.concatenate([P, Q], 1), 3),
  '6d b4': lambda: morton(np.concatenate([P, Q], 1), 4),
  '6d b5': lambda: morton(np.concatenate([P, Q], 1), 5),
  'p b10': lambda: morton(P, 10),
  'p b7 then q b7': lambda: morton(P, 7) * (1 << 21) + morton(Q, 7),
}
for name, kf in orders.items():
  for LEAF in (32, 64):
    order = np.argsort(kf(), kind='stable')
    Ps, Qs = P[order], Q[order]
    nl = -(-n // LEAF); pad = nl * LEAF - n
    Pp = np.concatenate([Ps, np.repeat(Ps[-1:], pad, 0)]); Qp = np.concatenate([Qs, np.repeat(Qs[-1:], pad, 0)])
    Pl = Pp.reshape(nl, LEAF, 3); Ql = Qp.reshape(nl, LEAF, 3)
    sz = np.full(nl, LEAF); sz[-1] = LEAF - pad
    Pmin, Pmax, Qmin, Qmax = Pl.min(1), Pl.max(1), Ql.min(1), Ql.max(1)
    c = (Pmin + Pmax) / 2; e = (Pmax - Pmin) / 2
    ub = []
    for R, t in hyps:
        xc = c @ R.T + t; xe = e @ np.abs(R).T
        gap = np.maximum(0, np.maximum((xc - xe) - Qmax, Qmin - (xc + xe)))
        ub.append(sz[(gap ** 2).sum(1) < thr * thr].sum())
    ub = np.array(ub)
    surv = ub > best
    print("%-16s leaf %2d: UB/N median %.3f p90 %.3f max(non-all-true) %.3f | survive UB>best: %.3f of hyps (all-true %d/%d, other %d/%d)" % (
        name, LEAF, np.median(ub)/n, np.percentile(ub, 90)/n, ub[ntrue<3].max()/n, surv.mean(), surv[ntrue==3].sum(), (ntrue==3).sum(), surv[ntrue<3].sum(), (ntrue<3).sum()))
    # also: prune with best*0.5 (early batch) 
