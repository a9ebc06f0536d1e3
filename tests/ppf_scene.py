"""Shared workload of the PPF tests: the relief part of 3dvision_amd/synth.py as a model of about 300 points with outward normals, and a
scene of about 1,500 points - the part at a known pose seen from a camera at the origin, the floor patch it lies on, and 10 % clutter -
with normals turned towards the camera, as a scan's are.  T_gt moves the scene onto the model.  Chosen on the CPU so that the numpy
restatement alone finds the pose (tests/test_ppf_abi.py); the GPU tests inherit it."""
import numpy as np

import ppf_restatement as R

F = np.float32
MODEL_STEP, SCENE_STEP, FLOOR_STEP = 0.0057, 0.0031, 0.0075
THR = 0.004                    # the ICP / scoring threshold of the tests: a little above the scene's spacing
ICP_ITERS = 50


def _surface(part, step, offset=0.0):
    """Points of the top surface on a grid of `step` (shifted by `offset`) and their unit normals (-dh/dx, -dh/dy, 1), by central differences."""
    h = 1e-5
    fine = lambda x, y: _height(part, x, y)
    xs = np.arange(-part.L / 2 + offset, part.L / 2 + 1e-9, step)
    ys = np.arange(-part.W / 2 + offset, part.W / 2 + 1e-9, step)
    X, Y = np.meshgrid(xs, ys)
    X, Y = X.ravel(), Y.ravel()
    Z = fine(X, Y)
    n = np.stack([-(fine(X + h, Y) - fine(X - h, Y)) / (2 * h), -(fine(X, Y + h) - fine(X, Y - h)) / (2 * h), np.ones_like(X)], 1)
    return np.stack([X, Y, Z], 1), n / np.linalg.norm(n, axis=1, keepdims=True)


def _height(part, x, y):
    z = np.zeros_like(x)
    for bx, by, amp, sx, sy, rot in part.bumps:
        c, s = np.cos(rot), np.sin(rot)
        u = (x - bx) * c + (y - by) * s; v = -(x - bx) * s + (y - by) * c
        z += amp * np.exp(-0.5 * ((u / sx) ** 2 + (v / sy) ** 2))
    return z


def build(synth, seed=3, instance=1):
    part = synth.ReliefPart(seed)
    rng = np.random.default_rng(seed)
    mp, mn = _surface(part, MODEL_STEP)
    sp, sn = _surface(part, SCENE_STEP, offset=0.0011)
    # the floor the part lies on: a frame around it, normals up
    fx = np.arange(-part.L / 2 - 0.03, part.L / 2 + 0.03 + 1e-9, FLOOR_STEP)
    fy = np.arange(-part.W / 2 - 0.03, part.W / 2 + 0.03 + 1e-9, FLOOR_STEP)
    FX, FY = (a.ravel() for a in np.meshgrid(fx, fy))
    out = (np.abs(FX) > part.L / 2 + 0.002) | (np.abs(FY) > part.W / 2 + 0.002)
    fp = np.stack([FX[out], FY[out], np.full(out.sum(), -0.004)], 1)
    fn = np.tile([0.0, 0.0, 1.0], (len(fp), 1))
    S = synth.instance_pose(instance, 0.5, 30.0)               # part frame -> camera frame
    pts = np.concatenate([sp, fp]) @ S[:3, :3].T + S[:3, 3]
    nrm = np.concatenate([sn, fn]) @ S[:3, :3].T
    pts = pts + rng.normal(0, 1e-4, pts.shape)
    seen = (nrm * -pts).sum(1) > 0                             # one side: what faces the camera
    pts, nrm = pts[seen], nrm[seen]
    nc = len(pts) // 9                                         # 10 % of the total
    lo, hi = pts.min(0), pts.max(0)
    cp = lo + rng.random((nc, 3)) * (hi - lo)
    cn = rng.normal(size=(nc, 3)); cn /= np.linalg.norm(cn, axis=1, keepdims=True)
    cn[(cn * -cp).sum(1) < 0] *= -1                            # consistently oriented: towards the camera
    pts, nrm = np.concatenate([pts, cp]), np.concatenate([nrm, cn])
    o = rng.permutation(len(pts))
    sc = dict(model=mp.astype(F), model_normals=mn.astype(F), scene=pts[o].astype(F), scene_normals=nrm[o].astype(F), T_gt=np.linalg.inv(S))
    for a in sc.values():
        a.setflags(write=False)
    return sc


_RESTATED = {}


def restated(synth):
    """The restatement on the scene at the default parameters, computed once per process and never modified: dict(model, peaks, poses)."""
    if "ref" not in _RESTATED:
        sc = build(synth)
        model, pk, poses = R.match(sc["scene"], sc["scene_normals"], sc["model"], sc["model_normals"])
        pk.setflags(write=False)
        _RESTATED["ref"] = dict(model=model, peaks=pk, poses=poses)
    return _RESTATED["ref"]
