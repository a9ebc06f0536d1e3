"""Scenes for the TSDF tests (tests/test_tsdf_abi.py, tests/test_gpu_tsdf.py, tests/test_gpu_tsdf_state.py): a part rendered from a few
camera poses around its scan pose into raw u16 frames, and the volume that holds it.  Poses are MODEL_TO_CAMERA (the part's frame, which
is the volume's, to the camera's), row-major [4, 4].  Everything comes from 3dvision_amd.synth and fixed numbers."""
import importlib

import numpy as np

import tsdf_restatement as R

synth = importlib.import_module("3dvision_amd.synth")
F = np.float32
SCALE = 10000.0


def view_poses(distance, tilts):
    """The scan pose at `distance` with the part turned by each (axis, degrees) of tilts about its own origin."""
    scan = synth.scan_pose(distance)
    return np.stack([scan @ synth.make_transform(axis, deg, (0.0, 0.0, 0.0)).astype(np.float64) for axis, deg in tilts]).astype(F)


FOUR_VIEWS = (([1.0, 0.0, 0.0], 0.0), ([1.0, 0.0, 0.0], 25.0), ([1.0, 0.0, 0.0], -25.0), ([0.0, 1.0, 0.0], 25.0))


def render(points, poses, f, width, height):
    """uint16 [n, height, width] frames of the surface samples, principal point at the centre; intrinsics (scale, fx, fy, cx, cy)."""
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    frames = np.stack([synth.render_depth(points, np.asarray(T, np.float64), f, f, cx, cy, width, height, SCALE)[0] for T in poses])
    return frames, (SCALE, f, f, cx, cy)


def relief_scene():
    """ReliefPart() seen from 0.4 m in four views (FOUR_VIEWS: the scan pose, the part turned by +-25 degrees about x and by 25 about y),
    640 x 480 frames at f = 1400, scale 10000, a volume of 136 x 96 x 40 voxels of 1 mm around the plate.  The surface is sampled every
    0.3 mm, about one sample per pixel (a pixel is 0.29 mm at 0.4 m): a frame has holes where no sample fell, as a sensor's frame has
    dropouts, and the other views see into them."""
    part = synth.ReliefPart()
    poses = view_poses(0.4, FOUR_VIEWS)
    frames, intr = render(part.surface_points(0.0003), poses, 1400.0, 640, 480)
    vol = R.Volume((-0.068, -0.048, -0.016), 0.001, (136, 96, 40))
    return dict(part=part, vol=vol, frames=frames, poses=poses, intr=intr)


def true_surface(part, xyz, step=0.00025):
    """(h, normal) of the part's height field at the points' (x, y): bilinear in a grid of `step`, the normal from central differences."""
    xs, ys, Z = part.height_grid(step)
    gy, gx = np.gradient(Z, step)
    fx = np.clip((xyz[:, 0].astype(np.float64) - xs[0]) / step, 0, len(xs) - 1 - 1e-9)
    fy = np.clip((xyz[:, 1].astype(np.float64) - ys[0]) / step, 0, len(ys) - 1 - 1e-9)
    i, j = fx.astype(int), fy.astype(int)
    a, b = fx - i, fy - j

    def bilinear(A):
        return (A[j, i] * (1 - a) + A[j, i + 1] * a) * (1 - b) + (A[j + 1, i] * (1 - a) + A[j + 1, i + 1] * a) * b

    h, hx, hy = bilinear(Z), bilinear(gx), bilinear(gy)
    n = np.stack([-hx, -hy, np.ones_like(hx)], 1)
    return h, n / np.linalg.norm(n, axis=1, keepdims=True)


def small_scene(dims, n_frames, size=(96, 72), f=230.0, voxel=0.001, distance=0.3, seed=3):
    """A small ReliefPart under a volume of dims voxels (the volume is centred on the part in x and y and may be smaller than it), seen in
    n_frames frames: the scan pose, then tilts of growing angle about alternating axes."""
    part = synth.ReliefPart(seed=seed, L=0.06, W=0.03, feature=0.006)
    tilts = [([1.0, 0.0, 0.0], 0.0)] + [([1.0, 0.0, 0.0] if k % 2 else [0.0, 1.0, 0.0], (5.0 + 0.45 * k) * (-1) ** (k // 2)) for k in range(1, n_frames)]
    if n_frames:
        poses = view_poses(distance, tilts[:n_frames])
        frames, intr = render(part.surface_points(0.0002), poses, f, *size)
    else:
        poses, frames = np.zeros((0, 4, 4), F), np.zeros((0, size[1], size[0]), np.uint16)
        intr = (SCALE, f, f, (size[0] - 1) / 2.0, (size[1] - 1) / 2.0)
    nx, ny, nz = dims
    vol = R.Volume((-nx * voxel / 2.0, -ny * voxel / 2.0, -0.3 * nz * voxel), voxel, dims)
    return dict(part=part, vol=vol, frames=frames, poses=poses, intr=intr)
