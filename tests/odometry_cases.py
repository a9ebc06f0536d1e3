"""Scenes for the depth odometry tests (tests/test_odometry_abi.py, tests/test_gpu_odometry.py, tests/test_gpu_odometry_state.py): a small
ReliefPart at 0.3 m rendered from the scan pose and from views turned by a few degrees about a fixed axis, with the ground truth of the
motion between two views.  Rendered with tests/tsdf_cases.py's view_poses and render; everything comes from 3dvision_amd.synth and fixed
numbers.  Poses are row-major [4, 4]."""
import functools
import importlib

import numpy as np

import tsdf_cases

synth = importlib.import_module("3dvision_amd.synth")
F = np.float32
AXIS = [0.3, 1.0, 0.2]
ANGLES = (1.0, 2.0, 4.0)
SIZES = {(96, 72): 230.0, (160, 120): 420.0}
DISTANCE = 0.3
ACCURACY_DEPTH_DIFF = 0.004


@functools.lru_cache(maxsize=None)
def _points():
    return synth.ReliefPart(seed=3, L=0.06, W=0.03, feature=0.006).surface_points(0.0002)


def truth(pose_src, pose_tgt):
    """The motion that takes source-camera coordinates to target-camera coordinates (O5's T) of two MODEL_TO_CAMERA view poses, float64."""
    return np.asarray(pose_tgt, np.float64) @ np.linalg.inv(np.asarray(pose_src, np.float64))


@functools.lru_cache(maxsize=None)
def views(size, angles):
    """dict(frames uint16[n, h, w], intr, poses [n, 4, 4]): the scan pose, then the part turned by each of `angles` degrees about AXIS."""
    poses = tsdf_cases.view_poses(DISTANCE, [(AXIS, 0.0)] + [(AXIS, float(a)) for a in angles])
    frames, intr = tsdf_cases.render(_points(), poses, SIZES[size], *size)
    frames.setflags(write=False)
    return dict(frames=frames, intr=intr, poses=poses)


def pair(size, angle):
    """dict(src, tgt, intr, T_gt): the view turned by `angle` degrees as the source, the scan pose's view as the target."""
    v = views(size, (float(angle),))
    return dict(src=v["frames"][1], tgt=v["frames"][0], intr=v["intr"], T_gt=truth(v["poses"][1], v["poses"][0]))


def pairs():
    """The six pairs of the accuracy condition: ((width, height), degrees) -> pair()."""
    return {(size, a): pair(size, a) for size in SIZES for a in ANGLES}


def sequence(size, n_frames, step=1.0):
    """n_frames views, each turned by `step` degrees more than the one before: dict(frames, intr, poses, T_gt [n, 4, 4] - pair k's truth,
    entry 0 the identity)."""
    v = views(size, tuple(step * k for k in range(1, n_frames)))
    T = [np.eye(4)] + [truth(v["poses"][k], v["poses"][k - 1]) for k in range(1, n_frames)]
    return dict(frames=v["frames"][:n_frames], intr=v["intr"], poses=v["poses"][:n_frames], T_gt=np.stack(T))


def errors(T_est, T_gt):
    """(rotation error in degrees, translation error in metres)."""
    rot, tr = synth.pose_error(np.asarray(T_est, np.float64), T_gt)
    return float(np.degrees(rot)), tr
