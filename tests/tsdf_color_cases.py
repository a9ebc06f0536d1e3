"""Colour images for tests/tsdf_cases.py's small scene (tests/test_tsdf_color_abi.py, tests/test_gpu_tsdf_color.py,
tests/test_gpu_tsdf_color_state.py): uint8 [n, h, w, 3], B, G, R, one per depth frame.
  random_images  seeded random bytes that include 0 and 255: for the byte-for-byte tests, where any bytes will do.
  ramp_images    a texture painted on the part, each channel a linear ramp of the part-frame x and y: a hit pixel is deprojected with its
                 rendered depth and the inverse of its frame's pose, and gets the texture at that point, rounded to the nearest byte.  For
                 the accuracy test, which needs to know the colour the surface has where a crossing lies.
Everything comes from the frames and fixed numbers."""
import numpy as np

F = np.float32
# channel = RAMP_OFFSET + RAMP_GRADIENT . (x, y), per metre; inside [0.05, 0.95] on the small scene's part (60 x 30 mm)
RAMP_OFFSET = np.array([0.5, 0.5, 0.5])                                            # r, g, b
RAMP_GRADIENT = np.array([[15.0, 0.0], [0.0, 30.0], [7.0, -14.0]])


def random_images(frames, seed=7):
    frames = np.asarray(frames)
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, frames.shape + (3,), dtype=np.uint8)
    if img.size >= 6:                                                              # both ends of the byte range, whatever the draw
        img.reshape(-1)[:6] = (0, 255, 0, 255, 255, 0)
        img.reshape(-1, 3)[rng.permutation(img.size // 3)[:max(img.size // 30, 2)]] = rng.choice(np.array([0, 255], np.uint8), 3)
    return img


def ramp(xy):
    """The texture (r, g, b) at the part-frame points xy [n, 2], float64."""
    return RAMP_OFFSET[None, :] + np.asarray(xy, np.float64) @ RAMP_GRADIENT.T


def ramp_images(frames, poses, intr):
    """frames uint16 [n, h, w] at MODEL_TO_CAMERA poses [n, 4, 4] (the part's frame to the camera's), intr = (scale, fx, fy, cx, cy)."""
    frames = np.asarray(frames, np.uint16)
    scale, fx, fy, cx, cy = (float(x) for x in intr)
    n, h, w = frames.shape
    vv, uu = np.mgrid[0:h, 0:w]
    img = np.zeros((n, h, w, 3), np.uint8)
    for k in range(n):
        z = frames[k].astype(np.float64) / scale
        cam = np.stack([(uu - cx) * z / fx, (vv - cy) * z / fy, z, np.ones_like(z)], -1)
        part = cam @ np.linalg.inv(np.asarray(poses[k], np.float64)).T
        rgb = ramp(part[..., :2].reshape(-1, 2)).reshape(h, w, 3)
        assert ((rgb > 0.0) & (rgb < 1.0))[frames[k] != 0].all(), "the ramp leaves [0, 1] on the part"
        img[k] = np.where((frames[k] != 0)[..., None], np.round(np.clip(rgb, 0, 1) * 255.0), 0).astype(np.uint8)[..., ::-1]     # RGB -> BGR
    return img
