"""Hand-built world-space clouds for the GPU parity tests (test_gpu_quirks.py, test_gpu_limits.py).

The calibration is the identity rotation plus a shift of -0.5 m in z (camera z = world z + 0.5 > 0, so that negative world
heights exist); `cloud()` takes world coordinates and returns the camera-space float32 frame [H, W, 3] both implementations read.
"""
import numpy as np

Z_SHIFT = 0.5


def calibration(ssd, z_shift=Z_SHIFT):
    t = ssd.GeometricTransformation()                   # identity (transformation.h:51-55) ...
    t.constants.b[2] = -z_shift                         # ... with the camera `z_shift` below the world origin
    return t


def plane_points(z, n, x_range, y_range, nx=None):
    """n points of a plane at height z on a regular grid inside the world rectangle (so that they rasterise to a solid block);
    nx columns (default: a square grid; images of very unequal pixel sides want one column per pixel column)"""
    (x0, x1), (y0, y1) = x_range, y_range
    if nx is None:
        nx = max(1, int(round(np.sqrt(n * (x1 - x0) / max(y1 - y0, 1e-9)))))
    ny = (n + nx - 1) // nx
    gx, gy = np.meshgrid(np.linspace(x0, x1, nx), np.linspace(y0, y1, ny))
    return np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], 1)[:n]


def cloud(planes, width, height, extra=None, seed=0, z_shift=Z_SHIFT):
    """planes: list of (z, n_points, (x0, x1), (y0, y1)[, nx]) in world coordinates -> float32 [height, width, 3]; the points
    land on random pixels of the camera frame (in their order), the rest of the frame is invalid (0, 0, 0)."""
    rng = np.random.default_rng(seed)
    pts = [plane_points(*pl) for pl in planes]
    if extra is not None:
        pts.append(np.asarray(extra, dtype=np.float64))
    p = np.concatenate(pts) if pts else np.zeros((0, 3))
    n = width * height
    assert len(p) <= n
    out = np.zeros((n, 3), dtype=np.float32)
    idx = rng.permutation(n)[:len(p)]
    p = p.copy()
    p[:, 2] += z_shift                                  # world -> camera
    out[np.sort(idx)] = p.astype(np.float32)
    return out.reshape(height, width, 3)
