"""The ground fit restated for the tests (include/ssd_hip.h): the floor-point rule and its integer moments in
numpy, the scenes and priors the CPU and the GPU tests share, and the host-path refinement the accuracy figures come from
(profiles/ground_fit_accuracy.txt, written by tools/ground_fit_accuracy.py).  TEST INFRASTRUCTURE; no GPU needed."""
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 256, 192
TOLERANCES = (0.08, 0.03, 0.012)
MIN_POINTS = 2000
PRIOR_OFF = (3.0, 2.0, 0.04)                 # degrees of pitch, degrees of roll, metres of height
POSE = dict(cam_height=1.0, pitch_deg=50.0, roll_deg=0.0)


def moments_np(cfg, cal, pts, tol):
    """the rule on float32 camera points [N, 3] -> (n, [3 sums], [6 sums]) as Python ints"""
    p32 = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    a, b = list(cal.a), list(cal.b)
    with np.errstate(invalid="ignore", over="ignore"):
        wx = ((a[0] * x + a[1] * y) + a[2] * z) + b[0]
        wy = ((a[3] * x + a[4] * y) + a[5] * z) + b[1]
        wz = ((a[6] * x + a[7] * y) + a[8] * z) + b[2]
        q = np.rint(p * 65536)
        ok = (p32[:, 2] > 0) & (wx > cfg.x_min) & (wx < cfg.x_max) & (wy > cfg.y_min) & (wy < cfg.y_max) & (-tol <= wz) & (wz <= tol) \
            & np.all(np.abs(q) < 2 ** 20, axis=1)
    qi = q[ok].astype(np.int64)
    return moments_of_q(qi)


def moments_of_q(qi):
    """exact sums of integer points [n, 3]"""
    qi = np.asarray(qi, dtype=np.int64).reshape(-1, 3)
    s = [int(v) for v in qi.sum(axis=0)]
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    ss = [int(np.sum(qi[:, i] * qi[:, j])) for i, j in pairs]
    return len(qi), s, ss


def moments_tuple(m):
    return int(m.n), [int(v) for v in m.s], [int(v) for v in m.ss]


def moments_struct(ssd, n, s, ss):
    m = ssd.GroundMoments()
    m.n = n
    m.s[:] = s
    m.ss[:] = ss
    return m


def scatter_exact(n, s, ss):
    """N SS - S (x) S as Python ints, 3 x 3"""
    at = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    return [[n * ss[at[i][j]] - s[i] * s[j] for j in range(3)] for i in range(3)]


def eigh_of(n, s, ss):
    """numpy's word on the same scatter, in m^2: (ascending eigenvalues, unit normal of the smallest signed towards the centroid, dist)"""
    c = np.array([[float(v) for v in row] for row in scatter_exact(n, s, ss)]) / (float(n) * float(n) * 65536.0 * 65536.0)
    lam, vec = np.linalg.eigh(c)
    n0 = vec[:, 0] / np.linalg.norm(vec[:, 0])
    centroid = np.array([float(v) for v in s]) / (n * 65536.0)
    if n0 @ centroid < 0:
        n0 = -n0
    return lam, n0, float(n0 @ centroid)


def angle(u, v):
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return math.atan2(np.linalg.norm(np.cross(u, v)), float(u @ v))


def plane_of(cal):
    """(n0, dist) a calibration's CameraToWorld stands for"""
    return np.array([-cal.a[6], -cal.a[7], -cal.a[8]]), float(cal.b[2])


def scene(ssd, kind, seed=7, width=W, height=H, sign=0, **kw):
    """kind: 'floor' (bare, no noise), 'steps' (3 steps), 'outliers' (5 %), 'invalid' (10 % invalid pixels); sign != 0: the pose moved by
    sign * PRIOR_OFF - what a rough prior is the calibration of"""
    args = dict(POSE, n_steps=3, sigma=0.001, seed=seed)
    if kind == "floor":
        args.update(n_steps=0, sigma=0.0)
    elif kind == "outliers":
        args.update(outlier_frac=0.05)
    elif kind == "invalid":
        args.update(invalid_frac=0.10)
    args.update(kw)
    args["pitch_deg"] += sign * PRIOR_OFF[0]
    args["roll_deg"] += sign * PRIOR_OFF[1]
    args["cam_height"] += sign * PRIOR_OFF[2]
    return ssd.make_scene(width, height, **args)


def refine_host(ssd, cfg, frame, prior_cal, tolerances=TOLERANCES, min_points=MIN_POINTS):
    """Detector.refine_calibration for one frame on the host functions -> the last pass's GroundFit (OK passes chained)"""
    cal, fit = prior_cal, None
    for tol in tolerances:
        fit = ssd.ground_fit_solve(ssd.ground_moments_host(cfg, cal, frame, tol), cal, min_points)
        cal = fit.cal
    return fit


def errors(fit, truth_cal):
    """(angle between the fitted and the true normal in radians, |height error| in metres)"""
    n0, dist = plane_of(truth_cal)
    return angle(list(fit.normal), n0), abs(fit.dist - dist)


def accuracy_cases(ssd):
    """the 3-step scene at sigma 1 mm and 3 mm under the priors +-PRIOR_OFF: (name, cfg, frame, truth, prior) each"""
    out = []
    cfg = ssd.default_config(W, H)
    for sigma in (0.001, 0.003):
        sc = scene(ssd, "steps", sigma=sigma)
        frame = ssd.synth_host([sc])[0]
        truth = ssd.transformation_for_scene(sc).constants
        for sign in (+1, -1):
            prior = ssd.transformation_for_scene(scene(ssd, "steps", sigma=sigma, sign=sign)).constants
            out.append(("sigma %g mm, prior %+d x (3 deg, 2 deg, 4 cm)" % (sigma * 1e3, sign), cfg, frame, truth, prior))
    return out


ACCURACY_FILE = os.path.join(ROOT, "profiles", "ground_fit_accuracy.txt")


def recorded_accuracy():
    """{'worst_angle_rad', 'worst_height_m'} from profiles/ground_fit_accuracy.txt"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out
