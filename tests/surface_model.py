"""The surface fit restated for the tests (include/ssd_hip.h): per-surface integer moments from a label array
in Python integers, the oracle-to-planes chain on the host functions, and the scenes and calibrations the accuracy figures come from
(profiles/surface_fit_accuracy.txt, written by tools/surface_fit_accuracy.py).  TEST INFRASTRUCTURE; no GPU needed."""
import os

import numpy as np

import ground_model as gm
import oracle_binding as ob
from test_labels import expected_labels, surfaces

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = gm.W, gm.H
MIN_POINTS = 200
LIMIT = 1 << 20
# the calibration in use: the true one, and the ones of a pose pitched / rolled by a few tenths of a degree
CAL_OFFSETS = [("true", {}), ("pitch +0.3 deg", dict(pitch_deg=0.3)), ("pitch -0.2 deg", dict(pitch_deg=-0.2)),
               ("roll +0.3 deg", dict(roll_deg=0.3)), ("roll -0.4 deg", dict(roll_deg=-0.4))]
SIGMAS = (0.001, 0.003)


def moments_py(pts, labels, n_surfaces):
    """[(n, [3 sums], [6 sums], n_far)] per surface 0 .. n_surfaces - 1, Python ints: q = rint(double(v) * 65536) of the float32
    camera points [N, 3] labelled k + 1; a point with some |q| >= 2^20 counts in n_far alone"""
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    lab = np.asarray(labels).reshape(-1)
    out = []
    for k in range(n_surfaces):
        n, s, ss, far = 0, [0, 0, 0], [0] * 6, 0
        for i in np.flatnonzero(lab == k + 1):
            q = [int(np.rint(v * 65536.0)) for v in p[i]]
            if any(abs(v) >= LIMIT for v in q):
                far += 1
                continue
            n += 1
            for a in range(3):
                s[a] += q[a]
            for j, (a, b) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
                ss[j] += q[a] * q[b]
        out.append((n, s, ss, far))
    return out


def moments_np(pts, labels, n_surfaces):
    """the same with numpy int64 sums (whole frames): exact, as every sum stays below 2^63"""
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    lab = np.asarray(labels).reshape(-1)
    q = np.rint(p * 65536.0)
    near = np.all(np.abs(q) < LIMIT, axis=1)
    out = []
    for k in range(n_surfaces):
        mine = lab == k + 1
        n, s, ss = gm.moments_of_q(q[mine & near].astype(np.int64))
        out.append((n, s, ss, int((mine & ~near).sum())))
    return out


def frame_tuple(fm):
    """FrameMoments -> (n_surfaces, ground, [(n, s, ss, n_far)] for all SSD_MAX_STEPS records)"""
    return int(fm.n_surfaces), int(fm.ground), [gm.moments_tuple(r.m) + (int(r.n_far),) for r in fm.s]


def pad(rows, total):
    return list(rows) + [(0, [0, 0, 0], [0] * 6, 0)] * (total - len(rows))


def oracle_planes(ssd, oracle, cfg, cal, xyz, min_points=MIN_POINTS):
    """oracle -> expected_labels -> ssd_surface_moments_host -> ssd_surface_fit_solve: (oracle record, labels, FrameMoments, FrameSurfaces)"""
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), xyz)[0]
    labels = expected_labels(oracle, cfg, cal, res, xyz)
    surf = surfaces(res)
    fm = ssd.surface_moments_host(cfg, xyz, labels, len(surf), 1 if surf and surf[0][2] else 0)
    return res, labels, fm, ssd.surface_fit_solve(fm, cal, min_points)


def accuracy_cases(ssd):
    """the 3-step 256 x 192 scene at sigma 1 mm and 3 mm under each calibration of CAL_OFFSETS: (name, cfg, frame, truth, cal in use)"""
    out = []
    cfg = ssd.default_config(W, H)
    for sigma in SIGMAS:
        sc = gm.scene(ssd, "steps", sigma=sigma)
        frame = ssd.synth_host([sc])[0]
        truth = ssd.transformation_for_scene(sc).constants
        for name, off in CAL_OFFSETS:
            kw = {k: gm.POSE[k] + v for k, v in off.items()}
            cal = ssd.transformation_for_scene(gm.scene(ssd, "steps", sigma=sigma, **kw)).constants
            out.append(("sigma %g mm, calibration %s" % (sigma * 1e3, name), cfg, frame, truth, cal))
    return out


def tilt_errors(ssd, oracle, cfg, frame, truth, cal):
    """every surface of the scene is level, so under the calibration in use each shows the angle between the true calibration's up
    vector and that calibration's: -> (that angle, [(surface, status, n, tilt, |tilt - angle|, rms)])"""
    want = gm.angle(gm.plane_of(truth)[0], gm.plane_of(cal)[0])
    res, _, fm, fit = oracle_planes(ssd, oracle, cfg, cal, frame)
    return want, res, [(k, fit.s[k].status, int(fit.s[k].n), fit.s[k].tilt, abs(fit.s[k].tilt - want), fit.s[k].rms) for k in range(fit.n_surfaces)]


ACCURACY_FILE = os.path.join(ROOT, "profiles", "surface_fit_accuracy.txt")


def recorded_accuracy():
    """{'worst_tilt_error_rad'} from profiles/surface_fit_accuracy.txt"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out
