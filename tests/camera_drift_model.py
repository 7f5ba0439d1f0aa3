"""Drift per camera restated for the tests (include/ssd_hip.h): the fold in Python integers, and the scenes,
table entries and error measures the accuracy figures come from (profiles/camera_drift_accuracy.txt, written by
tools/camera_drift_accuracy.py).  TEST INFRASTRUCTURE; no GPU needed."""
import os

import ground_model as gm
import surface_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = gm.W, gm.H
MIN_POINTS = gm.MIN_POINTS
# the frames of one camera: the same 3-step scene, another seed and another noise each
FRAMES = [(7, 0.001), (8, 0.0015), (9, 0.002), (10, 0.003)]
# how a camera's table entry differs from its true pose.  The first two are the test's cameras (tests/test_camera_surfaces.py):
# a true entry, and one pitched by 1 degree and lowered by 2 cm; the tool measures the others as well.
ENTRIES = [("true", {}), ("pitch +1 deg, 2 cm lower", dict(pitch_deg=1.0, cam_height=-0.02)),
           ("pitch -1 deg, 2 cm higher", dict(pitch_deg=-1.0, cam_height=0.02)), ("roll +1 deg, 1 cm lower", dict(roll_deg=1.0, cam_height=-0.01)),
           ("roll -0.5 deg, pitch +0.5 deg", dict(roll_deg=-0.5, pitch_deg=0.5))]
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


def sums_of(sm_rec):
    """a SurfaceMoments as eleven Python ints: n, s[3], ss[6], n_far"""
    n, s, ss = gm.moments_tuple(sm_rec.m)
    return [n] + s + ss + [int(sm_rec.n_far)]


def fold_py(moments, camera_of_frame, ncams):
    """the fold in Python integers -> per camera (frames, frames_ground, frames_left, eleven sums): in index order, a frame whole or not
    at all, skipped when a sum would leave int64"""
    out = [[0, 0, 0, [0] * 11] for _ in range(ncams)]
    for fm, c in zip(moments, camera_of_frame):
        rec = out[c]
        rec[0] += 1
        if fm.ground != 1 or fm.n_surfaces < 1:
            continue
        new = [a + b for a, b in zip(rec[3], sums_of(fm.s[0]))]
        if any(v > INT64_MAX or v < INT64_MIN for v in new):
            rec[2] += 1
            continue
        rec[3] = new
        rec[1] += 1
    return [tuple(r) for r in out]


def drift_tuple(d):
    """a CameraDrift's counts and sums as fold_py gives them"""
    n, s, ss = gm.moments_tuple(d.m)
    return int(d.frames), int(d.frames_ground), int(d.frames_left), [n] + s + ss + [int(d.n_far)]


def camera_case(ssd, oracle, offset):
    """one camera: FRAMES of the true pose, detected (the oracle's labels) under the table entry `offset` away from it
    -> (truth, entry, [FrameMoments per frame])"""
    cfg = ssd.default_config(W, H)
    entry_kw = {k: gm.POSE[k] + v for k, v in offset.items()}
    truth = entry = None
    moments = []
    for seed, sigma in FRAMES:
        sc = gm.scene(ssd, "steps", seed=seed, sigma=sigma)
        if truth is None:
            truth = ssd.transformation_for_scene(sc).constants
            entry = ssd.transformation_for_scene(gm.scene(ssd, "steps", seed=seed, sigma=sigma, **entry_kw)).constants
        frame = ssd.synth_host([sc])[0]
        moments.append(sm.oracle_planes(ssd, oracle, cfg, entry, frame)[2])
    return truth, entry, moments


def drift_errors(fit, truth, entry):
    """against the scene generator's pose, never the code under test: (|fit.tilt - angle between the true floor normal and the entry's|,
    |fit.height_delta - (true camera height - the entry's)|, angle between the fitted and the true normal)"""
    n_true, d_true = gm.plane_of(truth)
    n_entry, d_entry = gm.plane_of(entry)
    return abs(fit.tilt - gm.angle(n_true, n_entry)), abs(fit.height_delta - (d_true - d_entry)), gm.angle(list(fit.normal), n_true)


ACCURACY_FILE = os.path.join(ROOT, "profiles", "camera_drift_accuracy.txt")


def recorded_accuracy():
    """{'worst_tilt_error_rad', 'worst_height_error_m'} from profiles/camera_drift_accuracy.txt"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out
