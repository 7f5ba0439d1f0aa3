"""Drift per camera from refit records, restated for the tests (include/ssd_hip.h): the cameras of
tests/camera_drift_model.py with what a refit needs kept (frames and labels), the chain first fit -> gates -> refit -> fold on the host
functions with per-frame gates or with the camera's folded floor plane in front of the last pass (ssd_camera_ground_gates), and the
columns the accuracy figures come from (profiles/camera_drift_refit_accuracy.txt, written by tools/camera_drift_refit_accuracy.py).
TEST INFRASTRUCTURE; no GPU needed."""
import os

import camera_drift_model as cdm
import ground_model as gm
import surface_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SIGMAS = (2.5, 2.0)
PASSES = (1, 2)
# a column: "first", or (k_sigma, passes, camera gates in front of the last pass)
COLUMNS = ["first"] + [(ks, p, cam) for cam in (False, True) for ks in K_SIGMAS for p in PASSES]
ACCURACY_FILE = os.path.join(ROOT, "profiles", "camera_drift_refit_accuracy.txt")


def column_key(c):
    return "first" if c == "first" else "k%s_pass%d%s" % (("%g" % c[0]).replace(".", "p"), c[1], "_camera" if c[2] else "")


def camera_frames(ssd, oracle, offset):
    """camera_drift_model.camera_case, keeping each frame and its labels: FRAMES of the true pose, detected (the oracle's labels) under
    the table entry `offset` away from it -> (truth, entry, cfg, [(frame, labels, first-pass FrameMoments)])"""
    cfg = ssd.default_config(cdm.W, cdm.H)
    entry_kw = {k: gm.POSE[k] + v for k, v in offset.items()}
    truth = entry = None
    frames = []
    for seed, sigma in cdm.FRAMES:
        sc = gm.scene(ssd, "steps", seed=seed, sigma=sigma)
        if truth is None:
            truth = ssd.transformation_for_scene(sc).constants
            entry = ssd.transformation_for_scene(gm.scene(ssd, "steps", seed=seed, sigma=sigma, **entry_kw)).constants
        frame = ssd.synth_host([sc])[0]
        _, labels, fm, _ = sm.oracle_planes(ssd, oracle, cfg, entry, frame)
        frames.append((frame, labels, fm))
    return truth, entry, cfg, frames


def refit_records(ssd, cfg, entry, frames, k_sigma, passes, camera_gates, gate_min=0.0, min_points=sm.MIN_POINTS, fold_min_points=cdm.MIN_POINTS):
    """the frames of ONE camera through `passes` refit passes on the host functions, each pass gated by the planes of the one before
    (ssd_surface_gates_from_moments per frame); camera_gates: in front of the last pass the ground gates become the camera's - the fold
    of the records so far against `entry`, through ssd_camera_ground_gates -> [FrameMoments of the last pass]"""
    cur = [fm for _, _, fm in frames]
    idx = [0] * len(frames)
    for p in range(passes):
        gates = [ssd.surface_gates_from_moments(m, min_points, k_sigma, gate_min) for m in cur]
        if camera_gates and p == passes - 1:
            drift = ssd.camera_drift_fold(cur, idx, [entry], min_points=fold_min_points)
            gates = ssd.camera_ground_gates(cur, idx, drift, gates, k_sigma, gate_min)
        cur = [ssd.surface_refit_moments_host(cfg, f, lab, g, fm.n_surfaces, fm.ground) for (f, lab, fm), g in zip(frames, gates)]
    return cur


def ground_points(fm):
    return int(fm.s[0].m.n + fm.s[0].n_far) if fm.ground == 1 and fm.n_surfaces >= 1 else 0


def accuracy_rows(ssd, oracle, entries=cdm.ENTRIES, columns=COLUMNS):
    """per table entry of camera_drift_model: (name, {column: (tilt error, height error, normal error, status, ground points folded,
    the share of the first-pass fold's ground points the fold kept, the least share of a FRAME's first-pass ground points kept)}) - the
    errors against the scene generator's true pose"""
    out = []
    for name, offset in entries:
        truth, entry, cfg, frames = camera_frames(ssd, oracle, offset)
        first = [fm for _, _, fm in frames]
        total = sum(ground_points(f) for f in first)
        row = {}
        for c in columns:
            recs = first if c == "first" else refit_records(ssd, cfg, entry, frames, c[0], c[1], c[2])
            d = ssd.camera_drift_fold(recs, [0] * len(recs), [entry], min_points=cdm.MIN_POINTS)[0]
            share = min(ground_points(r) / ground_points(f) for r, f in zip(recs, first) if ground_points(f))
            row[c] = cdm.drift_errors(d.fit, truth, entry) + (int(d.fit.status), int(d.m.n), int(d.m.n + d.n_far) / total, share)
        out.append((name, row))
    return out


def worst_columns(rows, columns=COLUMNS):
    """{column: (worst tilt error, worst height error, least share kept by a fold, least share kept of a frame)}, the errors over the
    entries whose fold is OK"""
    return {c: (max(r[c][0] for _, r in rows if r[c][3] == 0), max(r[c][1] for _, r in rows if r[c][3] == 0), min(r[c][5] for _, r in rows),
                min(r[c][6] for _, r in rows)) for c in columns}


def recorded_accuracy():
    """{'worst_tilt_error_rad_first', 'worst_height_error_m_k2p5_pass1_camera', ..} from profiles/camera_drift_refit_accuracy.txt"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out
