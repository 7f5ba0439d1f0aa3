"""The riser fit restated for the tests (include/ssd_hip.h, DESIGN.md sections 7 and 7f): which points are evidence of which riser, from
a frame's record alone, in numpy doubles; the oracle-to-planes chain on the host functions; and the scenes the accuracy figures come
from (profiles/riser_fit_accuracy.txt, written by tools/riser_fit_accuracy.py).  TEST INFRASTRUCTURE; no GPU needed.

riser_labels() restates what k_final prepares for k_risers (the emitted surfaces with their camera-dependent-world heights and front
corners; zLo / zHi, u, len per riser; the bins of no plateau handed to the lowest riser whose bin range holds them) and then the point
rule of section 7.  `rec` is a frame record with the fields of ssd_debug_frame: the oracle's record (heights = the reference's running
double means) and a handle's debug record (heights = its fixed-point means) both serve, and each gives the labels of ITS risers.
"""
import math
import os

import numpy as np

import ground_model as gm
import oracle_binding as ob
from test_labels import effective_bins, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = gm.W, gm.H
TOL = 0.03
MIN_POINTS = 100
SIGMAS = (0.001, 0.003)
OFFSET_FIX = float(1 << 40)


def emitted(rec, limit=ob.MAX_STEPS):
    """the emitted surfaces in k_final's order: [(z, front-left x, y, front-right x, y)] in camera-dependent world coordinates; limit:
    the surfaces the record's maker can report (the oracle: all of them; a handle: SSD_MAX_STEPS, which shows on an overflowing frame)"""
    if (rec.status & ob.ST_THROW) or rec.first_valid_ind < 0:
        return []
    out = []
    if rec.ground_ind >= 0:
        # quirk Q6: a ground whose front edge is not found is the all-zero surface; its corners are no riser's (it is the lowest)
        out.append((rec.ground_mean_z if rec.ground_front_valid else 0.0, 0.0, 0.0, 0.0, 0.0))
    for k in range(rec.first_valid_ind, rec.n_plateaus):
        pl = rec.plateaus[k]
        if pl.valid:
            q = list(pl.quad_world)
            out.append((pl.mean_z, q[0], q[1], q[2], q[3]))
    return out[:limit]


def risers_of(cfg, rec, limit=ob.MAX_STEPS):
    """-> ([dict(ox, oy, ux, uy, len, zLo, zHi)] per riser, riser_of_bin as an int array of n_bins entries, -1 = none)"""
    surf = emitted(rec, limit)
    n_bins = rec.n_bins
    recip = 1.0 / cfg.height_interval
    free = np.ones(n_bins, dtype=bool)                      # the bins of no plateau
    for lo, hi in effective_bins(rec):
        free[max(lo, 0):hi + 1] = False
    of_bin = np.full(n_bins, -1, dtype=np.int64)
    out = []
    for i in range(max(len(surf) - 1, 0)):
        lower, upper = surf[i], surf[i + 1]
        dx, dy = upper[3] - upper[1], upper[4] - upper[2]
        ln = math.sqrt(dx * dx + dy * dy)
        z_lo, z_hi = lower[0] + cfg.height_interval, upper[0] - cfg.height_interval
        usable = ln > 0.0 and z_lo < z_hi
        out.append(dict(ox=upper[1], oy=upper[2], ux=dx / ln if usable else 0.0, uy=dy / ln if usable else 0.0,
                        len=ln if usable else -1.0, zLo=z_lo, zHi=z_hi))
        if usable:
            b_lo = max(0, min(int((z_lo - cfg.z_min) * recip), n_bins - 1))
            b_hi = max(0, min(int((z_hi - cfg.z_min) * recip), n_bins - 1))
            for b in range(b_lo, b_hi + 1):
                if free[b] and of_bin[b] < 0:
                    of_bin[b] = i
    return out, of_bin


def evidence(cfg, cal, rec, xyz, tol, limit=ob.MAX_STEPS):
    """-> (labels uint8 [W H]: i + 1 = evidence of riser i, s float64 [W H]: the point's signed distance from its riser's edge line)"""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    labels = np.zeros(len(p), dtype=np.uint8)
    off = np.zeros(len(p), dtype=np.float64)
    rs, of_bin = risers_of(cfg, rec, limit)
    if not rs:
        return labels, off
    wx, wy, wz = world(cal, p)
    ok = (p[:, 2] > 0) & (wx > cfg.x_min) & (wx < cfg.x_max) & (wy > cfg.y_min) & (wy < cfg.y_max) & (wz > cfg.z_min) & (wz < cfg.z_max)
    with np.errstate(invalid="ignore"):
        hbin = np.where(ok, (wz - cfg.z_min) * (1.0 / cfg.height_interval), -1.0).astype(np.int64)
    ok &= (hbin >= 0) & (hbin < len(of_bin))
    r_of = np.where(ok, of_bin[np.clip(hbin, 0, len(of_bin) - 1)], -1)
    for i, r in enumerate(rs):
        mine = (r_of == i) & (wz > r["zLo"]) & (wz < r["zHi"])
        a, b = wx - r["ox"], wy - r["oy"]
        s = b * r["ux"] - a * r["uy"]
        t = a * r["ux"] + b * r["uy"]
        mine &= (np.abs(s) <= tol) & (t >= 0.0) & (t <= r["len"])
        labels[mine] = i + 1
        off[mine] = s[mine]
    return labels, off


def riser_labels(cfg, cal, rec, xyz, tol, limit=ob.MAX_STEPS):
    """uint8 [W H]: label i + 1 = the point is evidence of riser i of the frame whose record is `rec`, 0 = of none"""
    return evidence(cfg, cal, rec, xyz, tol, limit)[0]


def counts_and_offsets(labels, off, n):
    """[(count, mean offset as k_riser_results forms it: the sum of round(s 2^40) over 2^40 over the count)] of labels 1 .. n"""
    out = []
    for i in range(n):
        s = off[labels == i + 1]
        tot = int(np.rint(s * OFFSET_FIX).astype(np.int64).sum(dtype=np.int64))
        out.append((len(s), (float(tot) / OFFSET_FIX) / len(s) if len(s) else 0.0))
    return out


def frame_risers(ssd, ora):
    """the oracle's list of Riser -> ssd.FrameRisers (what ssd_riser_fit_solve reads: the heights and the drawn edge)"""
    fr = ssd.FrameRisers()
    fr.n_risers = len(ora)
    for i, o in enumerate(ora):
        r = fr.risers[i]
        r.n_points, r.detected, r.height_bottom, r.height_top, r.mean_offset = o.n_points, o.detected, o.height_bottom, o.height_top, o.mean_offset
        r.left[:] = list(o.left)
        r.right[:] = list(o.right)
    return fr


def oracle_planes(ssd, oracle, cfg, cal, xyz, tol=TOL, min_points=MIN_POINTS):
    """oracle -> riser_labels -> ssd_surface_moments_host -> ssd_riser_fit_solve: (oracle's risers, labels, FrameMoments, FrameRiserFits)"""
    ocfg, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal)
    rec = oracle.process(ocfg, ocal, xyz)[0]
    ora = oracle.risers(ocfg, ocal, xyz, tol, 1)
    labels = riser_labels(cfg, cal, rec, xyz, tol)
    fm = ssd.surface_moments_host(cfg, xyz, labels, len(ora), 0)
    return ora, labels, fm, ssd.riser_fit_solve(fm, frame_risers(ssd, ora), cal, min_points)


def accuracy_cases(ssd):
    """the 3-step 256 x 192 scene of ground_model at sigma 1 mm and 3 mm, under the true calibration: (name, cfg, frame, cal, scene)"""
    out = []
    cfg = ssd.default_config(W, H)
    for sigma in SIGMAS:
        sc = gm.scene(ssd, "steps", sigma=sigma)
        out.append(("sigma %g mm" % (sigma * 1e3), cfg, ssd.synth_host([sc])[0], ssd.transformation_for_scene(sc).constants, sc))
    return out


def accuracy_of(ssd, oracle, cfg, frame, cal, sc):
    """the scene's risers are vertical, parallel to the edges and one tread apart:
    -> (statuses, worst |lean|, worst skew, worst |going - tread| over the OK risers (goings: where set), rows for the record)"""
    ora, _, fm, fit = oracle_planes(ssd, oracle, cfg, cal, frame)
    ok = [i for i in range(fit.n_risers) if fit.r[i].status == ssd.GF_OK]
    lean = max([abs(fit.r[i].lean) for i in ok], default=0.0)
    skew = max([fit.r[i].skew for i in ok], default=0.0)
    pairs = [i for i in ok if i + 1 in ok]
    going = max([abs(fit.r[i].going - sc.tread) for i in pairs], default=0.0)
    rows = [(i, fit.r[i].status, int(fit.r[i].n), fit.r[i].lean, fit.r[i].skew, fit.r[i].rms, fit.r[i].rise, fit.r[i].going) for i in range(fit.n_risers)]
    return [fit.r[i].status for i in range(fit.n_risers)], lean, skew, going, len(pairs), rows


ACCURACY_FILE = os.path.join(ROOT, "profiles", "riser_fit_accuracy.txt")


def recorded_accuracy():
    """{'worst_lean_rad', 'worst_skew_rad', 'worst_going_error_m'} from profiles/riser_fit_accuracy.txt"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out
