"""The tread clearance rule restated for the tests (include/ssd_hip.h) in numpy, on a result and a calibration:
which points stand on which reported surface, their mask and their exact integer moments; and the frames the CPU and the GPU tests
share - the 3-step scenes with a patch of points pulled off a tread, the full-width frames with raised points.
TEST INFRASTRUCTURE; no GPU needed.  Written from the rule's text, vectorised over the points: it shares no structure with the C text."""
import functools
import os

import numpy as np

import ground_model

RULE = (0.03, 0.03, 0.5)                      # margin, lo, hi: the defaults
WIDE_RULE = (0.03, 0.01, 0.5)                 # the full-width frames' (their steps rise 0.06 m)
W, H = ground_model.W, ground_model.H


def world(cfg, cal, xyz):
    """float32 camera points -> (valid-and-in-range mask, wx, wy, wz) in doubles, each row (a0 x + a1 y) + a2 z, then + b"""
    p32 = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    a, b = [float(v) for v in cal.a], [float(v) for v in cal.b]
    with np.errstate(invalid="ignore", over="ignore"):
        w = [((a[3 * r] * p[:, 0] + a[3 * r + 1] * p[:, 1]) + a[3 * r + 2] * p[:, 2]) + b[r] for r in range(3)]
        ok = (p32[:, 2] > 0) & (w[0] > cfg.x_min) & (w[0] < cfg.x_max) & (w[1] > cfg.y_min) & (w[1] < cfg.y_max) \
            & (w[2] > cfg.z_min) & (w[2] < cfg.z_max)
    return ok, w[0], w[1], w[2]


def inside_shrunk(quad, margin, ex, ey):
    """boolean per point: inside the quadrilateral (quad[8]: FL, FR, BL, BR as x, y pairs) shrunk by margin"""
    ring = [(quad[0], quad[1]), (quad[2], quad[3]), (quad[6], quad[7]), (quad[4], quad[5])]
    t = [ring[i][0] * ring[(i + 1) % 4][1] - ring[(i + 1) % 4][0] * ring[i][1] for i in range(4)]
    a2 = ((t[0] + t[1]) + t[2]) + t[3]
    if not (a2 > 0 or a2 < 0):                                     # zero or unordered
        return np.zeros(len(ex), dtype=bool)
    o = 1.0 if a2 > 0 else -1.0
    keep = np.ones(len(ex), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(4):
            (x0, y0), (x1, y1) = ring[i], ring[(i + 1) % 4]
            dx, dy = x1 - x0, y1 - y0
            c = o * (dx * (ey - y0) - dy * (ex - x0))
            keep &= (c >= 0) & (c * c >= (margin * margin) * (dx * dx + dy * dy))
    return keep


def occupants(cfg, cal, result, xyz, rule=RULE):
    """-> uint8 [W H]: k + 1 on an occupant of surface k of `result` (anything with n_steps, status, steps[k].height / .quad), 0 elsewhere"""
    margin, lo, hi = rule
    ok, wx, wy, wz = world(cfg, cal, xyz)
    out = np.zeros(len(ok), dtype=np.uint8)
    n = int(result.n_steps)
    if (int(result.status) & 1) or n == 0:
        return out
    r2, t2 = [float(v) for v in cal.r2], [float(v) for v in cal.t2]
    with np.errstate(invalid="ignore", over="ignore"):
        ex = (r2[0] * wx + r2[1] * wy) + t2[0]
        ey = (r2[2] * wx + r2[3] * wy) + t2[1]
        ez = wz + float(cal.world_z)
        heights = [float(result.steps[k].height) for k in range(n)]
        for h in heights:
            ok = ok & (np.abs(ez - h) > lo)
        for k in reversed(range(n)):                               # the lowest index wins: written last
            quad = [float(v) for v in result.steps[k].quad]
            take = ok & (ez > heights[k] + lo) & (ez < heights[k] + hi) & inside_shrunk(quad, margin, ex, ey)
            out[take] = k + 1
    return out


def sums(xyz, mask, n_surfaces):
    """the eleven sums per surface over the points of `mask` (k + 1 = surface k): [[n, sx, sy, sz, xx, xy, xz, yy, yz, zz, n_far]] as
    Python ints"""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    m = np.asarray(mask).reshape(-1)
    out = []
    for k in range(n_surfaces):
        q = np.rint(p[m == k + 1] * 65536.0)
        near = np.all(np.abs(q) < 2 ** 20, axis=1)
        n, s, ss = ground_model.moments_of_q(q[near].astype(np.int64))
        out.append([n] + s + ss + [int(np.count_nonzero(~near))])
    return out


def sums_of_record(rec, n_surfaces=None):
    """a FrameMoments in the form of sums()"""
    n = rec.n_surfaces if n_surfaces is None else n_surfaces
    return [[int(rec.s[k].m.n)] + [int(v) for v in rec.s[k].m.s] + [int(v) for v in rec.s[k].m.ss] + [int(rec.s[k].n_far)] for k in range(n)]


def hand_result(ssd, steps, status=0, n_steps=None):
    """a FrameResult of hand-made steps [(height, quad[8])]"""
    r = ssd.FrameResult()
    r.n_steps = len(steps) if n_steps is None else n_steps
    r.status = status
    for k, (h, quad) in enumerate(steps):
        r.steps[k].height = h
        r.steps[k].quad[:] = list(quad)
    return r


def result_of_oracle(ssd, res):
    """the oracle's record as the FrameResult a handle reports (steps_ext: height, then the quadrilateral)"""
    return hand_result(ssd, [(res.steps_ext[k][0], list(res.steps_ext[k][1:9])) for k in range(min(res.n_steps, ssd.MAX_STEPS))],
                       status=res.status, n_steps=res.n_steps)


def rule_of(ssd, rule):
    return ssd.ClearanceRule(*rule)


# ---- the frames ----

def patched(cfg, cal, result, xyz, labels, surface, n=300, pull=0.10):
    """a copy of the frame with n of the surface's labelled points pulled `pull` of the way towards the camera: a box on the tread.  The
    points are those whose PULLED position lies nearest the centre of the surface's quadrilateral in `result`, so the box stands at the
    tread's centre -> (frame, boolean [H, W] of the pulled pixels)"""
    f = np.array(xyz, dtype=np.float32, copy=True)
    flat = f.reshape(-1, 3)
    pulled = (flat.astype(np.float64) * (1.0 - pull)).astype(np.float32)
    _, wx, wy, _ = world(cfg, cal, pulled)
    r2, t2 = [float(v) for v in cal.r2], [float(v) for v in cal.t2]
    ex, ey = (r2[0] * wx + r2[1] * wy) + t2[0], (r2[2] * wx + r2[3] * wy) + t2[1]
    quad = np.array([float(v) for v in result.steps[surface].quad]).reshape(4, 2)
    d2 = (ex - quad[:, 0].mean()) ** 2 + (ey - quad[:, 1].mean()) ** 2
    d2[(np.asarray(labels).reshape(-1) != surface + 1) | ~(flat[:, 2] > 0)] = np.inf
    idx = np.argsort(d2, kind="stable")[:n]
    idx = idx[np.isfinite(d2[idx])]
    sel = np.zeros(len(flat), dtype=bool)
    sel[idx] = True
    flat[sel] = pulled[sel]
    return f, sel.reshape(f.shape[0], f.shape[1])


# the raised points of the full-width frames: (class, x range, y range) in world metres.  Class 0 is the ground (its rectangle is
# -0.3 .. 0.3 x 0.12 .. 0.22: the box lies 3 cm and more inside it).  Class 16 is the top step, 1.075 .. 1.225 in y; the steps below
# reach 1.115 (row 14) and 1.17 (row 15), so with the margin of 0.03 the lowest surface that holds a raised point is row 15 for
# y in 1.085 .. 1.14 and row 16 for y in 1.14 .. 1.195: the box spans 0.05 m of each, and a top-down pixel is 2.5 mm
RAISED_BOXES = ((0, (-0.2, 0.2), (0.155, 0.185)), (16, (-0.15, 0.15), (1.09, 1.19)))


def raised(ref, boxes=RAISED_BOXES, n=300, by=0.025, seed=5):
    """a copy of a full-width frame (full_width.Reference) with n points of each box's class inside the box raised by `by` metres (the
    camera looks along +z from below the world: raising is towards larger z).  The n are drawn by a fixed permutation of the candidates
    in (y, x) order, so every layout of the frame raises the same points -> (frame, boolean [W H] of the raised pixels)"""
    f = np.array(ref.xyz, dtype=np.float32, copy=True).reshape(-1, 3)
    sel = np.zeros(len(f), dtype=bool)
    for c, (x0, x1), (y0, y1) in boxes:
        idx = np.flatnonzero((ref.classes == c) & (f[:, 0] > x0) & (f[:, 0] < x1) & (f[:, 1] > y0) & (f[:, 1] < y1))
        idx = idx[np.lexsort((f[idx, 0], f[idx, 1]))]
        assert len(idx) >= n, (c, len(idx))
        sel[idx[np.random.default_rng(seed + c).permutation(len(idx))[:n]]] = True
    f[sel, 2] += np.float32(by)
    return f.reshape(ref.xyz.shape), sel


@functools.lru_cache(maxsize=None)
def scene_frame(ssd, sigma=0.001, seed=7):
    """ground_model's 256 x 192 3-step scene -> (cfg, trans, frame)"""
    sc = ground_model.scene(ssd, "steps", sigma=sigma, seed=seed)
    frame = ssd.synth_host([sc])[0]
    frame.setflags(write=False)
    return ssd.default_config(W, H), ssd.transformation_for_scene(sc), frame


# ---- the accuracy figures (tools/clearance_accuracy.py writes them, tests/test_clearance.py holds the host functions to them) ----
ACCURACY_FILE = os.path.join(ground_model.ROOT, "profiles", "clearance_accuracy.txt")
ACCURACY_SIGMAS, ACCURACY_SEEDS = (0.001, 0.003), (7, 11, 13, 17, 19)


def accuracy(ssd, oracle, sigmas=ACCURACY_SIGMAS, seeds=ACCURACY_SEEDS, rows=None):
    """The 3-step scene under the oracle and the default rule, through ssd_clearance_host and ssd_clearance_solve: occupants of the clean
    frames, the share of a 300-point patch found on its tread (tread 1, the top tread), and the solved centroid's distance from the mean
    of the patch's own points -> the worst of each; rows (a list): a line per case"""
    import oracle_binding as ob
    from test_labels import expected_labels
    out = dict(false_occupants_clean=0, worst_share_tread1=1.0, worst_share_top=1.0, worst_centroid_distance_m=0.0)
    rule = rule_of(ssd, RULE)
    for sigma in sigmas:
        for seed in seeds:
            cfg, trans, frame = scene_frame(ssd, sigma, seed)
            cal = trans.constants
            ocfg, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal)
            res = oracle.process(ocfg, ocal, frame)[0]
            fr = result_of_oracle(ssd, res)
            rec, _ = ssd.clearance_host(cfg, cal, frame, fr, 1, rule, mask=False)
            clean = sum(int(rec.s[k].m.n + rec.s[k].n_far) for k in range(fr.n_steps))
            out["false_occupants_clean"] += clean
            labels = expected_labels(oracle, cfg, cal, res, frame)
            line = "sigma %g mm seed %2d: clean %d" % (sigma * 1e3, seed, clean)
            for surface, key in ((1, "tread1"), (fr.n_steps - 1, "top")):
                f2, sel = patched(cfg, cal, fr, frame, labels, surface)
                fr2 = result_of_oracle(ssd, oracle.process(ocfg, ocal, f2)[0])
                rec, mask = ssd.clearance_host(cfg, cal, f2, fr2, 1, rule)
                share = np.count_nonzero(mask[sel] == surface + 1) / max(np.count_nonzero(sel), 1)
                sol = ssd.clearance_solve(rec, fr2, cal).s[surface]
                _, wx, wy, wz = world(cfg, cal, f2[sel])
                r2, t2 = [float(v) for v in cal.r2], [float(v) for v in cal.t2]
                own = np.array([np.mean((r2[0] * wx + r2[1] * wy) + t2[0]), np.mean((r2[2] * wx + r2[3] * wy) + t2[1]), np.mean(wz + cal.world_z)])
                dist = float(np.linalg.norm(np.array(list(sol.centroid)) - own)) if sol.status else float("inf")
                out["worst_share_" + key] = min(out["worst_share_" + key], share)
                out["worst_centroid_distance_m"] = max(out["worst_centroid_distance_m"], dist)
                line += " | %s: %d of %d (%.4f), height %.4f m, centroid off %.5f m" % (key, int(round(share * np.count_nonzero(sel))), np.count_nonzero(sel), share, sol.height_mean, dist)
            if rows is not None:
                rows.append(line)
    return out


def recorded_accuracy():
    """the `key = value` lines of profiles/clearance_accuracy.txt"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out
