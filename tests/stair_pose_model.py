"""The stair pose's rule restated for the tests (include/ssd_hip.h) in numpy: which points of a frame lie on which
tread and which riser of a stair MAP under a prior calibration, their exact integer moments, the fold in Python integers, and the small
helpers the CPU and the GPU tests share (targets, priors moved by a known rigid motion, records as tuples).
TEST INFRASTRUCTURE; no GPU needed.  Written from the rule's text, vectorised over the points: it shares no structure with the C text."""
import math
import os

import numpy as np

import ground_model

TREADS, RISERS, SUMS = 17, 16, 11
RULE = (0.03, 0.03, 0.03, 0.04)               # margin, band, clear, reach: the defaults (SSD_SP_*)
INT64_MAX, INT64_MIN = (1 << 63) - 1, -(1 << 63)


def external(cfg, cal, xyz):
    """float32 camera points -> (valid-and-in-range mask, ex, ey, ez) in doubles: w = A p + b, each row (a0 x + a1 y) + a2 z, then + b;
    in range: strictly inside the x and y measuring range; (ex, ey) = r2 w_xy + t2, row sums left to right; ez = w.z + world_z"""
    p32 = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    p = p32.astype(np.float64)
    a, b = [float(v) for v in cal.a], [float(v) for v in cal.b]
    r2, t2 = [float(v) for v in cal.r2], [float(v) for v in cal.t2]
    with np.errstate(invalid="ignore", over="ignore"):
        w = [((a[3 * r] * p[:, 0] + a[3 * r + 1] * p[:, 1]) + a[3 * r + 2] * p[:, 2]) + b[r] for r in range(3)]
        ok = (p32[:, 2] > 0) & (w[0] > cfg.x_min) & (w[0] < cfg.x_max) & (w[1] > cfg.y_min) & (w[1] < cfg.y_max)
        ex = (r2[0] * w[0] + r2[1] * w[1]) + t2[0]
        ey = (r2[2] * w[0] + r2[3] * w[1]) + t2[1]
        ez = w[2] + float(cal.world_z)
    return ok, ex, ey, ez


def in_tread(quad, margin, ex, ey):
    """inside the quadrilateral (FL, FR, BL, BR as x, y pairs) shrunk by margin: the ring FL, FR, BR, BL, its orientation o from twice the
    signed area ((t0 + t1) + t2) + t3, and per side c = o (dx (ey - y_i) - dy (ex - x_i)) with c >= 0 and c c >= margin^2 (dx^2 + dy^2)"""
    ring = [(quad[0], quad[1]), (quad[2], quad[3]), (quad[6], quad[7]), (quad[4], quad[5])]
    t = [ring[i][0] * ring[(i + 1) % 4][1] - ring[(i + 1) % 4][0] * ring[i][1] for i in range(4)]
    a2 = ((t[0] + t[1]) + t[2]) + t[3]
    if not (a2 > 0 or a2 < 0):
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


def at_riser(quad_up, reach, ex, ey):
    """within reach of the vertical plane under the front edge FL -> FR of the step above, between the edge's ends"""
    flx, fly = quad_up[0], quad_up[1]
    dx, dy = quad_up[2] - flx, quad_up[3] - fly
    l2 = dx * dx + dy * dy
    if not l2 > 0:
        return np.zeros(len(ex), dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b = ex - flx, ey - fly
        c = b * dx - a * dy
        t = a * dx + b * dy
        return (c * c <= (reach * reach) * l2) & (t >= 0) & (t <= l2)


def classes(cfg, cal, stairs, xyz, rule=RULE):
    """-> int [W H]: k on a point of tread k, 17 + i on a point of riser i, -1 elsewhere (stairs: anything with n_steps, status, steps)"""
    margin, band, clear, reach = rule
    ok, ex, ey, ez = external(cfg, cal, xyz)
    out = np.full(len(ok), -1, dtype=np.int64)
    n = int(stairs.n_steps)
    if (int(stairs.status) & 1) or n == 0:
        return out
    h = [float(stairs.steps[k].height) for k in range(n)]
    quads = [[float(v) for v in stairs.steps[k].quad] for k in range(n)]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in reversed(range(n - 1)):                           # the lowest index wins: written last; a tread beats every riser
            out[ok & (ez > h[i] + clear) & (ez < h[i + 1] - clear) & at_riser(quads[i + 1], reach, ex, ey)] = TREADS + i
        for k in reversed(range(n)):
            out[ok & ~(np.abs(ez - h[k]) > band) & in_tread(quads[k], margin, ex, ey)] = k
    return out


def record_np(cfg, cal, stair_map, xyz, rule=RULE):
    """the frame's record as the model has it: (headers (treads.n_surfaces, treads.ground, risers.n_surfaces, risers.ground),
    [17 treads' eleven sums], [17 riser slots' eleven sums]) in Python ints"""
    st = stair_map.stairs
    n = int(st.n_steps)
    zero = [[0] * SUMS for _ in range(TREADS)]
    if (int(st.status) & 1) or n == 0:
        return (0, 0, 0, 0), zero, [list(r) for r in zero]
    cls = classes(cfg, cal, st, xyz, rule)
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3).astype(np.float64)

    def sums(c):
        q = np.rint(p[cls == c] * 65536.0)
        near = np.all(np.abs(q) < 2 ** 20, axis=1)
        cnt, s, ss = ground_model.moments_of_q(q[near].astype(np.int64))
        return [cnt] + s + ss + [int(np.count_nonzero(~near))]
    treads = [sums(k) if k < n else [0] * SUMS for k in range(TREADS)]
    risers = [sums(TREADS + i) if i < n - 1 else [0] * SUMS for i in range(TREADS)]
    return (n, 1 if stair_map.ground != 0 else 0, max(n - 1, 0), 0), treads, risers


def record_tuple(rec):
    """a StairPoseMoments in the form of record_np()"""
    def half(fm):
        return [[int(fm.s[k].m.n)] + [int(v) for v in fm.s[k].m.s] + [int(v) for v in fm.s[k].m.ss] + [int(fm.s[k].n_far)] for k in range(TREADS)]
    return (int(rec.treads.n_surfaces), int(rec.treads.ground), int(rec.risers.n_surfaces), int(rec.risers.ground)), half(rec.treads), half(rec.risers)


def record_of(ssd, headers, treads, risers):
    """a StairPoseMoments from the form of record_np() (rows may be fewer than 17)"""
    rec = ssd.StairPoseMoments()
    rec.treads.n_surfaces, rec.treads.ground, rec.risers.n_surfaces, rec.risers.ground = headers
    for fm, rows in ((rec.treads, treads), (rec.risers, risers)):
        for k, row in enumerate(rows):
            fm.s[k].m.n = row[0]
            fm.s[k].m.s[:] = row[1:4]
            fm.s[k].m.ss[:] = row[4:10]
            fm.s[k].n_far = row[10]
    return rec


def fold_py(records):
    """the fold in Python integers over record_np() forms: the last headers, every sum added -> the same form, or None where a sum
    leaves int64"""
    headers, treads, risers = (0, 0, 0, 0), [[0] * SUMS for _ in range(TREADS)], [[0] * SUMS for _ in range(TREADS)]
    for hd, tr, ri in records:
        headers = hd
        treads = [[a + b for a, b in zip(x, y)] for x, y in zip(treads, tr)]
        risers = [[a + b for a, b in zip(x, y)] for x, y in zip(risers, ri)]
        if any(v > INT64_MAX or v < INT64_MIN for rows in (treads, risers) for r in rows for v in r):
            return None
    return headers, treads, risers


def target(ssd, cal, stair_map, intr=None):
    return ssd.stair_pose_target((cal, intr) if intr is not None else cal, stair_map)


def rule_of(ssd, rule=RULE):
    return ssd.StairPoseRule(*rule)


# ---- rigid motions of a calibration, in the external world (for the priors of the solve's tests and of the recorded recipe) ----

def rot(w):
    """Rot(w): the rotation by |w| radians about w (Rodrigues)"""
    w = np.asarray(w, dtype=np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + math.sin(th) / th * K + (1.0 - math.cos(th)) / (th * th) * (K @ K)


def affine_of(cal):
    """a calibration as e = T p + c, camera -> external world"""
    A = np.array([float(v) for v in cal.a]).reshape(3, 3)
    b = np.array([float(v) for v in cal.b])
    r2 = np.array([float(v) for v in cal.r2]).reshape(2, 2)
    M = np.eye(3)
    M[:2, :2] = r2
    T = M @ A
    c = M @ b + np.array([float(cal.t2[0]), float(cal.t2[1]), float(cal.world_z)])
    return T, c


def cal_of_affine(ssd, T, c, world_z):
    """the calibration whose affine map is e = T p + c (T a rotation): the floor plane n0 = -row 3 of T at dist = c_z - world_z gives
    a, b; r2 = T[0:2] a[0:2]^T; t2 = c_xy - by the library's host function for the plane, numpy for the rest"""
    base = ssd.GeometricTransformation().constants
    base.world_z = world_z
    cal = ssd.calibration_from_plane([-T[2, 0], -T[2, 1], -T[2, 2]], c[2] - world_z, base)
    A = np.array([float(v) for v in cal.a]).reshape(3, 3)
    r2 = T[:2] @ A[:2].T
    for i in range(4):
        cal.r2[i] = float(r2.ravel()[i])
    cal.t2[0], cal.t2[1] = float(c[0]), float(c[1])
    return cal


def moved(ssd, cal, w, tau, centre=(0.0, 0.0, 0.0)):
    """the calibration that maps a camera point to Rot(w)(e - centre) + centre + tau, e where `cal` maps it"""
    T, c = affine_of(cal)
    R = rot(w)
    ctr = np.asarray(centre, dtype=np.float64)
    return cal_of_affine(ssd, R @ T, R @ (c - ctr) + ctr + np.asarray(tau, dtype=np.float64), float(cal.world_z))


def pose_between(cal_a, cal_b):
    """the rigid motion that takes cal_a's external points to cal_b's: (rotation vector, translation at the origin)"""
    Ta, ca = affine_of(cal_a)
    Tb, cb = affine_of(cal_b)
    R = Tb @ Ta.T
    ang = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0)))
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    w = axis / (2.0 * math.sin(ang)) * ang if ang > 1e-12 else axis / 2.0
    return w, cb - R @ ca


# ---- the recorded recipe (profiles/stair_pose_accuracy.txt, written by tools/stair_pose_accuracy.py) ----

MIN_POINTS = 200
PASSES = 3
ROUNDING = 64.0 * 2.220446049250313e-16       # the solve's rounding level, as a ratio to lambda_max
DEG = math.pi / 180.0
# how a prior differs from the true pose: (rotation vector, translation) in the external world about the staircase's centre - x runs
# along the edges, y along the going, z up
OFFSETS = [("yaw 2 deg", (0.0, 0.0, 2.0 * DEG), (0.0, 0.0, 0.0)), ("going 3 cm", (0.0, 0.0, 0.0), (0.0, 0.03, 0.0)),
           ("pitch 1 deg", (1.0 * DEG, 0.0, 0.0), (0.0, 0.0, 0.0)), ("height 2 cm", (0.0, 0.0, 0.0), (0.0, 0.0, 0.02)),
           ("all together", (1.0 * DEG, 0.0, 2.0 * DEG), (0.0, 0.03, 0.02))]
COMPONENTS = ("pitch rad", "roll rad", "yaw rad", "going m", "height m")     # what a straight staircase observes


def recipe_scene(ssd, oracle):
    """the 3-step scene at 256 x 192 under camera_drift_model.FRAMES' seeds and noises -> (cfg, frames, the true calibration, the
    median map of the oracle's results under it)"""
    import camera_drift_model as cd
    import clearance_model as cm
    import oracle_binding as ob
    cfg = ssd.default_config(ground_model.W, ground_model.H)
    frames, truth = [], None
    for seed, sigma in cd.FRAMES:
        sc = ground_model.scene(ssd, "steps", seed=seed, sigma=sigma)
        if truth is None:
            truth = ssd.transformation_for_scene(sc).constants
        frames.append(ssd.synth_host([sc])[0])
    res = [cm.result_of_oracle(ssd, oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(truth), f)[0]) for f in frames]
    stair_map, used = ssd.stair_map_from_results(res)
    assert used == len(frames) and stair_map.stairs.n_steps == 3
    return cfg, frames, truth, stair_map


def chain_host(ssd, cfg, frames, prior, stair_map, passes=PASSES, rule=RULE, min_points=MIN_POINTS, observable=None):
    """Detector.locate_camera on the host functions: per pass the fold of every frame's record under the calibration so far, solved;
    OK passes chained -> (the calibration after each pass, each pass's StairPose)"""
    cal, cals, poses = prior, [], []
    for _ in range(passes):
        t = target(ssd, cal, stair_map)
        acc = ssd.StairPoseMoments()
        for f in frames:
            ssd.stair_pose_add(ssd.stair_pose_host(cfg, t, f, rule_of(ssd, rule)), acc)
        pose = ssd.stair_pose_solve(acc, t, min_points, ssd.SP_OBSERVABLE if observable is None else observable)
        poses.append(pose)
        if pose.status != ssd.GF_OK:
            break
        cal = pose.cal
        cals.append(cal)
    return cals, poses


def components(cal_ref, cal, centre):
    """how far `cal` is from `cal_ref`, as the rigid motion between their external worlds: (pitch, roll, yaw in radians, the centre's
    displacement along the going and in height in metres) - the five components a straight staircase observes"""
    w, t = pose_between(cal_ref, cal)
    ctr = np.asarray(centre, dtype=np.float64)
    d = rot(w) @ ctr + t - ctr
    return [float(w[0]), float(w[1]), float(w[2]), float(d[1]), float(d[2])]


def recipe(ssd, oracle):
    """-> dict: 'bias' (the components of (a)'s pose against the true calibration), 'spectrum_true' (the scaled eigenvalue ratios of
    (a)'s first pass), 'cases' {name: {'begin': [5], 'after': [[5] per pass], 'spectra': [[6] per pass], 'dof': [..], 'n': [..]}},
    'unobserved_max', 'observed_min' (over every recorded spectrum)"""
    cfg, frames, truth, stair_map = recipe_scene(ssd, oracle)
    cals_a, poses_a = chain_host(ssd, cfg, frames, truth, stair_map)
    assert len(cals_a) == PASSES
    cal_a, centre = cals_a[-1], list(poses_a[0].centre)
    ratios = lambda p: [e / p.eig[5] for e in p.eig]
    out = dict(bias=components(truth, cal_a, centre), first_pass=components(truth, cals_a[0], centre), spectrum_true=ratios(poses_a[0]),
               rms=(poses_a[0].rms_before, poses_a[-1].rms_after), n=int(poses_a[0].n), centre=centre, cases={})
    spectra = [ratios(p) for p in poses_a]
    for name, w, tau in OFFSETS:
        prior = moved(ssd, truth, w, tau, centre)
        cals, poses = chain_host(ssd, cfg, frames, prior, stair_map)
        out["cases"][name] = dict(begin=components(cal_a, prior, centre), after=[components(cal_a, c, centre) for c in cals],
                                  spectra=[ratios(p) for p in poses], dof=[int(p.dof) for p in poses], n=[int(p.n) for p in poses],
                                  status=[int(p.status) for p in poses])
        spectra += out["cases"][name]["spectra"]
    out["unobserved_max"] = max(s[0] for s in spectra)
    out["observed_min"] = min(s[1] for s in spectra)
    return out


ACCURACY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stair_pose_accuracy.txt")


def recorded_accuracy():
    """the `key = value` lines of profiles/stair_pose_accuracy.txt as floats"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out
