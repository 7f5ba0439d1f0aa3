"""The trimmed surface refit restated for the tests (include/ssd_hip.h), independent of the C code: the gate rule
in numpy doubles and the refit moments in Python / int64 integers, the gates from numpy.linalg.eigh, the gate-edge clouds the CPU and
the GPU tests share, and the chain first fit -> gates -> refit on the host functions that the accuracy figures come from
(profiles/surface_refit_accuracy.txt, written by tools/surface_refit_accuracy.py).  TEST INFRASTRUCTURE; no GPU needed."""
import math
import os

import numpy as np

import ground_model as gm
import surface_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_SIGMAS = (2.5, 2.0)
PASSES = 2


def gate_rows(gates):
    """FrameGates -> (n_surfaces, [(n [3], dist, gate)] for all SSD_MAX_STEPS gates) as Python floats"""
    return int(gates.n_surfaces), [([float(v) for v in g.n], float(g.dist), float(g.gate)) for g in gates.g]


def keeps(pts, labels, gates):
    """bool [N]: the labelled points inside their surface's gate.  The residual in doubles of the float32 coordinates, products first,
    the row sum left to right, then the distance: numpy's elementwise double arithmetic rounds each operation once, as the rule says."""
    p = np.ascontiguousarray(pts, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    lab = np.asarray(labels).reshape(-1)
    n_surfaces, rows = gate_rows(gates)
    keep = np.zeros(len(lab), dtype=bool)
    for k, (n, dist, gate) in enumerate(rows[:max(0, n_surfaces)]):
        if not (gate > 0.0 and math.isfinite(gate)):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            r = ((n[0] * p[:, 0] + n[1] * p[:, 1]) + n[2] * p[:, 2]) - dist
            keep |= (lab == k + 1) & (np.abs(r) <= gate)
    return keep


def refit_np(pts, labels, gates, n_surfaces):
    """[(n, s, ss, n_far)] per surface: the surface fit's sums (tests/surface_model.moments_np) over the kept points alone"""
    lab = np.where(keeps(pts, labels, gates), np.asarray(labels).reshape(-1), 0)
    return sm.moments_np(pts, lab, n_surfaces)


def refit_py(pts, labels, gates, n_surfaces):
    """the same in Python integers (small clouds)"""
    lab = np.where(keeps(pts, labels, gates), np.asarray(labels).reshape(-1), 0)
    return sm.moments_py(pts, lab, n_surfaces)


def make_gates(ssd, planes):
    """FrameGates of [(n [3], dist, gate)]"""
    g = ssd.FrameGates()
    g.n_surfaces = len(planes)
    for k, (n, dist, gate) in enumerate(planes):
        g.g[k].n[:] = [float(v) for v in n]
        g.g[k].dist, g.g[k].gate = float(dist), float(gate)
    return g


def gates_eigh(fm, min_points, k_sigma, gate_min):
    """numpy's word on ssd_surface_gates_from_moments for the surfaces whose fit is OK: {k: (n0, dist, gate)}; a surface with fewer than
    min_points points, or whose scatter fails the planarity rule, is left out (the caller knows which it built that way)"""
    out = {}
    for k in range(fm.n_surfaces):
        n, s, ss = gm.moments_tuple(fm.s[k].m)
        if n < max(min_points, 1):
            continue
        lam, n0, dist = gm.eigh_of(n, s, ss)
        if not (lam[1] > 0 and lam[1] >= 16.0 * max(lam[0], 0.0)):
            continue
        out[k] = (n0, dist, max(k_sigma * math.sqrt(max(lam[0], 0.0)), gate_min))
    return out


# ---- gate-edge clouds: every value dyadic, so that every product and sum below is exact and the edge is hit exactly ------------------
F = np.float32


def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


def edge_cloud_axis(centre=(0.0, 0.0, 1.5)):
    """A plane n = (0, 0, 1), dist = centre z, gate 2^-7, and points at dist +- gate (kept), one float ulp beyond on either side (trimmed),
    and a few well inside: -> (plane, points float32 [N, 3], kept bool [N]).  x, y scatter on a dyadic grid around the centre."""
    cx, cy, cz = centre
    gate = 2.0 ** -7
    pts, kept = [], []
    for i, (dx, dy) in enumerate([(-0.125, -0.0625), (0.125, 0.0625), (0.0, 0.03125), (0.0625, -0.03125)]):
        for z, k in ((F(cz + gate), True), (up(cz + gate), False), (F(cz - gate), True), (down(cz - gate), False), (F(cz + gate / 4 * i), True)):
            pts.append((cx + dx, cy + dy, z))
            kept.append(k)
    return ((0.0, 0.0, 1.0), cz, gate), np.array(pts, dtype=np.float32), np.array(kept)


def edge_cloud_tilted():
    """A dyadic tilted normal n = (2^-54, 1, -1) (not unit: the rule does not ask) and a point (1, 1 + 2^-10, 1) built so that
    (a + b) + c and a + (b + c) differ in the last bit: a = 2^-54 x is a quarter of an ulp of b = y in doubles, so a + b rounds a away,
    while b + c = y - z is small and exact and keeps it.  With dist = 0 and gate = y - z exactly, the stated order (a + b) + c gives a
    residual EQUAL to the gate (kept); the other order gives gate + 2^-54 (trimmed).  The same point one float ulp further in y is
    beyond the gate under either order; so on the other side.  -> (plane, points, kept, residuals under the other order)"""
    n = (2.0 ** -54, 1.0, -1.0)
    x, y, z = 1.0, 1.0 + 2.0 ** -10, 1.0
    gate = 2.0 ** -10
    a, b, c = n[0] * x, n[1] * y, n[2] * z
    assert (a + b) + c == gate and a + (b + c) == gate + 2.0 ** -54 and (a + b) + c != a + (b + c)
    y2 = float(up(y))                                       # one float ulp further: beyond the gate under either order
    pts = np.array([(x, y, z), (x, y2, z), (x, 1.0, 1.0 + 2.0 ** -10), (x, 1.0, float(up(1.0 + 2.0 ** -10)))], dtype=np.float32)
    # third point: a + b = 1 (a rounded away), + c = -(2^-10): |r| == gate, kept; under the other order |r| = 2^-10 - 2^-54: kept either way
    kept = np.array([True, False, True, False])
    p = pts.astype(np.float64)
    other = n[0] * p[:, 0] + (n[1] * p[:, 1] + n[2] * p[:, 2])
    return (n, 0.0, gate), pts, kept, other


# ---- the chain on the host functions -------------------------------------------------------------------------------------------------
def refit_chain(ssd, cfg, frame, labels, fm, k_sigma, gate_min=0.0, passes=PASSES, min_points=sm.MIN_POINTS, intr=None):
    """[FrameMoments of pass 1, 2, ..]: each pass gated by the planes of the one before, starting from the first fit's moments fm"""
    out, cur = [], fm
    for _ in range(passes):
        gates = ssd.surface_gates_from_moments(cur, min_points, k_sigma, gate_min)
        cur = ssd.surface_refit_moments_host(cfg, frame, labels, gates, fm.n_surfaces, fm.ground, intr=intr)
        out.append(cur)
    return out


def accuracy_rows(ssd, oracle, k_sigmas=K_SIGMAS, passes=PASSES):
    """The cases of tests/surface_model.accuracy_cases through the host functions on the oracle's labels: per case
    (name, want, [per surface: {'first': (err, rms, n), (k_sigma, pass): (err, rms, kept)}])"""
    out = []
    for name, cfg, frame, truth, cal in sm.accuracy_cases(ssd):
        want = gm.angle(gm.plane_of(truth)[0], gm.plane_of(cal)[0])
        res, labels, fm, fit = sm.oracle_planes(ssd, oracle, cfg, cal, frame)
        rows = [{"first": (abs(fit.s[k].tilt - want), fit.s[k].rms, int(fit.s[k].n), fit.s[k].status)} for k in range(fit.n_surfaces)]
        for ks in k_sigmas:
            for p, rm in enumerate(refit_chain(ssd, cfg, frame, labels, fm, ks, passes=passes)):
                f = ssd.surface_fit_solve(rm, cal, sm.MIN_POINTS)
                for k in range(f.n_surfaces):
                    rows[k][(ks, p + 1)] = (abs(f.s[k].tilt - want), f.s[k].rms, int(f.s[k].n + f.s[k].n_far), f.s[k].status)
        out.append((name, want, rows))
    return out


def worst_columns(cases, k_sigmas=K_SIGMAS, passes=PASSES):
    """{'first': worst tilt error, (k_sigma, pass): worst tilt error} and the smallest kept share per column"""
    cols = ["first"] + [(ks, p + 1) for ks in k_sigmas for p in range(passes)]
    worst = {c: max(r[c][0] for _, _, rows in cases for r in rows) for c in cols}
    share = {c: min(r[c][2] / r["first"][2] for _, _, rows in cases for r in rows) for c in cols if c != "first"}
    return worst, share


def column_key(c):
    return "first" if c == "first" else "k%s_pass%d" % (("%g" % c[0]).replace(".", "p"), c[1])


ACCURACY_FILE = os.path.join(ROOT, "profiles", "surface_refit_accuracy.txt")


def recorded_accuracy():
    """{'worst_tilt_error_rad_first', 'worst_tilt_error_rad_k2p5_pass1', ..} from profiles/surface_refit_accuracy.txt"""
    out = {}
    for line in open(ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            out[k.strip()] = float(v.split()[0])
    return out


def order_sensitive_points(pts, labels, k, per_kind=4):
    """Puts the order-sensitive construction of edge_cloud_tilted on surface k's own points (pts float32 [N, 3], changed in place; labels
    [N]): a plane n = (2^-58, 1, -j / 1024), dist 0, gate 2^-10, with j / 1024 the tread's median y / z, and - among the labelled
    points with x >= 1/8 and |y| >= 1/4 whose y / z is nearest to it - per_kind points moved by about a millimetre onto
    z' = z to 2^-12, y' = (j / 1024) z' + 2^-10 (every product and sum exact).  There a = n0 x is far below half an ulp of b = y', so
    the stated order gives (a + b) + c = 2^-10 = the gate exactly (kept), while a + (b + c) = 2^-10 + a lies beyond it (trimmed).
    Another per_kind points get y' one float ulp further: trimmed under either order.  -> (plane, indices on the edge, indices beyond)"""
    gate, n0 = 2.0 ** -10, 2.0 ** -58
    p = pts.astype(np.float64)
    mine = np.flatnonzero((np.asarray(labels).reshape(-1) == k + 1) & (p[:, 0] >= 0.125) & (np.abs(p[:, 1]) >= 0.25) & (p[:, 2] > 0.5))
    assert len(mine) >= 8 * per_kind, "the surface has points to choose from"
    j = int(np.rint(np.median(p[mine, 1] / p[mine, 2]) * 1024))
    n2 = -j / 1024.0
    near = mine[np.argsort(np.abs(p[mine, 1] + n2 * p[mine, 2] - gate))][:2 * per_kind]
    on, beyond = [int(i) for i in near[:per_kind]], [int(i) for i in near[per_kind:]]
    for idx, further in ((on, False), (beyond, True)):
        for i in idx:
            z = np.rint(p[i, 2] * 4096) / 4096
            y = -n2 * z + gate
            assert float(np.float32(y)) == y and float(np.float32(z)) == z, "the moved point is a float"
            pts[i, 2] = np.float32(z)
            pts[i, 1] = np.nextafter(np.float32(y), np.float32(np.inf)) if further else np.float32(y)
    q = pts[on].astype(np.float64)
    a, b, c = n0 * q[:, 0], q[:, 1], n2 * q[:, 2]
    assert np.all((a + b) + c == gate) and np.all(a + (b + c) > gate), "on the edge under the stated order, beyond it under the other"
    q = pts[beyond].astype(np.float64)
    assert np.all((n0 * q[:, 0] + q[:, 1]) + n2 * q[:, 2] > gate)
    return ((n0, 1.0, n2), 0.0, gate), on, beyond
