"""The tread grid on the host (include/ssd_hip.h): the exports and sizes, every refusal of the host functions,
ssd_tread_grid_host against the numpy restatement of tests/tread_grid_model.py cell by cell, the rule's edges on hand-made results with
lattice quadrilaterals (sides multiples of (3, 4): exact lengths; cell 0.25: exact divisions), the occupant identity against
ssd_clearance_host, ssd_tread_grid_solve against the model's brute force, and the recipe under the oracle - judged here, on the host
functions, because the device is held to them byte for byte (tests/test_gpu_tread_grid.py).  No GPU needed."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import clearance_model as cm
import full_width as fw
import ground_model as gm
import oracle_binding as ob
import tread_grid_model as tg
from test_labels import expected_labels

NAMES = ["ssd_enqueue_tread_grid", "ssd_enqueue_cameras_tread_grid", "ssd_fetch_tread_grid", "ssd_get_tread_grid_time", "ssd_tread_grid_host",
         "ssd_tread_grid_solve", "ssd_process_host_tread_grid", "ssd_process_host_cameras_tread_grid"]


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_tread_grid", "enqueue_cameras_tread_grid", "fetch_tread_grid", "tread_grid_time_ms", "process_host_tread_grid",
              "process_host_cameras_tread_grid"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.tread_grid_host) and callable(ssd.tread_grid_solve)
    assert (ssd.TG_COLS, ssd.TG_ROWS) == (tg.COLS, tg.ROWS) == (32, 8)
    assert (ssd.TG_OUT, ssd.TG_FREE, ssd.TG_OCCUPIED, ssd.TG_UNSEEN) == (tg.OUT, tg.FREE, tg.OCCUPIED, tg.UNSEEN) == (0, 1, 2, 3)
    assert C.sizeof(ssd.TreadGridRule) == 32 and C.sizeof(ssd.TreadGrid) == 3088 and C.sizeof(ssd.FrameTreadGrid) == 52504
    assert C.sizeof(ssd.Foothold) == 328 and C.sizeof(ssd.FrameFootholds) == 8 + ssd.MAX_STEPS * 328
    r = ssd.TreadGridRule()
    assert (r.clearance.margin, r.clearance.lo, r.clearance.hi) == (0.03, 0.03, 0.5) and 0.005 <= r.cell <= 1.0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssd_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in header
    assert "#define SSD_TG_COLS 32" in header and "#define SSD_TG_ROWS 8" in header


# ---- the hand-made world: camera = camera-dependent world = external world ------------------------------------------------------------
# The quadrilateral: front side 2 (3, 4) = 10 m long from FL = (0, 0), 2.5 m deep along (-0.8, 0.6).  With cell 0.25 the grid spans 8 m of
# the front edge and 2 m behind it, so the quadrilateral holds points beyond the grid on both axes.
E, N = (0.6, 0.8), (-0.8, 0.6)                          # unit vectors along the front edge and behind it
FL, FR, BR, BL = (0.0, 0.0), (6.0, 8.0), (4.0, 9.5), (-2.0, 1.5)
QUAD = [*FL, *FR, *BL, *BR]                             # ssd_step's order: front-left, front-right, back-left, back-right
MARGIN, LO, HI, HEIGHT, CELL = 5.0 / 128, 0.03125, 0.5, 0.5, 0.25
RULE = (MARGIN, LO, HI, CELL)
ON, ABOVE = HEIGHT, HEIGHT + 0.25                       # a tread point's and an occupant's z


def _identity(ssd, world_z=0.0):
    cal = ssd.Calibration()
    cal.a[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    cal.b[:] = [0, 0, 0]
    cal.r2[:] = [1, 0, 0, 1]
    cal.t2[:] = [0, 0]
    cal.world_z = world_z
    return cal


def _cfg(ssd, n):
    cfg = ssd.default_config(8, 4)
    cfg.width, cfg.height = n, 1
    cfg.x_min, cfg.x_max, cfg.y_min, cfg.y_max, cfg.z_min, cfg.z_max = -64.0, 64.0, -64.0, 64.0, 0.0, 8.0
    return cfg


def _at(u, v, z):
    """the point u along the front edge from FL and v behind it, in exact rational arithmetic.  Its coordinates are dyadic when 3 u - 4 v and 4 u + 3 v are multiples of 5 (in units of a power of two), which
    the tests' (u, v) are chosen for: u dx + v dy is then exact, and so is the division by L"""
    u, v = Fraction(u), Fraction(v)
    return (float(FL[0] + (3 * u - 4 * v) / 5), float(FL[1] + (4 * u + 3 * v) / 5), z)


def _lattice(u16, z):
    """(u, v) in sixteenths with v the smallest sixteenth >= 1 for which the point is dyadic: m = 3 n (mod 5)"""
    n = next(n for n in range(1, 6) if (u16 - 3 * n) % 5 == 0)
    return _at(u16 / 16.0, n / 16.0, z), n


def _grids(ssd, points, result, rule=RULE, cal=None):
    """ssd_tread_grid_host over hand-made points [(x, y, z)], checked against the model cell by cell and against ssd_clearance_host's
    n + n_far (the occupant identity) -> the record"""
    pts = np.array(points, dtype=np.float32).reshape(-1, 3)
    assert np.array_equal(pts.astype(np.float64), np.array(points, dtype=np.float64).reshape(-1, 3)), "the points are float32 values"
    cfg, cal = _cfg(ssd, len(pts)), cal or _identity(ssd)
    rec = ssd.tread_grid_host(cfg, cal, pts.reshape(1, -1, 3), result, 0, tg.rule_of(ssd, rule))
    n = 0 if (result.status & 1) else result.n_steps
    tg.assert_record(ssd, rec, tg.grids(cfg, cal, result, pts, rule), n, 0)
    _identity_holds(ssd, cfg, cal, pts.reshape(1, -1, 3), result, rule, rec)
    return rec


def _identity_holds(ssd, cfg, cal, frame, result, rule, rec, intr=None):
    """sum(occ) + n_occ_out of every surface = n + n_far of the clearance record for the same rule"""
    clear, _ = ssd.clearance_host(cfg, cal, frame, result, 0, cm.rule_of(ssd, rule[:3]), intr=intr, mask=False)
    for k in range(ssd.MAX_STEPS):
        g = tg.grid_of_record(rec, k)
        assert int(g["occ"].sum()) + g["n_occ_out"] == int(clear.s[k].m.n + clear.s[k].n_far), k


def _cells(rec, k, plane):
    """{(row, col): count} of the non-zero cells of a plane"""
    a = tg.grid_of_record(rec, k)[plane]
    return {(int(r), int(c)): int(a[r, c]) for r, c in zip(*np.nonzero(a))}


def test_cell_boundaries_and_the_grids_far_ends(ssd):
    res = cm.hand_result(ssd, [(HEIGHT, QUAD)])
    # u = 0.25 exactly, v = 3 / 16: the boundary between columns 0 and 1 belongs to the upper cell
    p, n = _lattice(4, ON)
    assert n == 3 and p == (0.0, 0.3125, ON)
    assert _cells(_grids(ssd, [p], res), 0, "seen") == {(0, 1): 1}
    # v = 0.25 exactly (n = 4 -> m = 2 (mod 5): u = 2 / 16 + 5 / 16): rows likewise
    q = _at(7 / 16.0, 4 / 16.0, ON)
    assert _cells(_grids(ssd, [q], res), 0, "seen") == {(1, 1): 1}
    # u - u0 = 32 cells = 8 m: out, and counted there; the cell below it is column 31
    far, n = _lattice(128, ON)
    near = _at(8.0 - 5 / 16.0, n / 16.0 + 0, ON)               # (123, n): 123 - 3 n = 120 for n = 1
    assert n == 1
    rec = _grids(ssd, [far, near, far[:2] + (ABOVE,), near[:2] + (ABOVE,)], res)
    assert _cells(rec, 0, "seen") == {(0, 30): 1} and _cells(rec, 0, "occ") == {(0, 30): 1}
    assert (rec.s[0].n_seen_out, rec.s[0].n_occ_out, rec.s[0].top_out) == (1, 1, 16384) and _cells(rec, 0, "top") == {(0, 30): 16384}
    # v = 8 cells = 2 m: out likewise (n = 32 -> m = 1 (mod 5): u = 1 / 16)
    deep = _at(1 / 16.0, 2.0, ON)
    rec = _grids(ssd, [deep, deep[:2] + (ABOVE,), _at(7 / 16.0, 29 / 16.0, ON)], res)
    assert (rec.s[0].n_seen_out, rec.s[0].n_occ_out) == (1, 1) and _cells(rec, 0, "seen") == {(7, 1): 1}


def test_a_parallelogram_whose_back_lies_left_of_its_front(ssd):
    """1.25 m deep, BL 1.25 m left of FL along the front edge: u0 = -1.25, the left side runs at u = -v, and the leftmost points (at the
    back) land in column 0.  (u, v) in sixteenths, m = 3 n (mod 5)"""
    bl = (1.25 * N[0] - 1.25 * E[0], 1.25 * N[1] - 1.25 * E[1])
    quad = [*FL, *FR, *bl, bl[0] + 6.0, bl[1] + 8.0]
    assert bl == (-1.75, -0.25) and tg.Axes(quad).u0 == -1.25
    res = cm.hand_result(ssd, [(HEIGHT, quad)])
    uv = [(-18, 19), (-13, 19), (-8, 19), (2, 19), (-19, 17), (3, 1), (-2, 1)]      # (-19, 17) and (-2, 1) lie outside the left side: nobody's
    for m, n in uv:
        assert (m - 3 * n) % 5 == 0
    rec = _grids(ssd, [_at(m / 16.0, n / 16.0, z) for m, n in uv for z in (ON, ABOVE)], res)
    want = {(4, 0): 1, (4, 1): 1, (4, 3): 1, (4, 5): 1, (0, 5): 1}
    assert _cells(rec, 0, "seen") == want == _cells(rec, 0, "occ") and rec.s[0].n_seen_out == rec.s[0].n_occ_out == 0


def test_both_ring_orientations_give_the_same_grid(ssd):
    """the quadrilateral mirrored in the line x = y is walked clockwise: a point mirrored with it has the same (u, v)"""
    mirrored = [QUAD[i ^ 1] for i in range(8)]
    assert tg.Axes(QUAD).o == 1.0 and tg.Axes(mirrored).o == -1.0
    uv = [(4, 3), (7, 4), (13, 1), (19, 3), (33, 16), (123, 1), (128, 1), (1, 32)]
    for m, n in uv:
        assert (m - 3 * n) % 5 == 0
    zs = [ON, ABOVE]
    a = _grids(ssd, [_at(m / 16.0, n / 16.0, z) for m, n in uv for z in zs], cm.hand_result(ssd, [(HEIGHT, QUAD)]))
    b = _grids(ssd, [(y, x, z) for x, y, z in (_at(m / 16.0, n / 16.0, z) for m, n in uv for z in zs)], cm.hand_result(ssd, [(HEIGHT, mirrored)]))
    assert bytes(a) == bytes(b) and sum(_cells(a, 0, "seen").values()) == 6 and a.s[0].n_seen_out == 2 and a.s[0].n_occ_out == 2


def test_degenerate_quadrilaterals_and_dead_frames(ssd):
    pts = [_at(19 / 16.0, 3 / 16.0, ON), _at(19 / 16.0, 3 / 16.0, ABOVE)]
    # FL == FR with an area: a triangle whose front edge has no length - the grid is not live, everything is counted outside it
    tri = [*FL, *FL, *BL, *BR]
    x, y = (BL[0] + BR[0]) / 3.0, (BL[1] + BR[1]) / 3.0
    inside = [(float(np.float32(x)), float(np.float32(y)), z) for z in (ON, ABOVE)]
    rec = _grids(ssd, inside, cm.hand_result(ssd, [(HEIGHT, tri)]))
    assert (rec.s[0].n_seen_out, rec.s[0].n_occ_out, rec.s[0].top_out) == (1, 1, 16384) and not _cells(rec, 0, "seen") and not _cells(rec, 0, "occ")
    # zero area and a NaN corner: nothing is counted anywhere, and nothing is hidden from the next surface
    nan = list(QUAD)
    nan[5] = math.nan
    for quad in ([0.0] * 8, [*FL, *FR, *FL, *FR], nan):
        rec = _grids(ssd, pts, cm.hand_result(ssd, [(HEIGHT, quad)]))
        assert bytes(rec)[8:] == bytes(52504 - 8)
        rec = _grids(ssd, pts, cm.hand_result(ssd, [(HEIGHT, quad), (HEIGHT, QUAD)]))
        assert bytes(rec.s[0]) == bytes(3088) and _cells(rec, 1, "seen") == {(0, 4): 1} and _cells(rec, 1, "occ") == {(0, 4): 1}
    # a frame the reference would have thrown on, and one without a step: no counts, a zero header
    for res in (cm.hand_result(ssd, [(HEIGHT, QUAD)], status=ob.ST_THROW), cm.hand_result(ssd, [(HEIGHT, QUAD)], n_steps=0)):
        assert bytes(_grids(ssd, pts, res)) == bytes(52504)
    assert _cells(_grids(ssd, pts, cm.hand_result(ssd, [(HEIGHT, QUAD)], status=2)), 0, "seen") == {(0, 4): 1}
    # invalid and out-of-range points
    assert bytes(_grids(ssd, [(0.0, 0.3125, 0.0), (0.0, 0.3125, -0.5), (0.0, 0.3125, 9.0)], cm.hand_result(ssd, [(HEIGHT, QUAD)])))[8:] == bytes(52504 - 8)


def test_the_slab_ends_and_the_lowest_index(ssd):
    x, y, _ = _at(19 / 16.0, 3 / 16.0, 0.0)
    res = cm.hand_result(ssd, [(HEIGHT, QUAD)])
    lo_z = np.float32(HEIGHT + LO)
    assert float(lo_z) == HEIGHT + LO
    # exactly lo above and below the height: tread points; the next float beyond: an occupant above (the band holds it), nothing below
    zs = [float(lo_z), float(np.float32(HEIGHT - LO)), float(np.nextafter(lo_z, np.float32(9))), float(np.nextafter(np.float32(HEIGHT - LO), np.float32(0)))]
    rec = _grids(ssd, [(x, y, z) for z in zs], res)
    assert _cells(rec, 0, "seen") == {(0, 4): 2} and _cells(rec, 0, "occ") == {(0, 4): 1}
    assert _cells(rec, 0, "top") == {(0, 4): int(np.rint((zs[2] - HEIGHT) * 65536.0))} == {(0, 4): 2048}
    # world_z moves the slab with it
    rec = _grids(ssd, [(x, y, z - 0.25) for z in zs], res, cal=_identity(ssd, world_z=0.25))
    assert _cells(rec, 0, "seen") == {(0, 4): 2} and _cells(rec, 0, "occ") == {(0, 4): 1}
    # overlapping quadrilaterals: the lowest index wins, for tread points and for occupants, in either order of the heights
    for h0, h1 in ((HEIGHT, HEIGHT + 0.015625), (HEIGHT + 0.015625, HEIGHT)):
        rec = _grids(ssd, [(x, y, HEIGHT + 0.0078125), (x, y, ABOVE)], cm.hand_result(ssd, [(h0, QUAD), (h1, QUAD)]))
        assert _cells(rec, 0, "seen") == {(0, 4): 1} and _cells(rec, 0, "occ") == {(0, 4): 1} and bytes(rec.s[1]) == bytes(3088)
    # in the slab of surface 1 alone, whose quadrilateral lies elsewhere: no tread point of anyone, and no occupant of surface 0
    far = [v + 16.0 for v in QUAD]
    rec = _grids(ssd, [(x, y, ABOVE)], cm.hand_result(ssd, [(HEIGHT, QUAD), (ABOVE, far)]))
    assert bytes(rec)[8:] == bytes(52504 - 8)
    # the lower index does not hold it: the next one does
    rec = _grids(ssd, [(x, y, ON), (x, y, ABOVE)], cm.hand_result(ssd, [(HEIGHT, far), (HEIGHT, QUAD)]))
    assert bytes(rec.s[0]) == bytes(3088) and _cells(rec, 1, "seen") == {(0, 4): 1} and _cells(rec, 1, "occ") == {(0, 4): 1}


def test_top_is_the_exact_rounded_maximum(ssd):
    x, y, _ = _at(19 / 16.0, 3 / 16.0, 0.0)
    x2, y2, _ = _at(33 / 16.0, 16 / 16.0, 0.0)
    res = cm.hand_result(ssd, [(HEIGHT, QUAD)])
    half = HEIGHT + 0.25 + 2.0 ** -17                       # 16384.5 units: rounds to even
    pts = [(x, y, HEIGHT + 0.125), (x, y, half), (x, y, HEIGHT + 0.0625), (x2, y2, HEIGHT + 0.375 + 3 * 2.0 ** -17), (x2, y2, HEIGHT + 0.25)]
    rec = _grids(ssd, pts, res)
    assert _cells(rec, 0, "occ") == {(0, 4): 3, (4, 8): 2} and _cells(rec, 0, "top") == {(0, 4): 16384, (4, 8): 24578}
    sol = ssd.tread_grid_solve(rec, res, tg.rule_of(ssd, RULE))
    assert sol.s[0].tallest == 24578 / 65536.0


def test_every_refusal_of_the_host_functions(ssd):
    L = ssd.lib()
    cfg, cal = _cfg(ssd, 2), _identity(ssd)
    pts = np.zeros((1, 2, 3), np.float32)
    res, rule, out = cm.hand_result(ssd, [(HEIGHT, QUAD)]), ssd.TreadGridRule(), ssd.FrameTreadGrid()
    p = pts.ctypes.data_as(C.c_void_p)

    def host(cfg=cfg, cal=cal, inp=0, intr=None, frame=p, res=res, rule=rule, out=out):
        return L.ssd_tread_grid_host(C.byref(cfg) if cfg else None, C.byref(cal) if cal else None, inp, C.byref(intr) if intr else None, frame,
                                     C.byref(res) if res else None, 0, C.byref(rule) if rule else None, C.byref(out) if out else None)

    assert host() == 0
    for kw in (dict(cfg=None), dict(cal=None), dict(frame=None), dict(res=None), dict(rule=None), dict(out=None), dict(inp=2), dict(inp=-1), dict(inp=1)):
        assert host(**kw) == -1 and L.ssd_last_error(), kw
    assert host(inp=1, intr=ssd.Intrinsics()) == -1 and b"intrinsics" in L.ssd_last_error()
    zero = ssd.default_config(8, 4)
    zero.width = 0
    assert host(cfg=zero) == -1
    for n in (-1, ssd.MAX_STEPS + 1):
        assert host(res=cm.hand_result(ssd, [], n_steps=n)) == -1 and b"n_steps" in L.ssd_last_error()
    nan = math.nan
    bad_rules = [(-0.01, 0.03, 0.5, 0.02), (1.01, 0.03, 0.5, 0.02), (nan, 0.03, 0.5, 0.02), (0.03, 0.0, 0.5, 0.02), (0.03, 1.01, 0.5, 0.02),
                 (0.03, nan, 0.5, 0.02), (0.03, 0.03, 0.03, 0.02), (0.03, 0.03, 8.01, 0.02), (0.03, 0.03, nan, 0.02),
                 (0.03, 0.03, 0.5, 0.0049), (0.03, 0.03, 0.5, 1.01), (0.03, 0.03, 0.5, nan), (0.03, 0.03, 0.5, 0.0), (0.03, 0.03, 0.5, -0.02)]
    good_rules = [(0.0, 0.03, 0.5, 0.005), (1.0, 1.0, 8.0, 1.0)]
    for bad in bad_rules:
        assert host(rule=ssd.TreadGridRule(*bad)) == -1 and b"rule" in L.ssd_last_error(), bad
    for good in good_rules:
        assert host(rule=ssd.TreadGridRule(*good)) == 0, good
    sol = ssd.FrameFootholds()

    def solve(grid=out, res=res, rule=rule, foot=(0.0, 0.0), sol=sol):
        return L.ssd_tread_grid_solve(C.byref(grid) if grid else None, C.byref(res) if res else None, C.byref(rule) if rule else None, 1, 1,
                                      foot[0], foot[1], C.byref(sol) if sol else None)

    assert solve() == 0
    for kw in (dict(grid=None), dict(res=None), dict(rule=None), dict(sol=None), dict(foot=(-0.01, 0.0)), dict(foot=(0.0, -0.01)), dict(foot=(nan, 0.0)),
               dict(foot=(0.0, nan))):
        assert solve(**kw) == -1 and L.ssd_last_error(), kw
    for bad in bad_rules:
        assert solve(rule=ssd.TreadGridRule(*bad)) == -1 and b"rule" in L.ssd_last_error(), bad
    for n in (-1, ssd.MAX_STEPS + 1):
        g = ssd.FrameTreadGrid()
        g.n_surfaces = n
        assert solve(grid=g) == -1 and b"n_surfaces" in L.ssd_last_error()
    # the device entry points without a handle
    dummy = C.c_void_p(4096)
    assert L.ssd_enqueue_tread_grid(None, dummy, 12 * 8, 1, None, 0, C.byref(rule), dummy) == -1 and b"null" in L.ssd_last_error()
    assert L.ssd_enqueue_cameras_tread_grid(None, dummy, 12 * 8, 1, None, 0, C.byref(rule), dummy) == -1
    assert L.ssd_fetch_tread_grid(None, None) == -1
    assert L.ssd_get_tread_grid_time(None, C.byref(C.c_float(0.0))) == -1
    r1, o1 = (ssd.FrameResult * 1)(), (ssd.FrameFootholds * 1)()
    assert L.ssd_process_host_tread_grid(None, dummy, 1, 0, C.byref(rule), 1, 1, 0.0, 0.0, r1, None, o1) == -1
    assert L.ssd_process_host_cameras_tread_grid(None, dummy, 1, None, 0, C.byref(rule), 1, 1, 0.0, 0.0, r1, None, o1) == -1
    with pytest.raises(ssd.SsdError, match="one frame"):
        ssd.tread_grid_host(cfg, cal, np.zeros((3, 3), np.float32), res, 0)


# ---- the solve against the brute force --------------------------------------------------------------------------------------------------
def _solve_both(ssd, per_surface, quads, rule=RULE, **kw):
    """ssd_tread_grid_solve on hand-made planes against the model's solve, surface by surface -> the FrameFootholds"""
    res = cm.hand_result(ssd, [(HEIGHT, q) for q in quads])
    rec = tg.record_of(ssd, per_surface, len(quads))
    sol = ssd.tread_grid_solve(rec, res, tg.rule_of(ssd, rule), **kw)
    assert (sol.n_surfaces, sol.ground) == (len(quads), 1)
    for k, q in enumerate(quads):
        tg.assert_solved(sol.s[k], tg.solve(tg.grid_of_record(rec, k), q, rule, **kw))
    assert bytes(sol)[8 + len(quads) * 328:] == bytes((ssd.MAX_STEPS - len(quads)) * 328), "records at k >= n_surfaces are zero"
    return sol


def _planes(free=(), occ=(), seen_n=1, occ_n=1):
    """planes with seen_n on the cells of the rectangles `free` [(row0, col0, rows, cols)] and occ_n on those of `occ`"""
    g = dict(seen=np.zeros((tg.ROWS, tg.COLS), np.int64), occ=np.zeros((tg.ROWS, tg.COLS), np.int64), top=np.zeros((tg.ROWS, tg.COLS), np.int64))
    for r0, c0, rows, cols in free:
        g["seen"][r0:r0 + rows, c0:c0 + cols] = seen_n
    for r0, c0, rows, cols in occ:
        g["occ"][r0:r0 + rows, c0:c0 + cols] = occ_n
    return g


def test_the_solve_on_grids_built_so_that_ties_occur(ssd):
    rect = lambda s: (s.col0, s.row0, s.cols, s.rows)
    # equal areas: 2 x 6 at row 4, 3 x 4 at row 1 (the smallest row0 wins), 4 x 3 at row 1 further right (the smallest col0 wins)
    sol = _solve_both(ssd, [_planes(free=[(4, 0, 2, 6), (1, 10, 3, 4), (1, 20, 4, 3)])], [QUAD])
    assert rect(sol.s[0]) == (10, 1, 4, 3) and sol.s[0].foothold == 1 and sol.s[0].n_free == 36
    # same row0 and col0: an L of 2 x 6 and 6 x 2 sharing their corner - the most cols
    sol = _solve_both(ssd, [_planes(free=[(1, 3, 2, 6), (1, 3, 6, 2)])], [QUAD])
    assert rect(sol.s[0]) == (3, 1, 6, 2)
    assert np.allclose(list(sol.s[0].centre), _at(1.5, 0.5, 0)[:2], rtol=0, atol=1e-9) and list(sol.s[0].size) == [1.5, 0.5]
    # a foot that fits only one of two equal-area rectangles, and one that fits nothing
    two = [_planes(free=[(0, 0, 2, 8), (3, 0, 4, 4)])]
    assert rect(_solve_both(ssd, two, [QUAD]).s[0]) == (0, 0, 8, 2)
    assert rect(_solve_both(ssd, two, [QUAD], foot_along=0.5, foot_deep=0.75).s[0]) == (0, 3, 4, 4)
    assert rect(_solve_both(ssd, two, [QUAD], foot_along=1.75, foot_deep=0.26).s[0]) == (0, 0, 8, 2)
    none = _solve_both(ssd, two, [QUAD], foot_along=1.1, foot_deep=0.6).s[0]
    assert none.foothold == 0 and rect(none) == (0, 0, 0, 0) and list(none.centre) == [0.0, 0.0] and list(none.size) == [0.0, 0.0] and none.n_free == 32
    assert _solve_both(ssd, two, [QUAD], foot_along=9.0).s[0].foothold == 0
    # supports: occupied wins over free; below both supports a cell is unseen; a support below 1 counts as 1
    g = _planes(free=[(0, 0, 8, 32)], occ=[(2, 5, 2, 3)], seen_n=4, occ_n=2)
    g["seen"][6, 20], g["seen"][6, 21] = 0, 3
    for ms, mo in ((1, 1), (4, 2), (4, 3), (5, 1), (0, 0), (-3, -3)):
        sol = _solve_both(ssd, [g], [QUAD], min_seen=ms, min_occ=mo)
        assert sol.s[0].n_occupied == (6 if mo <= 2 else 0) and sol.s[0].n_unseen == (256 - sol.s[0].n_occupied if ms == 5 else 2 if ms == 4 else 1)
    # tallest from top_out alone, and from a cell; two surfaces, the second a triangle without a front edge: every cell OUT
    g = _planes(free=[(0, 0, 8, 32)], occ=[(2, 5, 1, 1)])
    g["top"][2, 5], g["top_out"], g["n_occ_out"] = 3000, 70000, 2
    sol = _solve_both(ssd, [g, g], [QUAD, [*FL, *FL, *BL, *BR]])
    assert sol.s[0].tallest == 70000 / 65536.0 and sol.s[0].n_occupied == 1 and sol.s[0].n_free == 255
    assert sol.s[1].tallest == 70000 / 65536.0 and (sol.s[1].n_free, sol.s[1].n_occupied, sol.s[1].n_unseen, sol.s[1].foothold) == (0, 0, 0, 0)
    g["top_out"] = 5
    assert _solve_both(ssd, [g], [QUAD]).s[0].tallest == 3000 / 65536.0


def test_the_solve_marks_cells_outside_the_shrunk_quadrilateral(ssd):
    """a quadrilateral narrower and shallower than the grid, clockwise too: the cells whose centre lies outside are OUT, whatever they hold"""
    fr_, bl_ = (3.0 * 0.625, 4.0 * 0.625), (-0.8 * 1.25, 0.6 * 1.25)      # 3.125 m of front edge, 1.25 m deep
    quad = [*FL, *fr_, *bl_, fr_[0] + bl_[0], fr_[1] + bl_[1]]
    g = _planes(free=[(0, 0, 8, 32)])
    sol = _solve_both(ssd, [g], [quad])
    st = np.ctypeslib.as_array(sol.s[0].state)
    assert sol.s[0].n_free == 12 * 5 and np.all(st[:5, :12] == tg.FREE) and np.all(st[5:] == tg.OUT) and np.all(st[:, 13:] == tg.OUT)
    assert (sol.s[0].col0, sol.s[0].row0, sol.s[0].cols, sol.s[0].rows) == (0, 0, 12, 5)
    mirrored = [*FL, *fr_, -bl_[0], -bl_[1], fr_[0] - bl_[0], fr_[1] - bl_[1]]
    sol2 = _solve_both(ssd, [g], [mirrored])
    assert bytes(sol2.s[0].state) == bytes(sol.s[0].state)


# ---- host against model on the scenes -----------------------------------------------------------------------------------------------------
def _oracle_result(ssd, oracle, cfg, cal, frame):
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), frame)[0]
    return res, cm.result_of_oracle(ssd, res)


def _host_equals_model(ssd, cfg, cal, frame, fr, rule, intr=None, pts=None):
    """ssd_tread_grid_host on the frame against the model, cell by cell, and the occupant identity -> the record"""
    rec = ssd.tread_grid_host(cfg, cal, frame, fr, 1, tg.rule_of(ssd, rule), intr=intr)
    n = 0 if (fr.status & 1) else fr.n_steps
    tg.assert_record(ssd, rec, tg.grids(cfg, cal, fr, frame if pts is None else pts, rule), n, 1 if n else 0)
    _identity_holds(ssd, cfg, cal, frame, fr, rule, rec, intr=intr)
    return rec


def test_the_scene_clean_and_patched_vertices_and_depth(ssd, oracle):
    cfg, trans, frame = cm.scene_frame(ssd, 0.001, 7)
    cal = trans.constants
    res, fr = _oracle_result(ssd, oracle, cfg, cal, frame)
    assert fr.n_steps == 3 and fr.status == 0
    rec = _host_equals_model(ssd, cfg, cal, frame, fr, tg.RULE)
    assert all(tg.grid_of_record(rec, k)["seen"].sum() > 2000 and tg.grid_of_record(rec, k)["occ"].sum() == 0 for k in range(3))
    f2, sel = cm.patched(cfg, cal, fr, frame, expected_labels(oracle, cfg, cal, res, frame), 1)
    _, fr2 = _oracle_result(ssd, oracle, cfg, cal, f2)
    rec2 = _host_equals_model(ssd, cfg, cal, f2, fr2, tg.RULE)
    assert tg.grid_of_record(rec2, 1)["occ"].sum() >= 285 and tg.grid_of_record(rec2, 1)["top"].max() > 0.04 * 65536
    # another cell size and rule: the grid no longer holds the whole tread
    rec3 = _host_equals_model(ssd, cfg, cal, f2, fr2, (0.0, 0.02, 0.4, 0.02))
    assert rec3.s[1].n_seen_out > 0
    # 16-bit depth: the same pixels pulled in the depth image, judged on the deprojected points
    sc = gm.scene(ssd, "steps", sigma=0.001, seed=7)
    intr, depth = ssd.intrinsics_for_scene(sc), ssd.synth_depth_host([sc])[0]
    pts = ssd.deproject_host(intr, depth)
    resd, frd = _oracle_result(ssd, oracle, cfg, cal, pts)
    _, sel = cm.patched(cfg, cal, frd, pts, expected_labels(oracle, cfg, cal, resd, pts), 1)
    d2 = depth.copy()
    d2[sel] = np.round(d2[sel] * 0.9).astype(np.uint16)
    pts2 = ssd.deproject_host(intr, d2)
    _, fr2 = _oracle_result(ssd, oracle, cfg, cal, pts2)
    recd = _host_equals_model(ssd, cfg, cal, d2, fr2, tg.RULE, intr=intr, pts=pts2)
    assert tg.grid_of_record(recd, 1)["occ"].sum() >= 285
    recd0 = _host_equals_model(ssd, cfg, cal, depth, frd, tg.RULE, intr=intr, pts=pts)
    assert all(tg.grid_of_record(recd0, k)["occ"].sum() == 0 for k in range(3))


@pytest.mark.parametrize("layout", fw.FULL_LAYOUTS[:2])
def test_the_17_surface_frames_with_raised_points(ssd, oracle, layout):
    ref = fw.reference(ssd, oracle, layout)
    f, sel = cm.raised(ref)
    res, fr = _oracle_result(ssd, oracle, ref.cfg, ref.cal, f)
    assert (fr.n_steps, fr.status) == (ssd.MAX_STEPS, 0)
    rec = _host_equals_model(ssd, ref.cfg, ref.cal, f, fr, tg.WIDE_RULE)
    for k in range(ssd.MAX_STEPS):
        g = tg.grid_of_record(rec, k)
        assert g["occ"].sum() + g["n_occ_out"] >= 100 and g["seen"].sum() + g["n_seen_out"] > 0, k


# ---- the recipe under the oracle --------------------------------------------------------------------------------------------------------
def test_the_recipe_under_the_oracle(ssd, oracle):
    """the 3-step scene at sigma 1 mm under (0.03, 0.03, 0.5) with the model's cell and supports: the model meets the conditions, and the
    host functions give the model's states"""
    r = tg.recipe(ssd, oracle)
    n = r["fr"].n_steps
    assert n == r["fr2"].n_steps == 3
    assert all(s["n_occupied"] == 0 for s in r["clean"]), "no cell of a clean frame is OCCUPIED"
    st = r["patched"][1]["state"]
    assert r["patched"][1]["n_occupied"] >= 1, "the patched tread has an OCCUPIED cell"
    near = np.zeros_like(r["pulled_cells"])
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            shifted = np.zeros_like(near)
            src = r["pulled_cells"][max(0, -dr):tg.ROWS - max(0, dr), max(0, -dc):tg.COLS - max(0, dc)]
            shifted[max(0, dr):max(0, dr) + src.shape[0], max(0, dc):max(0, dc) + src.shape[1]] = src
            near |= shifted
    assert np.all(near[st == tg.OCCUPIED]), "every OCCUPIED cell lies within one cell of a cell that holds a pulled point"
    for k in (0, 2):
        assert np.array_equal(r["patched"][k]["state"], r["clean"][k]["state"]) and r["patched"][k]["rect"] == r["clean"][k]["rect"], k
    seen = r["grids_patched"][1]["seen"]
    vac = r["vacated_cells"]
    assert vac.any() and np.all((st[vac] != tg.FREE) | (seen[vac] >= tg.RECIPE_MIN_SEEN)), "a vacated cell is FREE only through other tread points"
    assert np.count_nonzero(vac & (st == tg.UNSEEN)) + np.count_nonzero(vac & (st == tg.OCCUPIED)) >= 1
    # the host functions on the same frames: the model's states, counts, rectangles and centres
    rule = tg.rule_of(ssd, r["rule"])
    for key, f, fr in (("clean", r["frames"][0], r["fr"]), ("patched", r["frames"][1], r["fr2"])):
        rec = ssd.tread_grid_host(r["cfg"], r["cal"], f, fr, 1, rule)
        sol = ssd.tread_grid_solve(rec, fr, rule, tg.RECIPE_MIN_SEEN, tg.RECIPE_MIN_OCC)
        for k in range(n):
            tg.assert_solved(sol.s[k], r[key][k])
    # the recorded figures (tools/tread_grid_accuracy.py) are this recipe's
    recorded = {}
    for line in open(tg.ACCURACY_FILE):
        if "=" in line and not line.startswith("#"):
            k, v = line.split("=", 1)
            recorded[k.strip()] = float(v.split()[0])
    assert (recorded["cell_m"], recorded["min_seen"], recorded["min_occ"]) == (tg.RECIPE_CELL, tg.RECIPE_MIN_SEEN, tg.RECIPE_MIN_OCC)
    assert recorded["occupied_cells_clean"] == 0 and recorded["occupied_cells_patched_tread"] == r["patched"][1]["n_occupied"]
