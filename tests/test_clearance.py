"""Tread clearance on the host (include/ssd_hip.h): the exports, every refusal of the host functions,
ssd_clearance_host against the numpy restatement of tests/clearance_model.py per pixel and per sum, the rule's edges on hand-made results
with lattice quadrilaterals (sides multiples of (3, 4): exact lengths), ssd_clearance_solve on lattice blobs, and the recipe under the
oracle - judged here, on the host functions, because the device is held to them byte for byte (tests/test_gpu_clearance.py).
No GPU needed."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import clearance_model as cm
import full_width as fw
import ground_model as gm
import oracle_binding as ob
from test_labels import expected_labels

NAMES = ["ssd_enqueue_clearance", "ssd_enqueue_cameras_clearance", "ssd_fetch_clearance", "ssd_get_clearance_time", "ssd_clearance_host",
         "ssd_clearance_solve", "ssd_process_host_clearance", "ssd_process_host_cameras_clearance"]


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_clearance", "enqueue_cameras_clearance", "fetch_clearance", "clearance_time_ms", "process_host_clearance",
              "process_host_cameras_clearance"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.clearance_host) and callable(ssd.clearance_solve)
    assert C.sizeof(ssd.ClearanceRule) == 24 and C.sizeof(ssd.Clearance) == 104 and C.sizeof(ssd.FrameClearance) == 8 + ssd.MAX_STEPS * 104
    r = ssd.ClearanceRule()
    assert (r.margin, r.lo, r.hi) == (0.03, 0.03, 0.5)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssd_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in header


# ---- the hand-made world: camera = camera-dependent world = external world ------------------------------------------------------------
S = 0.125                                               # the lattice: sides are S (3, 4) and S (-4, 3), 0.625 m long
FL, FR, BR, BL = (0.0, 0.25), (0.375, 0.75), (-0.125, 1.125), (-0.5, 0.625)
QUAD = [*FL, *FR, *BL, *BR]                             # ssd_step's order: front-left, front-right, back-left, back-right
MARGIN = 5.0 / 128                                      # 0.8 and 0.6 of it are dyadic: a point exactly on the shrunk side exists
LO, HI, HEIGHT = 0.03125, 0.5, 0.5


def _identity(ssd, t2=(0.0, 0.0), world_z=0.0):
    cal = ssd.Calibration()
    cal.a[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    cal.b[:] = [0, 0, 0]
    cal.r2[:] = [1, 0, 0, 1]
    cal.t2[:] = list(t2)
    cal.world_z = world_z
    return cal


def _cfg(ssd, n):
    cfg = ssd.default_config(8, 4)
    cfg.width, cfg.height = n, 1
    cfg.x_min, cfg.x_max, cfg.y_min, cfg.y_max, cfg.z_min, cfg.z_max = -8.0, 8.0, -8.0, 8.0, 0.0, 8.0
    return cfg


def _occupants(ssd, points, result, rule, cal=None):
    """the mask of ssd_clearance_host over hand-made points [(x, y, z)], checked against the model and its own sums"""
    pts = np.array(points, dtype=np.float32).reshape(-1, 3)
    assert np.array_equal(pts.astype(np.float64), np.array(points, dtype=np.float64).reshape(-1, 3)), "the points are float32 values"
    cfg, cal = _cfg(ssd, len(pts)), cal or _identity(ssd)
    rec, mask = ssd.clearance_host(cfg, cal, pts.reshape(1, -1, 3), result, 0, cm.rule_of(ssd, rule))
    mask = mask.reshape(-1)
    assert np.array_equal(mask, cm.occupants(cfg, cal, result, pts, rule))
    n = 0 if (result.status & 1) else result.n_steps
    assert rec.n_surfaces == n and cm.sums_of_record(rec, ssd.MAX_STEPS) == cm.sums(pts, mask, ssd.MAX_STEPS)
    return [int(v) for v in mask]


def _inward(t, d):
    """the point S t (3, 4) along the front side from FL, d inside it (the inward unit normal is (-0.8, 0.6))"""
    return (FL[0] + 3 * S * t - 0.8 * d, FL[1] + 4 * S * t + 0.6 * d)


def test_a_point_exactly_margin_from_a_side_is_kept_and_the_next_double_is_not(ssd):
    res = cm.hand_result(ssd, [(HEIGHT, QUAD)])
    rule = (MARGIN, LO, HI)
    x, y = _inward(0.5, MARGIN)
    assert (x, y) == (0.15625, 0.5234375)
    z = 0.75
    assert _occupants(ssd, [(x, y, z), _inward(0.5, MARGIN / 2) + (z,), _inward(0.5, 2 * MARGIN) + (z,)], res, rule) == [1, 0, 1]
    # the next double inside the margin, through the calibration's translation: ey = y + t2[1] is the double below y
    down = np.nextafter(y, 0.0)
    t2y = down - y
    assert y + t2y == down and t2y < 0
    assert _occupants(ssd, [(x, y, z)], res, rule, _identity(ssd, (0.0, t2y))) == [0]
    assert _occupants(ssd, [(x, y, z)], res, rule, _identity(ssd, (0.0, -t2y))) == [1]
    # margin 0 keeps a point on the side itself, and not the next double outside
    on = _inward(0.5, 0.0)
    assert _occupants(ssd, [on + (z,)], res, (0.0, LO, HI)) == [1]
    assert _occupants(ssd, [on + (z,)], res, (0.0, LO, HI), _identity(ssd, (0.0, np.nextafter(on[1], 0.0) - on[1]))) == [0]
    # all four sides: the point margin inside the middle of each is kept, the one half a margin inside is not
    ring, normals = [FL, FR, BR, BL], [(-0.8, 0.6), (-0.6, -0.8), (0.8, -0.6), (0.6, 0.8)]
    for i in range(4):
        mx, my = (ring[i][0] + ring[(i + 1) % 4][0]) / 2, (ring[i][1] + ring[(i + 1) % 4][1]) / 2
        pts = [(mx + d * normals[i][0], my + d * normals[i][1], z) for d in (MARGIN, MARGIN / 2)]
        assert _occupants(ssd, pts, res, rule) == [1, 0], i


def test_the_band_is_open_at_both_ends(ssd):
    res = cm.hand_result(ssd, [(HEIGHT, QUAD)])
    x, y = _inward(0.5, 0.3125)
    lo_z, hi_z = np.float32(HEIGHT + LO), np.float32(HEIGHT + HI)
    zs = [lo_z, np.nextafter(lo_z, np.float32(9)), np.nextafter(hi_z, np.float32(0)), hi_z, np.float32(HEIGHT), np.float32(HEIGHT - 0.25)]
    assert _occupants(ssd, [(x, y, float(z)) for z in zs], res, (MARGIN, LO, HI)) == [0, 1, 1, 0, 0, 0]
    # world_z moves the band with it
    assert _occupants(ssd, [(x, y, float(z) - 0.25) for z in zs], res, (MARGIN, LO, HI), _identity(ssd, world_z=0.25)) == [0, 1, 1, 0, 0, 0]


def test_the_slab_of_another_surface_and_the_lowest_surface_wins(ssd):
    far = [v + 4.0 for v in QUAD]
    x, y = _inward(0.5, 0.3125)
    rule = (MARGIN, LO, HI)
    # surface 1 lies elsewhere, 0.25 higher: points within lo of ITS height are nobody's, whatever its quadrilateral says
    res = cm.hand_result(ssd, [(HEIGHT, QUAD), (HEIGHT + 0.25, far)])
    zs = [0.75 - LO, 0.75, 0.75 + LO, float(np.nextafter(np.float32(0.75 + LO), np.float32(9))), float(np.nextafter(np.float32(0.75 - LO), np.float32(0)))]
    assert _occupants(ssd, [(x, y, z) for z in zs], res, rule) == [0, 0, 0, 1, 1]
    # overlapping quadrilaterals, both bands hold the point: the lowest index, in either order of the heights
    for h0, h1 in ((HEIGHT, HEIGHT + 0.0625), (HEIGHT + 0.0625, HEIGHT)):
        res = cm.hand_result(ssd, [(h0, QUAD), (h1, QUAD)])
        assert _occupants(ssd, [(x, y, 0.75)], res, rule) == [1]
    # above the lower surface's band, inside the upper one's
    res = cm.hand_result(ssd, [(HEIGHT, QUAD), (HEIGHT + 0.25, QUAD)])
    assert _occupants(ssd, [(x, y, 0.9375), (x, y, 1.0), (x, y, 1.0625)], res, rule) == [1, 2, 2]
    # the lower index does not hold it: the next one does
    res = cm.hand_result(ssd, [(HEIGHT, far), (HEIGHT, QUAD)])
    assert _occupants(ssd, [(x, y, 0.75), (x + 4.0, y + 4.0, 0.75)], res, rule) == [2, 1]


def test_ring_orientation_degenerate_quadrilaterals_and_dead_frames(ssd):
    x, y = _inward(0.5, 0.3125)
    pts = [(x, y, 0.75), (2.0, 2.0, 0.75)]
    rule = (MARGIN, LO, HI)
    mirrored = [*FR, *FL, *BR, *BL]                       # the same quadrilateral walked clockwise
    for quad in (QUAD, mirrored):
        assert _occupants(ssd, pts, cm.hand_result(ssd, [(HEIGHT, quad)]), rule) == [1, 0]
    nan = list(QUAD)
    nan[5] = math.nan
    for quad in ([0.0] * 8, [*FL, *FR, *FL, *FR], [x, y] * 4, nan):
        assert _occupants(ssd, pts, cm.hand_result(ssd, [(HEIGHT, quad)]), rule) == [0, 0]
        # ... and it hides nothing from the next surface
        assert _occupants(ssd, pts, cm.hand_result(ssd, [(HEIGHT, quad), (HEIGHT, QUAD)]), rule) == [2, 0]
    assert _occupants(ssd, pts, cm.hand_result(ssd, [(math.nan, QUAD)]), rule) == [0, 0]
    assert _occupants(ssd, pts, cm.hand_result(ssd, [(HEIGHT, QUAD)], status=ob.ST_THROW), rule) == [0, 0]
    assert _occupants(ssd, pts, cm.hand_result(ssd, [(HEIGHT, QUAD)], status=2), rule) == [1, 0]
    assert _occupants(ssd, pts, cm.hand_result(ssd, [(HEIGHT, QUAD)], n_steps=0), rule) == [0, 0]
    # invalid and out-of-range points
    res = cm.hand_result(ssd, [(HEIGHT - 1.0, QUAD)])
    assert _occupants(ssd, [(x, y, 0.0), (x, y, -0.25)], res, (MARGIN, LO, 2.0)) == [0, 0]


def test_every_refusal_of_the_host_functions(ssd):
    L = ssd.lib()
    cfg, cal = _cfg(ssd, 2), _identity(ssd)
    pts = np.zeros((1, 2, 3), np.float32)
    res, rule, out = cm.hand_result(ssd, [(HEIGHT, QUAD)]), ssd.ClearanceRule(), ssd.FrameMoments()
    p = pts.ctypes.data_as(C.c_void_p)

    def host(cfg=cfg, cal=cal, inp=0, intr=None, frame=p, res=res, rule=rule):
        return L.ssd_clearance_host(C.byref(cfg) if cfg else None, C.byref(cal) if cal else None, inp, C.byref(intr) if intr else None, frame,
                                    C.byref(res) if res else None, 0, C.byref(rule) if rule else None, C.byref(out), None)

    assert host() == 0
    assert L.ssd_clearance_host(C.byref(cfg), C.byref(cal), 0, None, p, C.byref(res), 0, C.byref(rule), None, None) == 0    # both outputs may be null
    for kw in (dict(cfg=None), dict(cal=None), dict(frame=None), dict(res=None), dict(rule=None), dict(inp=2), dict(inp=-1), dict(inp=1)):
        assert host(**kw) == -1 and L.ssd_last_error(), kw
    bad_intr = ssd.Intrinsics()
    assert host(inp=1, intr=bad_intr) == -1 and b"intrinsics" in L.ssd_last_error()
    zero = ssd.default_config(8, 4)
    zero.width = 0
    assert host(cfg=zero) == -1
    for n in (-1, ssd.MAX_STEPS + 1):
        assert host(res=cm.hand_result(ssd, [], n_steps=n)) == -1 and b"n_steps" in L.ssd_last_error()
    nan = math.nan
    for bad in ((-0.01, 0.03, 0.5), (1.01, 0.03, 0.5), (nan, 0.03, 0.5), (0.03, 0.0, 0.5), (0.03, 1.01, 0.5), (0.03, nan, 0.5),
                (0.03, 0.03, 0.03), (0.03, 0.03, 8.01), (0.03, 0.03, nan)):
        assert host(rule=ssd.ClearanceRule(*bad)) == -1 and b"rule" in L.ssd_last_error(), bad
    for good in ((0.0, 0.03, 0.5), (1.0, 1.0, 8.0), (0.0, 1e-9, 2e-9)):
        assert host(rule=ssd.ClearanceRule(*good)) == 0, good
    sol = ssd.FrameClearance()
    assert L.ssd_clearance_solve(None, C.byref(res), C.byref(cal), 1, C.byref(sol)) == -1
    assert L.ssd_clearance_solve(C.byref(out), None, C.byref(cal), 1, C.byref(sol)) == -1
    assert L.ssd_clearance_solve(C.byref(out), C.byref(res), None, 1, C.byref(sol)) == -1
    assert L.ssd_clearance_solve(C.byref(out), C.byref(res), C.byref(cal), 1, None) == -1
    for n in (-1, ssd.MAX_STEPS + 1):
        m = ssd.FrameMoments()
        m.n_surfaces = n
        assert L.ssd_clearance_solve(C.byref(m), C.byref(res), C.byref(cal), 1, C.byref(sol)) == -1 and b"n_surfaces" in L.ssd_last_error()
    # the device entry points without a handle
    dummy = C.c_void_p(4096)
    assert L.ssd_enqueue_clearance(None, dummy, 12 * 8, 1, None, 0, C.byref(rule), dummy, None, 0) == -1 and b"null" in L.ssd_last_error()
    assert L.ssd_enqueue_cameras_clearance(None, dummy, 12 * 8, 1, None, 0, C.byref(rule), dummy, None, 0) == -1
    assert L.ssd_fetch_clearance(None, None) == -1
    assert L.ssd_get_clearance_time(None, C.byref(C.c_float(0.0))) == -1
    r1, o1 = (ssd.FrameResult * 1)(), (ssd.FrameClearance * 1)()
    assert L.ssd_process_host_clearance(None, dummy, 1, 0, C.byref(rule), 50, r1, None, None, o1) == -1
    assert L.ssd_process_host_cameras_clearance(None, dummy, 1, None, 0, C.byref(rule), 50, r1, None, None, o1) == -1
    with pytest.raises(ssd.SsdError, match="one frame"):
        ssd.clearance_host(cfg, cal, np.zeros((3, 3), np.float32), res, 0)


# ---- the solve on lattice blobs -----------------------------------------------------------------------------------------------------
def test_solve_on_lattice_blobs(ssd):
    """a blob of dyadic points standing on the lattice quadrilateral, under a calibration whose up axis is the camera's z: every figure
    has a closed form"""
    cal = _identity(ssd, t2=(0.25, -0.5), world_z=0.125)
    quad = [QUAD[i] + (0.25 if i % 2 == 0 else -0.5) for i in range(8)]
    res = cm.hand_result(ssd, [(HEIGHT + 0.125, quad), (2.0, quad)])
    # 5 x 4 x 3 points on a grid of 1/64 m around a point 0.3125 behind the middle of the front side
    cx, cy = _inward(0.5, 0.3125)
    g = np.array([(cx + i / 64.0, cy + j / 64.0, 0.625 + k / 64.0) for i in range(5) for j in range(4) for k in range(3)])
    pts = g.astype(np.float32)
    assert np.array_equal(pts.astype(np.float64), g)
    cfg = _cfg(ssd, len(pts))
    rule = ssd.ClearanceRule(MARGIN, LO, HI)
    rec, mask = ssd.clearance_host(cfg, cal, pts.reshape(1, -1, 3), res, 0, rule)
    assert mask.reshape(-1).tolist() == [1] * len(pts) and rec.s[0].m.n == 60 and rec.s[1].m.n == 0
    for support, status in ((60, ssd.CL_OCCUPIED), (61, ssd.CL_FREE), (0, ssd.CL_OCCUPIED), (-5, ssd.CL_OCCUPIED)):
        sol = ssd.clearance_solve(rec, res, cal, support)
        s = sol.s[0]
        assert (sol.n_surfaces, s.status, s.n, s.n_far) == (2, status, 60, 0)
        if status == ssd.CL_FREE:
            assert list(s.centroid) == [0.0] * 3 and (s.height_mean, s.height_rms, s.from_front, s.along_front) == (0.0,) * 4 and list(s.extent) == [0.0] * 3
            continue
        mean = g.mean(axis=0)
        want = [mean[0] + 0.25, mean[1] - 0.5, mean[2] + 0.125]
        assert np.allclose(list(s.centroid), want, rtol=0, atol=1e-9)
        assert abs(s.height_mean - (mean[2] + 0.125 - (HEIGHT + 0.125))) < 1e-9
        assert abs(s.height_rms - g[:, 2].std()) < 1e-9
        # the blob's middle: 2 / 64 right and 1.5 / 64 up of (cx, cy), which is 0.3125 behind the middle of the front side
        off = np.array([2 / 64.0, 1.5 / 64.0])
        assert abs(s.along_front - (0.3125 + off @ np.array([0.6, 0.8]))) < 1e-9
        assert abs(s.from_front - (0.3125 + off @ np.array([-0.8, 0.6]))) < 1e-9
        ext = np.sqrt(np.sort(np.linalg.eigvalsh(np.cov(g.T, bias=True)))[::-1])
        assert np.allclose(list(s.extent), ext, rtol=0, atol=1e-9)
        assert sol.s[1].status == ssd.CL_FREE and sol.s[1].n == 0
        assert bytes(sol)[8 + 2 * 104:] == bytes(8 + ssd.MAX_STEPS * 104 - 8 - 2 * 104), "records at k >= n_surfaces are zero"
    # a clockwise ring measures the same distance behind the front edge
    mirrored = [quad[2], quad[3], quad[0], quad[1], quad[6], quad[7], quad[4], quad[5]]
    s = ssd.clearance_solve(rec, cm.hand_result(ssd, [(HEIGHT + 0.125, mirrored)]), cal, 1).s[0]
    assert abs(s.from_front - (0.3125 + np.array([2 / 64.0, 1.5 / 64.0]) @ np.array([-0.8, 0.6]))) < 1e-9 and abs(s.along_front - (0.625 - (0.3125 + np.array([2 / 64.0, 1.5 / 64.0]) @ np.array([0.6, 0.8])))) < 1e-9


# ---- the recipe under the oracle ----------------------------------------------------------------------------------------------------
def _oracle_result(ssd, oracle, cfg, cal, frame):
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), frame)[0]
    return res, cm.result_of_oracle(ssd, res)


def _host_equals_model(ssd, cfg, cal, frame, fr, rule, intr=None, pts=None):
    """ssd_clearance_host on the frame against the model, per pixel and per sum -> (record, mask)"""
    rec, mask = ssd.clearance_host(cfg, cal, frame, fr, 1, cm.rule_of(ssd, rule), intr=intr)
    pts = frame if pts is None else pts
    want = cm.occupants(cfg, cal, fr, pts, rule)
    assert np.array_equal(mask.reshape(-1), want)
    n = 0 if (fr.status & 1) else fr.n_steps
    assert (rec.n_surfaces, rec.ground) == (n, 1 if n else 0)
    assert cm.sums_of_record(rec, ssd.MAX_STEPS) == cm.sums(pts, want, ssd.MAX_STEPS)
    return rec, mask


@pytest.mark.parametrize("sigma", [0.001, 0.003])
@pytest.mark.parametrize("seed", [7, 11])
def test_clean_scenes_hold_nothing_and_the_margin_is_why(ssd, oracle, sigma, seed):
    cfg, trans, frame = cm.scene_frame(ssd, sigma, seed)
    cal = trans.constants
    res, fr = _oracle_result(ssd, oracle, cfg, cal, frame)
    assert fr.n_steps == 3 and fr.status == 0
    rec, mask = _host_equals_model(ssd, cfg, cal, frame, fr, cm.RULE)
    assert [int(rec.s[k].m.n + rec.s[k].n_far) for k in range(ssd.MAX_STEPS)] == [0] * ssd.MAX_STEPS and not mask.any()
    rec0, _ = _host_equals_model(ssd, cfg, cal, frame, fr, (0.0,) + cm.RULE[1:])
    assert max(int(rec0.s[k].m.n) for k in range(fr.n_steps)) > 500, "without the margin the riser faces leak in"


@pytest.mark.parametrize("sigma", [0.001, 0.003])
def test_a_patch_pulled_off_a_tread_is_found_on_it(ssd, oracle, sigma):
    """tread 1 and the top tread, vertices and 16-bit depth; the recorded shares (profiles/clearance_accuracy.txt) less 0.03"""
    recorded = cm.recorded_accuracy()
    cfg, trans, frame = cm.scene_frame(ssd, sigma, 7)
    cal = trans.constants
    res, fr = _oracle_result(ssd, oracle, cfg, cal, frame)
    labels = expected_labels(oracle, cfg, cal, res, frame)
    for surface, key in ((1, "tread1"), (fr.n_steps - 1, "top")):
        f2, sel = cm.patched(cfg, cal, fr, frame, labels, surface)
        res2, fr2 = _oracle_result(ssd, oracle, cfg, cal, f2)
        assert fr2.n_steps == fr.n_steps and fr2.status == 0
        rec, mask = _host_equals_model(ssd, cfg, cal, f2, fr2, cm.RULE)
        share = np.count_nonzero(mask[sel] == surface + 1) / np.count_nonzero(sel)
        assert share >= recorded["worst_share_%s" % key] - 0.03, share
        if surface == 1:
            assert share >= 0.95 and not mask[~sel].any() and not (mask[sel] > 0)[mask[sel] != surface + 1].any(), "on its tread, none elsewhere"
        sol = ssd.clearance_solve(rec, fr2, cal)
        assert sol.s[surface].status == ssd.CL_OCCUPIED
        if surface == 1:
            assert [sol.s[k].status for k in range(fr2.n_steps)] == [ssd.CL_FREE, ssd.CL_OCCUPIED, ssd.CL_FREE]
        assert 0.04 < sol.s[surface].height_mean < 0.12
    # 16-bit depth: the same pixels pulled in the depth image, judged on the deprojected points
    sc = gm.scene(ssd, "steps", sigma=sigma, seed=7)
    intr, depth = ssd.intrinsics_for_scene(sc), ssd.synth_depth_host([sc])[0]
    pts = ssd.deproject_host(intr, depth)
    resd, frd = _oracle_result(ssd, oracle, cfg, cal, pts)
    _, sel = cm.patched(cfg, cal, frd, pts, expected_labels(oracle, cfg, cal, resd, pts), 1)
    d2 = depth.copy()
    d2[sel] = np.round(d2[sel] * 0.9).astype(np.uint16)
    pts2 = ssd.deproject_host(intr, d2)
    res2, fr2 = _oracle_result(ssd, oracle, cfg, cal, pts2)
    rec, mask = _host_equals_model(ssd, cfg, cal, d2, fr2, cm.RULE, intr=intr, pts=pts2)
    assert np.count_nonzero(mask[sel] == 2) >= 0.95 * np.count_nonzero(sel) and not mask[~sel].any()


@pytest.mark.parametrize("layout", fw.FULL_LAYOUTS)
def test_every_row_of_the_17_surface_frames(ssd, oracle, layout):
    ref = fw.reference(ssd, oracle, layout)
    f, sel = cm.raised(ref)
    res, fr = _oracle_result(ssd, oracle, ref.cfg, ref.cal, f)
    assert (fr.n_steps, fr.status) == (ssd.MAX_STEPS, 0), "the raised points leave the frame its 17 surfaces"
    rec, mask = _host_equals_model(ssd, ref.cfg, ref.cal, f, fr, cm.WIDE_RULE)
    rows = [int(rec.s[k].m.n + rec.s[k].n_far) for k in range(ssd.MAX_STEPS)]
    assert min(rows) >= 100, rows
    # ... and without them only the faces hanging over the overlapping treads: the ground and the two top surfaces hold nothing
    _, fr0 = _oracle_result(ssd, oracle, ref.cfg, ref.cal, ref.xyz)
    rec0, _ = _host_equals_model(ssd, ref.cfg, ref.cal, ref.xyz, fr0, cm.WIDE_RULE)
    rows0 = [int(rec0.s[k].m.n) for k in range(ssd.MAX_STEPS)]
    assert rows0[0] == rows0[15] == rows0[16] == 0 and min(rows0[1:15]) > 500, rows0


def test_the_recorded_accuracy_holds(ssd, oracle):
    """tools/clearance_accuracy.py's figures again, on the first seed: the zero, and the shares less 0.03"""
    recorded = cm.recorded_accuracy()
    assert recorded["false_occupants_clean"] == 0
    got = cm.accuracy(ssd, oracle, sigmas=(0.001, 0.003), seeds=(7,))
    assert got["false_occupants_clean"] == 0
    for key in ("worst_share_tread1", "worst_share_top"):
        assert got[key] >= recorded[key] - 0.03, (key, got[key], recorded[key])
    assert got["worst_centroid_distance_m"] <= recorded["worst_centroid_distance_m"] + 0.01
