"""The surface fit on the host (include/ssd_hip.h): ssd_surface_moments_host against Python integers, the solve
on synthetic patches of known tilt, the statuses, surface 0 through the ground fit's solve, and the chain oracle -> labels -> sums ->
planes on staircase scenes - judged here, on the host functions, because the device is held to the host sums bit for bit
(tests/test_gpu_surface_fit.py).  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import ground_model as gm
import surface_model as sm

NAMES = ["ssd_enqueue_surface_moments", "ssd_enqueue_depth_surface_moments", "ssd_get_surface_moments_time_back", "ssd_surface_moments_host",
         "ssd_surface_fit_solve", "ssd_process_host_surfaces"]


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_surface_moments", "process_host_surfaces", "surface_moments_time_ms"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.surface_moments_host) and callable(ssd.surface_fit_solve)
    assert C.sizeof(ssd.SurfaceMoments) == 88 and C.sizeof(ssd.FrameMoments) == 8 + ssd.MAX_STEPS * 88
    assert C.sizeof(ssd.SurfaceFit) == 24 + 8 * 10 and C.sizeof(ssd.FrameSurfaces) == 8 + ssd.MAX_STEPS * C.sizeof(ssd.SurfaceFit)


def test_null_arguments_are_rejected(ssd):
    L = ssd.lib()
    dummy = C.c_void_p(4096)
    assert L.ssd_enqueue_surface_moments(None, dummy, 12 * 640 * 480, 1, None, dummy) == -1
    assert b"null" in L.ssd_last_error()
    assert L.ssd_enqueue_depth_surface_moments(None, dummy, 2 * 640 * 480, 1, None, dummy) == -1
    ms = C.c_float(0.0)
    assert L.ssd_get_surface_moments_time_back(None, 0, C.byref(ms)) == -1
    res, out = (ssd.FrameResult * 1)(), (ssd.FrameSurfaces * 1)()
    assert L.ssd_process_host_surfaces(None, dummy, 1, 0, res, None, 1, out) == -1
    assert L.ssd_surface_fit_solve(None, None, 1, None) == -1
    assert L.ssd_surface_moments_host(None, 0, None, None, None, 0, 0, None) == -1


def hand_made(ssd):
    """(cfg, points [H, W, 3], labels [H, W]): three surfaces, every coordinate at, next to and beyond 16 m, negative ones too"""
    w, h = 8, 4
    cfg = ssd.default_config(w, h)
    f = np.float32
    down = lambda v: np.nextafter(f(v), f(0.0))            # noqa: E731
    rows = [
        ((0.25, -0.5, 1.0), 1), ((0.2500153, 0.3, 1.2), 1), ((-1.5, 2.0, 0.75), 1), ((3.0, -2.0, 4.0), 0),
        ((15.99999, 1.0, 1.0), 2),                      # q = 1048575: the last one inside 2^20
        ((down(16.0), 1.0, 1.0), 2),                    # |v| < 16 but q rounds to 2^20: far
        ((16.0, 1.0, 1.0), 2), ((1.0, -16.0, 1.0), 2), ((1.0, 1.0, 17.5), 2), ((-15.99999, -15.99999, 15.99999), 2),
        ((1.0, 1.0, 1.0), 3), ((-16.0, 40.0, 1.0), 3), ((0.1, 0.2, 0.3), 3), ((1e-6, -1e-6, 7.62939453125e-06), 3),   # halves round to even
        ((100.0, 0.0, 1.0), 0), ((0.0, 0.0, 0.0), 0),
        ((2.0, 2.0, 2.0), 1), ((0.5, 0.25, 0.125), 2),
    ]
    pts = np.zeros((h * w, 3), dtype=np.float32)
    lab = np.zeros(h * w, dtype=np.uint8)
    for i, (p, l) in enumerate(rows):
        pts[i], lab[i] = p, l
    return cfg, pts.reshape(h, w, 3), lab.reshape(h, w)


def test_moments_of_hand_made_labels_equal_python_integers(ssd):
    cfg, pts, lab = hand_made(ssd)
    want = sm.moments_py(pts, lab, 3)
    assert [r[0] for r in want] == [4, 3, 3] and [r[3] for r in want] == [0, 4, 1], "the cloud reaches both sides of 16 m"
    assert want == sm.moments_np(pts, lab, 3)
    got = ssd.surface_moments_host(cfg, pts, lab, 3, 1)
    assert sm.frame_tuple(got) == (3, 1, sm.pad(want, ssd.MAX_STEPS))
    # more surfaces declared than labels name: their records are zero; ground as given
    got = ssd.surface_moments_host(cfg, pts, lab, 5, 0)
    assert sm.frame_tuple(got) == (5, 0, sm.pad(want, ssd.MAX_STEPS))
    with pytest.raises(ssd.SsdError, match="label"):
        ssd.surface_moments_host(cfg, pts, lab, 2, 1)
    with pytest.raises(ssd.SsdError, match="n_surfaces"):
        ssd.surface_moments_host(cfg, pts, lab, ssd.MAX_STEPS + 1, 1)
    none = ssd.surface_moments_host(cfg, pts, np.zeros_like(lab), 0, 0)
    assert bytes(none) == bytes(C.sizeof(ssd.FrameMoments))


def test_depth_input_is_its_deprojection(ssd):
    sc = gm.scene(ssd, "steps")
    depth = ssd.synth_depth_host([sc])[0]
    intr = ssd.intrinsics_for_scene(sc)
    pts = ssd.deproject_host(intr, depth)
    cfg = ssd.default_config(gm.W, gm.H)
    rng = np.random.default_rng(3)
    lab = rng.integers(0, 4, size=(gm.H, gm.W)).astype(np.uint8)
    got = ssd.surface_moments_host(cfg, depth, lab, 3, 1, intr=intr)
    assert bytes(got) == bytes(ssd.surface_moments_host(cfg, pts, lab, 3, 1))
    assert sm.frame_tuple(got)[2] == sm.pad(sm.moments_np(pts, lab, 3), ssd.MAX_STEPS) and got.s[0].m.n > 1000


def _calibration(ssd, pitch_deg=50.0, roll_deg=0.0, yaw=(0.6, -0.8, 0.8, 0.6), t2=(1.5, -2.5), world_z=0.25):
    cal = ssd.transformation_for_scene(gm.scene(ssd, "floor", pitch_deg=pitch_deg, roll_deg=roll_deg)).constants
    out = ssd.Calibration()
    C.memmove(C.byref(out), C.byref(cal), C.sizeof(out))
    out.r2[:] = yaw
    out.t2[:] = t2
    out.world_z = world_z
    return out


def _patch(cal, normal_ext, centre_ext, half=(0.4, 0.15), n=4000, sigma=0.0, seed=1):
    """camera points (float32 [n, 3]) of a rectangular patch with the given unit normal and centre in EXTERNAL world coordinates"""
    rng = np.random.default_rng(seed)
    a = np.array(list(cal.a)).reshape(3, 3)
    b = np.array(list(cal.b))
    r2 = np.array(list(cal.r2)).reshape(2, 2)
    nrm = np.asarray(normal_ext, dtype=np.float64)
    nrm = nrm / np.linalg.norm(nrm)
    u = np.cross(nrm, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    ext = (np.asarray(centre_ext)[None, :] + rng.uniform(-half[0], half[0], (n, 1)) * u + rng.uniform(-half[1], half[1], (n, 1)) * v
           + rng.normal(0.0, sigma, (n, 1)) * nrm if sigma > 0 else
           np.asarray(centre_ext)[None, :] + rng.uniform(-half[0], half[0], (n, 1)) * u + rng.uniform(-half[1], half[1], (n, 1)) * v)
    w = ext.copy()
    w[:, :2] = (ext[:, :2] - np.array(list(cal.t2))) @ np.linalg.inv(r2).T
    w[:, 2] = ext[:, 2] - cal.world_z
    cam = (w - b) @ a                                   # a is a rotation: its inverse is its transpose
    return cam.astype(np.float32), nrm


def _frame_moments(ssd, patches):
    """FrameMoments of hand-placed patches (one surface each) through ssd_surface_moments_host"""
    n = sum(len(p) for p in patches)
    cfg = ssd.default_config(n, 1)
    pts = np.concatenate(patches).reshape(1, n, 3)
    lab = np.concatenate([np.full(len(p), k + 1, dtype=np.uint8) for k, p in enumerate(patches)]).reshape(1, n)
    return ssd.surface_moments_host(cfg, pts, lab, len(patches), 0)


@pytest.mark.parametrize("pitch_deg,roll_deg", [(50.0, 0.0), (38.0, 4.0)])
def test_the_solve_recovers_known_normals_and_tilts(ssd, pitch_deg, roll_deg):
    """noise-free patches: the 2^-16 m fixed point is 4.4e-6 m rms over half-extents of 0.15 m and more - 1e-4 rad; centroids of 4000
    points to 1e-5 m; with 2 mm of noise across the plane 0.002 / (0.087 sqrt(4000)) = 4e-4 rad at one sigma, five allowed"""
    cal = _calibration(ssd, pitch_deg, roll_deg)
    cases = [((0.0, 0.0, 1.0), (1.0, -2.0, 0.25)), ((0.0, math.sin(0.05), math.cos(0.05)), (1.2, -1.6, 0.45)),
             ((math.sin(0.2), 0.0, math.cos(0.2)), (1.1, -1.9, 0.60)), ((0.1, -0.2, 0.9), (1.4, -1.7, 0.35))]
    patches, normals = zip(*[_patch(cal, nrm, c, seed=i) for i, (nrm, c) in enumerate(cases)])
    fit = ssd.surface_fit_solve(_frame_moments(ssd, patches), cal, 100)
    assert fit.n_surfaces == 4 and fit.ground == 0
    for k, ((_, centre), nrm) in enumerate(zip(cases, normals)):
        s = fit.s[k]
        assert s.status == ssd.GF_OK and s.n == 4000 and s.n_far == 0
        assert abs(np.linalg.norm(list(s.normal)) - 1.0) < 1e-12 and s.normal[2] > 0
        assert gm.angle(list(s.normal), nrm) <= 1e-4, k
        assert abs(s.tilt - math.acos(nrm[2])) <= 1e-4, k
        assert np.max(np.abs(np.array(list(s.centroid)) - centre)) <= 0.02, "a uniform sample's mean: 0.4 / sqrt(3 * 4000) = 4e-3 at one sigma"
        assert s.rms <= 1e-5 and s.extent[0] >= s.extent[1] > 0.05
        assert abs(s.extent[0] - 0.4 / math.sqrt(3)) < 0.02 and abs(s.extent[1] - 0.15 / math.sqrt(3)) < 0.01
    for k in range(4, ssd.MAX_STEPS):
        assert bytes(fit.s[k]) == bytes(C.sizeof(ssd.SurfaceFit))
    noisy, nrm = _patch(cal, (0.1, -0.2, 0.9), (1.4, -1.7, 0.35), sigma=0.002, seed=9)
    s = ssd.surface_fit_solve(_frame_moments(ssd, [noisy]), cal, 100).s[0]
    assert s.status == ssd.GF_OK and gm.angle(list(s.normal), nrm) <= 2e-3 and abs(s.rms - 0.002) < 2e-4


def test_the_centroid_is_the_mean_in_external_world_coordinates(ssd):
    cal = _calibration(ssd)
    patch, _ = _patch(cal, (0.0, 0.0, 1.0), (1.0, -2.0, 0.25), n=1000)
    s = ssd.surface_fit_solve(_frame_moments(ssd, [patch]), cal, 100).s[0]
    a, b = np.array(list(cal.a)).reshape(3, 3), np.array(list(cal.b))
    q = np.rint(patch.astype(np.float64) * 65536.0) / 65536.0
    w = q.mean(axis=0) @ a.T + b
    want = np.array(list(np.array(list(cal.r2)).reshape(2, 2) @ w[:2] + np.array(list(cal.t2))) + [w[2] + cal.world_z])
    assert np.max(np.abs(np.array(list(s.centroid)) - want)) < 1e-12


def _zero_doubles(s):
    return list(s.normal) == [0.0] * 3 and list(s.centroid) == [0.0] * 3 and s.tilt == 0.0 and s.rms == 0.0 and list(s.extent) == [0.0, 0.0]


def test_status_few_and_degenerate(ssd):
    cal = _calibration(ssd)
    patch, _ = _patch(cal, (0.0, 0.0, 1.0), (1.0, -2.0, 0.25), n=500)
    t = np.linspace(-0.5, 0.5, 800)[:, None]
    line = (np.array([0.2, -0.1, 1.5]) + t * np.array([0.3, -0.7, 0.11])).astype(np.float32)
    rng = np.random.default_rng(5)
    blob = (np.array([0.0, 0.0, 1.5]) + rng.uniform(-0.05, 0.05, (3000, 3))).astype(np.float32)
    far = patch.copy()
    far[:, 0] += 20.0
    fm = _frame_moments(ssd, [patch, line, blob, far])
    fit = ssd.surface_fit_solve(fm, cal, 500)
    assert [fit.s[k].status for k in range(4)] == [ssd.GF_OK, ssd.GF_DEGENERATE, ssd.GF_DEGENERATE, ssd.GF_FEW]
    assert [int(fit.s[k].n) for k in range(4)] == [500, 800, 3000, 0] and fit.s[3].n_far == 500
    assert all(_zero_doubles(fit.s[k]) for k in (1, 2, 3)) and not _zero_doubles(fit.s[0])
    fit = ssd.surface_fit_solve(fm, cal, 501)
    assert fit.s[0].status == ssd.GF_FEW and _zero_doubles(fit.s[0]) and fit.s[0].n == 500
    for min_points in (0, 1):
        assert ssd.surface_fit_solve(fm, cal, min_points).s[3].status == ssd.GF_FEW, "no point at all is FEW whatever min_points"
    bad = ssd.FrameMoments()
    bad.n_surfaces = ssd.MAX_STEPS + 1
    with pytest.raises(ssd.SsdError, match="n_surfaces"):
        ssd.surface_fit_solve(bad, cal, 1)


@pytest.mark.parametrize("kind", ["steps", "outliers"])
def test_surface_0_goes_straight_into_the_ground_fit(ssd, oracle, kind):
    """surface 0's m through ssd_ground_fit_solve = a direct ground-fit solve of the same moments, byte for byte - and the plane it
    gives is the surface fit's own: the same normal (through -A and r2) and the same rms"""
    sc = gm.scene(ssd, kind)
    cfg = ssd.default_config(gm.W, gm.H)
    cal = ssd.transformation_for_scene(sc).constants
    frame = ssd.synth_host([sc])[0]
    res, labels, fm, fit = sm.oracle_planes(ssd, oracle, cfg, cal, frame)
    assert fm.ground == 1 and fm.n_surfaces == res.n_steps >= 2
    direct = ssd.ground_fit_solve(gm.moments_struct(ssd, *gm.moments_tuple(fm.s[0].m)), cal, sm.MIN_POINTS)
    through = ssd.ground_fit_solve(fm.s[0].m, cal, sm.MIN_POINTS)
    assert bytes(through) == bytes(direct) and direct.status == ssd.GF_OK
    a = np.array(list(cal.a)).reshape(3, 3)
    up = -(a @ np.array(list(direct.normal)))
    r2 = np.array(list(cal.r2)).reshape(2, 2)
    want = list(r2 @ up[:2]) + [up[2]]
    assert np.max(np.abs(np.array(list(fit.s[0].normal)) - want)) < 1e-15 and fit.s[0].rms == direct.rms
    assert abs(fit.s[0].tilt - direct.tilt) < 1e-9, "the prior is the calibration in use: the ground fit's tilt is the surface's"


def test_the_oracles_surfaces_come_out_level_to_the_recorded_accuracy(ssd, oracle):
    """3-step 256 x 192 scenes, sigma 1 mm and 3 mm, the true calibration and calibrations pitched or rolled by a few tenths of a degree:
    every surface's tilt against the angle between the true calibration's up vector and the used one's.  The bound is three times the
    worst figure tools/surface_fit_accuracy.py recorded (profiles/surface_fit_accuracy.txt) - the margin is for other seeds, not for the
    code."""
    rec = sm.recorded_accuracy()
    assert 0 < rec["worst_tilt_error_rad"] < 0.02
    for name, cfg, frame, truth, cal in sm.accuracy_cases(ssd):
        want, res, rows = sm.tilt_errors(ssd, oracle, cfg, frame, truth, cal)
        assert res.n_steps == len(rows) >= 3, name
        for k, status, n, tilt, err, rms in rows:
            print("%s surface %d: tilt %.3e error %.3e rms %.2e n %d" % (name, k, tilt, err, rms, n))
            assert status == ssd.GF_OK and n >= sm.MIN_POINTS, (name, k)
            assert err <= 3 * rec["worst_tilt_error_rad"], (name, k, err)


def test_the_sums_carry_the_labels_counts(ssd, oracle):
    """m.n + n_far per surface = the oracle's n_in_quad; a frame without stairs is all zero"""
    cfg = ssd.default_config(gm.W, gm.H)
    sc = gm.scene(ssd, "steps")
    cal = ssd.transformation_for_scene(sc).constants
    frame = ssd.synth_host([sc])[0]
    res, labels, fm, fit = sm.oracle_planes(ssd, oracle, cfg, cal, frame)
    counts = np.bincount(labels, minlength=ssd.MAX_STEPS + 1)
    assert [int(fm.s[k].m.n + fm.s[k].n_far) for k in range(ssd.MAX_STEPS)] == [int(c) for c in counts[1:]]
    assert int(fm.s[0].m.n + fm.s[0].n_far) == res.ground_n_in_quad
    assert sm.frame_tuple(fm)[2] == sm.pad(sm.moments_np(frame, labels, fm.n_surfaces), ssd.MAX_STEPS)
    floor = ssd.synth_host([gm.scene(ssd, "floor")])[0]
    res, labels, fm, fit = sm.oracle_planes(ssd, oracle, cfg, cal, floor)
    assert res.n_steps == 0 and bytes(fm) == bytes(C.sizeof(ssd.FrameMoments)) and bytes(fit) == bytes(C.sizeof(ssd.FrameSurfaces))
