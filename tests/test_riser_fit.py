"""The riser fit on the host (include/ssd_hip.h): the riser model of tests/riser_model.py against the oracle's own
riser evidence, the record layout, ssd_riser_fit_solve on hand-made moments (lean, skew, going, the statuses), the shared solve left as
it was, and the chain oracle -> riser labels -> sums -> planes on a staircase scene - judged here, on the host functions, because the
device is held to the host sums bit for bit (tests/test_gpu_riser_fit.py).  No GPU needed."""
import ctypes as C
import math

import numpy as np
import pytest

import ground_model as gm
import oracle_binding as ob
import riser_model as rm
import scenes
import surface_model as sm
from test_gpu_parity import SCENES

NAMES = ["ssd_set_riser_moments", "ssd_fetch_riser_moments", "ssd_riser_fit_solve", "ssd_process_host_riser_fits",
         "ssd_process_host_cameras_riser_fits"]


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("set_riser_moments", "fetch_riser_moments", "process_host_riser_fits", "process_host_cameras_riser_fits"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.riser_fit_solve)
    assert C.sizeof(ssd.RiserFit) == 24 + 8 * 13 and C.sizeof(ssd.FrameRiserFits) == 8 + ssd.MAX_RISERS * C.sizeof(ssd.RiserFit)
    assert ssd.MAX_RISERS == ssd.MAX_STEPS - 1 == len(ssd.FrameRisers().risers)


def test_null_arguments_are_rejected(ssd):
    L = ssd.lib()
    dummy = C.c_void_p(4096)
    fm, fr, cal, out = ssd.FrameMoments(), ssd.FrameRisers(), ssd.Calibration(), ssd.FrameRiserFits()
    for args in ((None, fr, cal, out), (fm, None, cal, out), (fm, fr, None, out), (fm, fr, cal, None)):
        a = [C.byref(v) if v is not None else None for v in args]
        assert L.ssd_riser_fit_solve(a[0], a[1], a[2], 1, a[3]) == -1
        assert b"null" in L.ssd_last_error()
    assert L.ssd_set_riser_moments(None, 1) == -1
    assert L.ssd_fetch_riser_moments(None, (ssd.FrameMoments * 1)(), 1, None) == -1
    res, ris, fits = (ssd.FrameResult * 1)(), (ssd.FrameRisers * 1)(), (ssd.FrameRiserFits * 1)()
    assert L.ssd_process_host_riser_fits(None, dummy, 1, 0, res, ris, None, 1, fits) == -1
    idx = (C.c_uint16 * 1)(0)
    assert L.ssd_process_host_cameras_riser_fits(None, dummy, 1, idx, 0, res, ris, None, 1, fits) == -1
    # the header must be the risers': n_surfaces outside 0 .. SSD_MAX_RISERS, or not n_risers
    fm.n_surfaces = ssd.MAX_RISERS + 1
    fr.n_risers = ssd.MAX_RISERS + 1
    with pytest.raises(ssd.SsdError, match="n_surfaces"):
        ssd.riser_fit_solve(fm, fr, cal, 1)
    fm.n_surfaces, fr.n_risers = 2, 3
    with pytest.raises(ssd.SsdError, match="n_surfaces"):
        ssd.riser_fit_solve(fm, fr, cal, 1)


# --------------------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("name", SCENES)
def test_the_model_reproduces_the_oracles_riser_evidence(ssd, oracle, name):
    """riser_labels on the oracle's record: per riser the count is the oracle's n_points, exactly, and the mean of s in 2^-40 m fixed
    point its mean_offset within 1e-12 m (parity.compare_risers' tolerance) - what validates the model before the GPU tests compare
    with it"""
    sc = scenes.make(ssd, name)
    trans = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(sc.width, sc.height, max_frames_per_batch=1)
    xyz = ssd.synth_host([sc])[0]
    ocfg, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants)
    rec = oracle.process(ocfg, ocal, xyz)[0]
    ora = oracle.risers(ocfg, ocal, xyz, rm.TOL, 200)
    labels, off = rm.evidence(cfg, trans.constants, rec, xyz, rm.TOL)
    assert int(labels.max(initial=0)) <= len(ora)
    got = rm.counts_and_offsets(labels, off, len(ora))
    for i, (o, (cnt, mean)) in enumerate(zip(ora, got)):
        assert cnt == o.n_points, (name, i, cnt, o.n_points)
        assert abs(mean - o.mean_offset) <= 1e-12, (name, i, mean, o.mean_offset)
    if name == "xga_config1":
        assert len(ora) == 3 and all(o.n_points >= 200 for o in ora), "the tests below are not vacuous"


# --------------------------------------------------------------------------- the record layout
def test_riser_moments_are_the_sums_over_the_riser_labels(ssd, oracle):
    """one 256 x 192 frame: ssd_surface_moments_host(frame, riser labels, n_risers, 0) = Python-integer sums over the labelled points"""
    sc = gm.scene(ssd, "steps")
    cfg = ssd.default_config(gm.W, gm.H)
    cal = ssd.transformation_for_scene(sc).constants
    frame = ssd.synth_host([sc])[0]
    ora, labels, fm, fit = rm.oracle_planes(ssd, oracle, cfg, cal, frame)
    assert len(ora) >= 2 and min(o.n_points for o in ora) >= rm.MIN_POINTS
    want = sm.moments_py(frame, labels, len(ora))
    assert sm.frame_tuple(fm) == (len(ora), 0, sm.pad(want, ssd.MAX_STEPS))
    assert [int(fm.s[i].m.n + fm.s[i].n_far) for i in range(len(ora))] == [o.n_points for o in ora]
    assert fit.n_risers == len(ora)
    floor = ssd.synth_host([gm.scene(ssd, "floor")])[0]
    ora, labels, fm, fit = rm.oracle_planes(ssd, oracle, cfg, cal, floor)
    assert ora == [] and not labels.any() and bytes(fm) == bytes(C.sizeof(ssd.FrameMoments)) and bytes(fit) == bytes(C.sizeof(ssd.FrameRiserFits))


# --------------------------------------------------------------------------- the solve on hand-made moments
def _calibration(ssd):
    """a camera 1 m above the floor looking along world y: world = (x, z, 1 - y); ToExternalWorld a quarter turn, a shift and 0.25 m"""
    cal = ssd.Calibration()
    cal.a[:] = [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.0]
    cal.b[:] = [0.0, 0.0, 1.0]
    cal.r2[:] = [0.0, -1.0, 1.0, 0.0]
    cal.t2[:] = [1.5, -2.5]
    cal.world_z = 0.25
    return cal


def _face(dist, back=0.0, nx=41, ny=17, x0=-0.5):
    """camera lattice points (multiples of 2^-10 m: exact in 2^-16 m fixed point) of a face of the staircase at world y = dist +
    back * world z: vertical for back = 0, leaning back (looking upward) by atan(back) otherwise"""
    x = x0 + np.arange(nx) / 1024.0 * 25.0
    y = 0.5 + np.arange(ny) / 1024.0 * 8.0                       # camera y = 1 - world z
    xx, yy = np.meshgrid(x, y)
    zz = dist + back * (1.0 - yy)
    p = np.stack([xx, yy, zz], axis=-1).reshape(-1, 3)
    assert np.all(p * 65536.0 == np.rint(p * 65536.0)), "exact lattice points"
    return p.astype(np.float32)


def _moments(ssd, faces):
    n = sum(len(p) for p in faces)
    cfg = ssd.default_config(n, 1)
    pts = np.concatenate(faces).reshape(1, n, 3)
    lab = np.concatenate([np.full(len(p), k + 1, dtype=np.uint8) for k, p in enumerate(faces)]).reshape(1, n)
    return ssd.surface_moments_host(cfg, pts, lab, len(faces), 0)


def _risers(ssd, cal, edges, heights):
    """FrameRisers with the drawn edges (left, right in camera-dependent world x / y, taken through ToExternalWorld) and heights"""
    fr = ssd.FrameRisers()
    fr.n_risers = len(edges)
    r2, t2 = np.array(list(cal.r2)).reshape(2, 2), np.array(list(cal.t2))
    for i, ((l, r), (zb, zt)) in enumerate(zip(edges, heights)):
        fr.risers[i].left[:] = list(r2 @ np.array(l) + t2)
        fr.risers[i].right[:] = list(r2 @ np.array(r) + t2)
        fr.risers[i].height_bottom, fr.risers[i].height_top = zb + cal.world_z, zt + cal.world_z
    return fr


def _zero_doubles(f):
    return list(f.normal) == [0.0] * 3 and list(f.centroid) == [0.0] * 3 and f.lean == 0.0 and f.skew == 0.0 and f.rms == 0.0 \
        and list(f.extent) == [0.0, 0.0] and f.going == 0.0


def test_lean_skew_and_going_of_known_faces(ssd):
    """exact lattice points, so the scatter is exact and the solve's only error is Jacobi's rounding: lean and skew to 1e-9 rad.  Faces:
    vertical at y = 2; vertical at y = 2.28125, shifted sideways (going 0.28125 whatever the shift); leaning back by atan(1/8) at
    y = 2.5625 + z / 8.  Drawn edges: parallel, rotated by 0.05 rad, parallel."""
    cal = _calibration(ssd)
    phi, back = 0.05, 0.125
    faces = [_face(2.0), _face(2.28125, x0=-0.25), _face(2.5625, back=back)]
    edges = [((-0.5, 2.0), (0.5, 2.0)), ((-0.5, 2.3), (-0.5 + math.cos(phi), 2.3 + math.sin(phi))), ((-0.5, 2.6), (0.5, 2.6))]
    heights = [(0.0, 0.17), (0.17, 0.34), (0.34, 0.51)]
    fit = ssd.riser_fit_solve(_moments(ssd, faces), _risers(ssd, cal, edges, heights), cal, 100)
    assert fit.n_risers == 3 and fit.reserved == 0
    r2 = np.array(list(cal.r2)).reshape(2, 2)
    want_h = r2 @ np.array([0.0, -1.0])                    # out of the face toward the camera: -y, through the quarter turn
    for i, f in enumerate(fit.r[:3]):
        assert f.status == ssd.GF_OK and f.n == len(faces[i]) and f.n_far == 0
        assert abs(np.linalg.norm(list(f.normal)) - 1.0) < 1e-12
        h = np.array(list(f.normal)[:2]) / np.linalg.norm(list(f.normal)[:2])
        assert np.max(np.abs(h - want_h)) < 1e-9, (i, h)
        assert abs(f.rise - 0.17) < 1e-15 and f.rms < 1e-7 and f.extent[0] >= f.extent[1] > 0.03
    assert abs(fit.r[0].lean) <= 1e-9 and abs(fit.r[1].lean) <= 1e-9
    assert abs(fit.r[2].lean - math.atan(back)) <= 1e-9 and fit.r[2].normal[2] > 0, "leaning back: the face looks upward"
    assert abs(fit.r[0].skew) <= 1e-9 and abs(fit.r[1].skew - phi) <= 1e-9 and abs(fit.r[2].skew) <= 1e-9
    # the centroid: the mean of the lattice points through CameraToWorld and ToExternalWorld
    c = faces[0].astype(np.float64).mean(axis=0)
    w = np.array([c[0], c[2], 1.0 - c[1]])
    want = list(r2 @ w[:2] + np.array(list(cal.t2))) + [w[2] + cal.world_z]
    assert np.max(np.abs(np.array(list(fit.r[0].centroid)) - want)) < 1e-12
    # going: the horizontal distance between consecutive faces along the first one's normal; the last riser has no next one
    assert abs(fit.r[0].going - 0.28125) <= 1e-9
    c1, c2 = faces[1].astype(np.float64).mean(axis=0), faces[2].astype(np.float64).mean(axis=0)
    assert abs(fit.r[1].going - (c2[2] - c1[2])) <= 1e-9 and fit.r[2].going == 0.0
    for i in range(3, ssd.MAX_RISERS):
        assert bytes(fit.r[i]) == bytes(C.sizeof(ssd.RiserFit))


def test_status_few_and_degenerate_and_going_without_a_neighbour(ssd):
    cal = _calibration(ssd)
    t = np.arange(300)[:, None] / 1024.0
    line = (np.array([0.0, 0.5, 2.2]) + t * np.array([1.0, 0.25, 0.5])).astype(np.float32)
    short = line[:50]
    faces = [_face(2.0), _face(2.28125, nx=9, ny=9), _face(2.5625), line, short]
    edges = [((-0.5, 2.0 + 0.28 * i), (0.5, 2.0 + 0.28 * i)) for i in range(5)]
    heights = [(0.17 * i, 0.17 * (i + 1)) for i in range(5)]
    fm, fr = _moments(ssd, faces), _risers(ssd, cal, edges, heights)
    fit = ssd.riser_fit_solve(fm, fr, cal, 100)
    # FEW comes first: the short line determines no plane either
    assert [fit.r[i].status for i in range(5)] == [ssd.GF_OK, ssd.GF_FEW, ssd.GF_OK, ssd.GF_DEGENERATE, ssd.GF_FEW]
    assert [int(fit.r[i].n) for i in range(5)] == [len(f) for f in faces]
    assert all(_zero_doubles(fit.r[i]) for i in (1, 3, 4)) and not _zero_doubles(fit.r[2])
    assert all(abs(fit.r[i].rise - 0.17) < 1e-15 for i in range(5)), "rise is set whatever the status"
    assert fit.r[0].going == 0.0 and fit.r[2].going == 0.0, "a neighbour that is FEW or DEGENERATE gives no going"
    fit = ssd.riser_fit_solve(fm, fr, cal, 50)
    assert [fit.r[i].status for i in range(5)] == [ssd.GF_OK, ssd.GF_OK, ssd.GF_OK, ssd.GF_DEGENERATE, ssd.GF_DEGENERATE]
    assert abs(fit.r[0].going - 0.28125) <= 1e-9 and abs(fit.r[1].going - 0.28125) <= 1e-9 and fit.r[2].going == 0.0
    empty = ssd.riser_fit_solve(_moments(ssd, [np.zeros((0, 3), dtype=np.float32), _face(2.0)]), _risers(ssd, cal, edges[:2], heights[:2]), cal, 0)
    assert empty.r[0].status == ssd.GF_FEW and empty.r[1].status == ssd.GF_OK, "no point at all is FEW whatever min_points"


# --------------------------------------------------------------------------- the shared solve is what it was
def test_the_ground_and_the_surface_solve_are_unchanged(ssd, oracle):
    """plane_of_moments is shared by three solves now.  On the moments of tests/ground_model.py and tests/surface_model.py: the ground
    fit's plane is numpy's word on the exact scatter (gm.eigh_of), the surface fit's normal is that plane through -A and r2 and its
    rms the same double, the records carry the moments untouched - and ssd_riser_fit_solve of the same moments returns the surface
    fit's normal, centroid, rms and extents byte for byte: one core, three readers."""
    sc = gm.scene(ssd, "steps")
    cfg = ssd.default_config(gm.W, gm.H)
    cal = ssd.transformation_for_scene(sc).constants
    frame = ssd.synth_host([sc])[0]
    a, r2 = np.array(list(cal.a)).reshape(3, 3), np.array(list(cal.r2)).reshape(2, 2)
    # ground_model's floor moments
    n, s, ss = gm.moments_np(cfg, cal, frame, 0.03)
    m = gm.moments_struct(ssd, n, s, ss)
    assert gm.moments_tuple(ssd.ground_moments_host(cfg, cal, frame, 0.03)) == (n, s, ss)
    g = ssd.ground_fit_solve(m, cal, gm.MIN_POINTS)
    lam, n0, dist = gm.eigh_of(n, s, ss)
    assert g.status == ssd.GF_OK and gm.moments_tuple(g.m) == (n, s, ss)
    assert gm.angle(list(g.normal), n0) < 1e-9 and abs(g.dist - dist) < 1e-12 and abs(g.rms - math.sqrt(lam[0])) < 1e-12
    # surface_model's per-surface moments
    res, labels, fm, fit = sm.oracle_planes(ssd, oracle, cfg, cal, frame)
    assert fit.n_surfaces >= 3
    fr = ssd.FrameRisers()
    fr.n_risers = fm.n_surfaces
    rf = ssd.riser_fit_solve(fm, fr, cal, sm.MIN_POINTS)
    for k in range(fit.n_surfaces):
        sf = fit.s[k]
        assert sf.status == ssd.GF_OK
        mk = gm.moments_tuple(fm.s[k].m)
        lam, n0, dist = gm.eigh_of(*mk)
        gk = ssd.ground_fit_solve(fm.s[k].m, cal, sm.MIN_POINTS)
        up = -(a @ np.array(list(gk.normal)))
        assert np.max(np.abs(np.array(list(sf.normal)) - (list(r2 @ up[:2]) + [up[2]]))) < 1e-15 and sf.rms == gk.rms
        assert gm.angle(list(gk.normal), n0) < 1e-9 and abs(sf.rms - math.sqrt(lam[0])) < 1e-12
        assert abs(sf.extent[0] - math.sqrt(lam[2])) < 1e-12 and abs(sf.extent[1] - math.sqrt(lam[1])) < 1e-12
        assert int(sf.n) == mk[0] and int(sf.n_far) == int(fm.s[k].n_far)
        r = rf.r[k]
        assert r.status == sf.status and bytes(r.normal) == bytes(sf.normal) and bytes(r.centroid) == bytes(sf.centroid)
        assert r.rms == sf.rms and bytes(r.extent) == bytes(sf.extent) and (r.n, r.n_far) == (sf.n, sf.n_far)
        assert abs(r.lean - (math.pi / 2 - sf.tilt)) < 1e-6, "a tread seen as a face looks straight up"


# --------------------------------------------------------------------------- accuracy
def test_the_oracles_risers_come_out_vertical_parallel_and_a_tread_apart(ssd, oracle):
    """the 3-step 256 x 192 scene of ground_model (cam_height 1.0, pitch 50 degrees), sigma 1 mm and 3 mm, under the true calibration:
    the scene's risers are vertical, parallel to the edges and one tread apart.  The bounds are three times each figure
    tools/riser_fit_accuracy.py recorded (profiles/riser_fit_accuracy.txt) - the margin is for other seeds, not for the code."""
    rec = rm.recorded_accuracy()
    assert 0 < rec["worst_lean_rad"] < 0.05 and 0 < rec["worst_skew_rad"] < 0.05 and 0 < rec["worst_going_error_m"] < 0.01
    for name, cfg, frame, cal, sc in rm.accuracy_cases(ssd):
        status, lean, skew, going, pairs, rows = rm.accuracy_of(ssd, oracle, cfg, frame, cal, sc)
        for row in rows:
            print("%s riser %d: status %d n %d lean %+.3e skew %.3e rms %.2e rise %.4f going %.4f" % ((name,) + row))
        assert sum(1 for s in status if s == ssd.GF_OK) >= 2, (name, status)
        assert pairs >= 1, "a going is measured"
        assert lean <= 3 * rec["worst_lean_rad"], (name, lean)
        assert skew <= 3 * rec["worst_skew_rad"], (name, skew)
        assert going <= 3 * rec["worst_going_error_m"], (name, going)
        for i, st, n, ln, sk, rms, rise, go in rows:
            assert abs(rise - sc.rise) < 0.005, "the rise is the difference of two fitted heights"
