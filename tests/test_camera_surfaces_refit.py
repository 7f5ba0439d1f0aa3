"""Trimmed refit of cameras batches and the drift watch on refit records (include/ssd_hip.h), CPU tier: the ABI,
ssd_camera_ground_gates value by value and refusal by refusal, and what folding refit records does to the drift per camera - judged on
the host functions over the oracle's labels, because the device is held to the host sums bit for bit
(tests/test_gpu_camera_surfaces_refit.py).  No GPU needed."""
import ctypes as C
import os
import re

import pytest

import camera_drift_model as cdm
import camera_refit_model as crm
import ground_model as gm
import surface_model as sm

NAMES = ["ssd_enqueue_cameras_surface_refit", "ssd_process_host_cameras_surfaces_refit", "ssd_camera_ground_gates"]
E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_cameras_surface_refit", "process_host_cameras_surfaces_refit"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.camera_ground_gates)
    text = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    assert all(re.search(r"\bint %s\(" % n, text) for n in NAMES)
    assert "Out of scope: camera batches" not in text


def test_null_handles_are_refused(ssd):
    L = ssd.lib()
    dummy = C.c_void_p(4096)
    idx = (C.c_uint16 * 1)(0)
    gates = (ssd.FrameGates * 1)()
    res, out = (ssd.FrameResult * 1)(), (ssd.FrameSurfaces * 1)()
    assert L.ssd_enqueue_cameras_surface_refit(None, dummy, 12 * 640 * 480, 1, None, ssd.INPUT_VERTICES, gates, dummy) == E_ARG
    assert b"null" in L.ssd_last_error()
    assert L.ssd_process_host_cameras_surfaces_refit(None, dummy, 1, idx, ssd.INPUT_VERTICES, res, None, None, 200, 2.5, 0.0, 1, out) == E_ARG
    assert L.ssd_last_error()


def _moments(ssd, ground=1, n_surfaces=2):
    fm = ssd.FrameMoments()
    fm.n_surfaces, fm.ground = n_surfaces, ground
    return fm


def _gates(ssd, n_surfaces, seed):
    """FrameGates with every one of the SSD_MAX_STEPS gates filled by something recognisable"""
    g = ssd.FrameGates()
    g.n_surfaces = n_surfaces
    for k in range(ssd.MAX_STEPS):
        g.g[k].n[:] = [0.25 * seed, -0.5 * (k + 1), 0.125]
        g.g[k].dist, g.g[k].gate = 1.0 + seed + k / 16.0, 0.001 * (k + 1)
    return g


def _drift(ssd, status, normal=(0.0, 0.0, 0.0), dist=0.0, rms=0.0):
    d = ssd.CameraDrift()
    d.fit.status = status
    d.fit.normal[:] = list(normal)
    d.fit.dist, d.fit.rms = dist, rms
    return d


def test_ground_gates_replace_exactly_the_ground_gates_of_frames_whose_cameras_fold_is_ok(ssd):
    drift = [_drift(ssd, ssd.GF_OK, (0.1, -0.7, 0.7), 1.0625, 0.0021), _drift(ssd, ssd.GF_FEW, (0.3, 0.3, 0.3), 2.0, 0.5),
             _drift(ssd, ssd.GF_OK, (-0.2, -0.6, 0.77), 0.96875, 0.0003), _drift(ssd, ssd.GF_DEGENERATE, (1.0, 0.0, 0.0), 3.0, 0.1)]
    #          camera, ground, n_surfaces of the moments, n_surfaces of the gates given
    frames = [(0, 1, 3, 3), (0, 0, 3, 3), (1, 1, 3, 3), (2, 1, 2, 0), (0, 1, 0, 2), (3, 1, 2, 2), (2, 1, 1, 4), (2, 0, 0, 0)]
    moments = [_moments(ssd, g, ns) for _, g, ns, _ in frames]
    cam_of = [c for c, _, _, _ in frames]
    given = [_gates(ssd, gn, i) for i, (_, _, _, gn) in enumerate(frames)]
    for k_sigma, gate_min in ((2.5, 0.0), (2.0, 0.002)):
        got = ssd.camera_ground_gates(moments, cam_of, drift, given, k_sigma=k_sigma, gate_min=gate_min)
        for i, (c, ground, ns, gn) in enumerate(frames):
            fit = drift[c].fit
            if ground == 1 and ns >= 1 and fit.status == ssd.GF_OK:
                g = got[i].g[0]
                assert list(g.n) == list(fit.normal) and g.dist == fit.dist, i
                assert g.gate == max(k_sigma * fit.rms, gate_min), (i, "bit for bit: one product, one comparison")
                assert got[i].n_surfaces == max(gn, 1), i
                assert bytes(got[i])[8 + C.sizeof(ssd.PlaneGate):] == bytes(given[i])[8 + C.sizeof(ssd.PlaneGate):], "the treads' gates are left alone"
            else:
                assert bytes(got[i]) == bytes(given[i]), (i, "no ground, no surface, or a fold that is not OK: as given")
        assert [i for i in range(len(frames)) if bytes(got[i]) != bytes(given[i])] == [0, 3, 6]
        assert got[3].n_surfaces == 1 and given[3].n_surfaces == 0, "raised from 0 to 1"
        assert got[0].g[0].gate == (0.0021 * 2.5 if gate_min == 0.0 else 2.0 * 0.0021) and got[6].g[0].gate == (0.0003 * 2.5 if gate_min == 0.0 else 0.002)
    assert ssd.camera_ground_gates([], [], drift, []) == []


def test_ground_gates_refuse_bad_arguments_and_leave_the_gates_untouched(ssd):
    L = ssd.lib()
    n = 3
    mom = (ssd.FrameMoments * n)(*[_moments(ssd) for _ in range(n)])
    drift = (ssd.CameraDrift * 2)(_drift(ssd, ssd.GF_OK, (0.0, 0.0, 1.0), 1.0, 0.002), _drift(ssd, ssd.GF_OK, (0.0, 0.0, 1.0), 1.5, 0.002))
    gates = (ssd.FrameGates * n)(*[_gates(ssd, 2, i) for i in range(n)])
    before = bytes(gates)
    idx = (C.c_uint16 * n)(0, 1, 0)
    bad_idx = (C.c_uint16 * n)(0, 1, 2)
    nan = float("nan")
    for args in ((None, idx, n, drift, 2, 2.5, 0.0, gates), (mom, None, n, drift, 2, 2.5, 0.0, gates), (mom, idx, n, None, 2, 2.5, 0.0, gates),
                 (mom, idx, n, drift, 2, 2.5, 0.0, None), (mom, idx, n, drift, 0, 2.5, 0.0, gates), (mom, idx, n, drift, -1, 2.5, 0.0, gates),
                 (mom, idx, n, drift, ssd.MAX_CAMERAS + 1, 2.5, 0.0, gates), (mom, idx, -1, drift, 2, 2.5, 0.0, gates),
                 (mom, bad_idx, n, drift, 2, 2.5, 0.0, gates), (mom, idx, n, drift, 2, 0.0, 0.0, gates), (mom, idx, n, drift, 2, -1.0, 0.0, gates),
                 (mom, idx, n, drift, 2, 16.5, 0.0, gates), (mom, idx, n, drift, 2, nan, 0.0, gates), (mom, idx, n, drift, 2, 2.5, -0.001, gates),
                 (mom, idx, n, drift, 2, 2.5, 1.5, gates), (mom, idx, n, drift, 2, 2.5, nan, gates)):
        assert L.ssd_camera_ground_gates(*args) == E_ARG, args[2:7]
        assert L.ssd_last_error() and bytes(gates) == before, args[2:7]
    assert L.ssd_camera_ground_gates(mom, bad_idx, n, drift, 2, 2.5, 0.0, gates) == E_ARG and b"names camera 2 of 2" in L.ssd_last_error()
    assert L.ssd_camera_ground_gates(mom, idx, n, drift, 2, 16.0, 1.0, gates) == 0, "the ends of both ranges are inside"
    assert bytes(gates) != before and gates[1].g[0].dist == 1.5 and gates[0].g[0].gate == 1.0
    with pytest.raises(ssd.SsdError, match="camera_of_frame"):
        ssd.camera_ground_gates(list(mom), [0], list(drift), list(gates))
    with pytest.raises(ssd.SsdError, match="one FrameGates per frame"):
        ssd.camera_ground_gates(list(mom), [0, 1, 0], list(drift), list(gates)[:2])


@pytest.fixture(scope="module")
def camera(ssd, oracle):
    """the frames of the camera whose table entry is pitched by a degree and 2 cm low (tests/camera_drift_model.py), once"""
    return crm.camera_frames(ssd, oracle, cdm.ENTRIES[1][1])


def test_a_frame_whose_own_ground_fit_is_few_still_gives_its_floor_points(ssd, camera):
    """min_points above a frame's floor points: its own ground fit is FEW, its own gate all zero, its refit record's ground empty - and
    with the camera's fold (OK at its own min_points: four frames' points) its ground gate is usable and the record holds points"""
    truth, entry, cfg, frames = camera
    first = [fm for _, _, fm in frames]
    idx = [0] * len(frames)
    many = max(int(fm.s[0].m.n) for fm in first) + 1
    own = [ssd.surface_gates_from_moments(fm, many, 2.5, 0.0) for fm in first]
    assert all(ssd.surface_fit_solve(fm, entry, many).s[0].status == ssd.GF_FEW and g.g[0].gate == 0.0 for fm, g in zip(first, own))
    drift = ssd.camera_drift_fold(first, idx, [entry], min_points=many)
    assert drift[0].fit.status == ssd.GF_OK and drift[0].m.n >= many
    shared = ssd.camera_ground_gates(first, idx, drift, own, 2.5, 0.0)
    for (frame, lab, fm), g0, g1 in zip(frames, own, shared):
        alone = ssd.surface_refit_moments_host(cfg, frame, lab, g0, fm.n_surfaces, fm.ground)
        helped = ssd.surface_refit_moments_host(cfg, frame, lab, g1, fm.n_surfaces, fm.ground)
        assert alone.s[0].m.n == 0 and 0 < helped.s[0].m.n <= fm.s[0].m.n
        assert g1.g[0].gate == 2.5 * drift[0].fit.rms > 0.0 and list(g1.g[0].n) == list(drift[0].fit.normal)
    refit = [ssd.surface_refit_moments_host(cfg, f, lab, g, fm.n_surfaces, fm.ground) for (f, lab, fm), g in zip(frames, shared)]
    again = ssd.camera_drift_fold(refit, idx, [entry], min_points=many)[0]
    assert again.fit.status == ssd.GF_OK and again.frames_ground == len(frames), "and so the next fold has them"


def test_folding_refit_records_is_exact_order_independent_and_obeys_the_overflow_rule(ssd, camera):
    truth, entry, cfg, frames = camera
    refit = crm.refit_records(ssd, cfg, entry, frames, 2.5, 1, True)
    idx = [0] * len(refit)
    got = ssd.camera_drift_fold(refit, idx, [entry], min_points=cdm.MIN_POINTS)
    assert [cdm.drift_tuple(d) for d in got] == cdm.fold_py(refit, idx, 1) and got[0].frames_ground == len(refit)
    other = ssd.camera_drift_fold(refit[::-1], idx, [entry], min_points=cdm.MIN_POINTS)
    assert bytes(other[0]) == bytes(got[0]), "byte for byte, the fit included"
    huge = ssd.FrameMoments.from_buffer_copy(refit[0])
    huge.s[0].m.ss[5] = (1 << 63) - 1 - refit[1].s[0].m.ss[5] + 1          # one more than what still fits beside frame 1
    mixed = [refit[1], huge, refit[2]]
    left = ssd.camera_drift_fold(mixed, [0, 0, 0], [entry], min_points=cdm.MIN_POINTS)[0]
    assert cdm.drift_tuple(left) == cdm.fold_py(mixed, [0, 0, 0], 1)[0]
    assert (left.frames, left.frames_ground, left.frames_left) == (3, 2, 1) and left.m.n == refit[1].s[0].m.n + refit[2].s[0].m.n


# ---- accuracy -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def accuracy(ssd, oracle):
    return crm.accuracy_rows(ssd, oracle)


def test_the_first_column_reproduces_the_drift_folds_recorded_figures(accuracy):
    """the yardstick: the fold of the first-pass records is profiles/camera_drift_accuracy.txt's (3.2 mrad, 1.2 mm worst)"""
    worst = crm.worst_columns(accuracy)
    rec = cdm.recorded_accuracy()
    assert abs(worst["first"][0] - rec["worst_tilt_error_rad"]) <= 5e-7 and abs(worst["first"][1] - rec["worst_height_error_m"]) <= 5e-7


def test_no_refit_fold_is_worse_than_the_first_pass_fold_and_none_beyond_three_times_its_record(accuracy):
    """every column tools/camera_drift_refit_accuracy.py records - one and two refit passes at 2.5 and 2.0 rms, per-frame gates and the
    camera's folded plane in front of the last pass: the worst tilt and height errors over the entries against the first-pass fold's
    worst of the SAME run, and against three times the recorded figures (the margin this project gives every accuracy figure)"""
    worst = crm.worst_columns(accuracy)
    rec = crm.recorded_accuracy()
    for c in crm.COLUMNS:
        kt, kh = "worst_tilt_error_rad_" + crm.column_key(c), "worst_height_error_m_" + crm.column_key(c)
        print("%s = %.3e (recorded %.3e), %s = %.3e (recorded %.3e)" % (kt, worst[c][0], rec[kt], kh, worst[c][1], rec[kh]))
        assert all(r[c][3] == 0 for _, r in accuracy), "every fold is OK"
        assert 0 < rec[kt] < 0.01 and 0 < rec[kh] < 0.005 and worst[c][0] <= 3 * rec[kt] and worst[c][1] <= 3 * rec[kh], c
        if c != "first":
            assert worst[c][0] <= worst["first"][0] and worst[c][1] <= worst["first"][1], c


def test_the_folds_keep_nine_tenths_of_their_ground_points_at_2p5_rms(accuracy):
    """Section 7g's condition, through the fold as tests/test_surface_refit.py takes it for its own drift fold: the refit fold's ground
    points against the first-pass fold's, for every 2.5 rms column.  With per-frame gates the same holds frame by frame (section 7g's
    own granularity).  With the camera's gate it does NOT hold frame by frame, and that is recorded, not asserted: one plane and one
    width for frames of 1 to 3 mm of noise trims the noisiest frame hardest - 0.925 of its ground points after one pass, 0.894 after
    two (profiles/camera_drift_refit_accuracy.txt, least_frame_kept_share_*) - while the fold keeps 0.958."""
    worst = crm.worst_columns(accuracy)
    for c in crm.COLUMNS[1:]:
        print("%s: the fold keeps %.4f, the least of a frame %.4f" % (crm.column_key(c), worst[c][2], worst[c][3]))
        if c[0] == 2.5:
            assert worst[c][2] >= 0.9, c
            if not c[2]:
                assert worst[c][3] >= 0.9, c
