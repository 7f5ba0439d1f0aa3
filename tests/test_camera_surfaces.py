"""Surface fit of cameras batches and drift per camera (include/ssd_hip.h), CPU tier: the ABI, the fold against
Python integers, its overflow rule, empty and bad input, and that a camera whose table entry is off by a degree and two centimetres
is told so - judged on the host functions over the oracle's labels, because the device is held to the host sums bit for bit
(tests/test_gpu_camera_surfaces.py).  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import camera_drift_model as cdm
import ground_model as gm
import surface_model as sm

NAMES = ["ssd_enqueue_cameras_surface_moments", "ssd_process_host_cameras_surfaces", "ssd_camera_drift_fold"]
E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_cameras_surface_moments", "process_host_cameras_surfaces", "camera_drift"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.camera_drift_fold)
    text = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    assert all(re.search(r"\bint %s\(" % n, text) for n in NAMES)
    assert "out of scope" not in text


def test_struct_sizes_as_a_c_compiler_sees_them(ssd, tmp_path):
    src = tmp_path / "sizeof_drift.c"
    src.write_text('#include "ssd_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void)\n{\n'
                   '  printf("%d %d %d %d %d %d\\n", (int)sizeof(ssd_camera_drift), (int)offsetof(ssd_camera_drift, m), (int)offsetof(ssd_camera_drift, n_far),\n'
                   '         (int)offsetof(ssd_camera_drift, fit), (int)sizeof(ssd_ground_fit), (int)sizeof(ssd_frame_moments));\n  return 0;\n}\n')
    exe = tmp_path / "sizeof_drift"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = ssd.CameraDrift
    assert out == [C.sizeof(D), D.m.offset, D.n_far.offset, D.fit.offset, C.sizeof(ssd.GroundFit), C.sizeof(ssd.FrameMoments)]
    assert C.sizeof(D) == 16 + 80 + 8 + C.sizeof(ssd.GroundFit)


def test_null_handles_and_pointers_are_refused(ssd):
    L = ssd.lib()
    dummy = C.c_void_p(4096)
    idx = (C.c_uint16 * 1)(0)
    res, out = (ssd.FrameResult * 1)(), (ssd.FrameSurfaces * 1)()
    assert L.ssd_enqueue_cameras_surface_moments(None, dummy, 12 * 640 * 480, 1, None, idx, ssd.INPUT_VERTICES, dummy) == E_ARG
    assert b"null" in L.ssd_last_error()
    assert L.ssd_process_host_cameras_surfaces(None, dummy, 1, idx, ssd.INPUT_VERTICES, res, None, 1, out) == E_ARG
    assert L.ssd_last_error()


def _record(ssd, ground_sums=None, n_far=0, ground=1, n_surfaces=2, other=5):
    """a hand-made FrameMoments: surface 0 = the ten sums given, surface 1 = something that must never be folded"""
    fm = ssd.FrameMoments()
    fm.n_surfaces, fm.ground = n_surfaces, ground
    if ground_sums is not None:
        fm.s[0].m.n = ground_sums[0]
        fm.s[0].m.s[:] = ground_sums[1:4]
        fm.s[0].m.ss[:] = ground_sums[4:10]
        fm.s[0].n_far = n_far
    fm.s[1].m.n = other
    fm.s[1].m.ss[0] = other * 1000
    return fm


def _cams(ssd, n):
    return [ssd.transformation_for_scene(gm.scene(ssd, "floor", pitch_deg=40.0 + i)).constants for i in range(n)]


@pytest.fixture(scope="module")
def scene_records(ssd, oracle):
    """FrameMoments of 256 x 192 scenes through ssd_surface_moments_host on the oracle's labels, once: six staircases of one pose (a camera's
    frames: their floor is one plane), a bare floor (n_surfaces = 0: all zero), and records with ground = 0 and with the header alone (what SSD_ST_THROW leaves)"""
    cfg = ssd.default_config(gm.W, gm.H)
    recs = []
    for i in range(6):
        sc = gm.scene(ssd, "steps" if i % 2 == 0 else "outliers", seed=20 + i, sigma=0.001 + 0.0004 * i)
        fm = sm.oracle_planes(ssd, oracle, cfg, ssd.transformation_for_scene(sc).constants, ssd.synth_host([sc])[0])[2]
        assert fm.ground == 1 and fm.n_surfaces >= 2 and fm.s[0].m.n > 1000
        recs.append(fm)
    floor = gm.scene(ssd, "floor")
    bare = sm.oracle_planes(ssd, oracle, cfg, ssd.transformation_for_scene(floor).constants, ssd.synth_host([floor])[0])[2]
    assert bytes(bare) == bytes(C.sizeof(ssd.FrameMoments))
    no_ground = ssd.FrameMoments.from_buffer_copy(recs[0])
    no_ground.ground = 0
    no_surface = ssd.FrameMoments.from_buffer_copy(recs[1])
    no_surface.n_surfaces = 0
    return recs, [bare, no_ground, no_surface, ssd.FrameMoments()]


def test_the_fold_is_exact_and_independent_of_the_frame_order(ssd, scene_records):
    recs, skipped = scene_records
    moments = [recs[0], skipped[0], recs[1], recs[2], skipped[1], recs[3], skipped[2], recs[4], recs[5], skipped[3]]
    cam_of = [0, 0, 1, 0, 1, 1, 2, 2, 0, 2]
    cams = _cams(ssd, 4)                                       # camera 3: nobody names it
    want = cdm.fold_py(moments, cam_of, 4)
    assert [w[:3] for w in want] == [(4, 3, 0), (3, 2, 0), (3, 1, 0), (0, 0, 0)], "frames, folded, left per camera"
    got = ssd.camera_drift_fold(moments, cam_of, cams, min_points=1000)
    assert [cdm.drift_tuple(d) for d in got] == want and [d.camera for d in got] == [0, 1, 2, 3]
    for order in (list(reversed(range(10))), [3, 9, 0, 5, 2, 7, 4, 1, 8, 6]):
        other = ssd.camera_drift_fold([moments[i] for i in order], [cam_of[i] for i in order], cams, min_points=1000)
        assert [bytes(d) for d in other] == [bytes(d) for d in got], "byte for byte, the fit included"
    # the fit is the existing solve on the folded sums against the camera's own entry
    for d, cal in zip(got, cams):
        assert bytes(d.fit) == bytes(ssd.ground_fit_solve(d.m, cal, 1000))
        assert bytes(d.fit.m) == bytes(d.m)
    assert [d.fit.status for d in got] == [ssd.GF_OK, ssd.GF_OK, ssd.GF_OK, ssd.GF_FEW]
    assert got[3].frames == 0 and got[3].m.n == 0


def test_a_frame_that_would_overflow_is_left_whole(ssd):
    big = 1 << 62
    a = [1000, 5, -6, 7, big - 10, 11, 12, 13, 14, 15]
    b = [2000, -50, 60, 70, 5, 21, -22, 23, 24, big - 1]
    c = [3000, 1, 1, 1, 100, 1, 1, 1, 1, 1]                    # 2^62 - 10 + 5 + 100 fits; ss[5] = 2^62 - 1 + 15 + 1 = 2^62 + 15 fits too
    c[9] = big                                                  # ... but 2^62 - 1 + 15 + 2^62 does not
    small = [10, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    moments = [_record(ssd, a, n_far=1), _record(ssd, b, n_far=2), _record(ssd, c, n_far=4), _record(ssd, small, n_far=8)]
    got = ssd.camera_drift_fold(moments, [0, 0, 0, 0], _cams(ssd, 1), min_points=1)[0]
    assert cdm.drift_tuple(got) == cdm.fold_py(moments, [0, 0, 0, 0], 1)[0]
    assert (got.frames, got.frames_ground, got.frames_left) == (4, 3, 1)
    want = [x + y + z for x, y, z in zip(a, b, small)]
    assert cdm.drift_tuple(got)[3] == want + [11], "the sums of frames 0, 1 and 3: nothing of frame 2, nothing wrapped"
    assert got.m.ss[5] == big + 15 + 9 - 1 and got.m.ss[0] == big - 10 + 5 + 4
    # n_far alone overflowing leaves the frame out as well; negative sums too
    far = _record(ssd, small, n_far=(1 << 63) - 1)
    neg = [5, -(1 << 62), 0, 0, 1, 1, 1, 1, 1, 1]
    moments = [far, _record(ssd, small, n_far=1), _record(ssd, neg), _record(ssd, neg), _record(ssd, [5, -1, 0, 0, 1, 1, 1, 1, 1, 1])]
    got = ssd.camera_drift_fold(moments, [1, 1, 0, 0, 0], _cams(ssd, 2), min_points=1)
    assert [cdm.drift_tuple(d) for d in got] == cdm.fold_py(moments, [1, 1, 0, 0, 0], 2)
    assert (got[1].frames_ground, got[1].frames_left, got[1].n_far, got[1].m.n) == (1, 1, (1 << 63) - 1, 10)
    assert (got[0].frames_ground, got[0].frames_left, got[0].m.s[0]) == (2, 1, -(1 << 63)), "-2^63 itself fits; one less does not"


def test_empty_and_bad_input(ssd):
    L = ssd.lib()
    cams = _cams(ssd, 2)
    got = ssd.camera_drift_fold([_record(ssd, [10] * 10)], [1], cams, min_points=1)
    assert got[0].frames == 0 and got[0].fit.status == ssd.GF_FEW and bytes(got[0].m) == bytes(80)
    assert bytes(got[0].fit.cal) == bytes(cams[0]), "a fit that is not OK carries the entry unchanged"
    assert got[1].frames == 1 and got[1].frames_ground == 1
    none = ssd.camera_drift_fold([], [], cams)
    assert [(d.camera, d.frames, d.fit.status) for d in none] == [(0, 0, ssd.GF_FEW), (1, 0, ssd.GF_FEW)]
    arr = (ssd.Camera * 2)()
    for i, c in enumerate(cams):
        arr[i].cal = c
    mom = (ssd.FrameMoments * 2)(_record(ssd, [10] * 10), _record(ssd, [10] * 10))
    idx = (C.c_uint16 * 2)(0, 2)
    out = (ssd.CameraDrift * 2)()
    C.memset(out, 0xA5, C.sizeof(out))
    before = bytes(out)
    assert L.ssd_camera_drift_fold(mom, idx, 2, arr, 2, 1, out) == E_ARG
    assert b"names camera 2 of 2" in L.ssd_last_error() and bytes(out) == before
    idx[1] = 1
    for args in ((None, idx, 2, arr, 2, 1, out), (mom, None, 2, arr, 2, 1, out), (mom, idx, 2, None, 2, 1, out), (mom, idx, 2, arr, 2, 1, None),
                 (mom, idx, 2, arr, 0, 1, out), (mom, idx, 2, arr, -1, 1, out), (mom, idx, 2, arr, ssd.MAX_CAMERAS + 1, 1, out), (mom, idx, -1, arr, 2, 1, out)):
        assert L.ssd_camera_drift_fold(*args) == E_ARG, args[2:6]
        assert L.ssd_last_error() and bytes(out) == before
    assert L.ssd_camera_drift_fold(mom, idx, 2, arr, 2, 1, out) == 0 and out[0].frames == 1 and out[1].frames == 1
    with pytest.raises(ssd.SsdError, match="camera_of_frame"):
        ssd.camera_drift_fold(list(mom), [0], cams)


def test_drift_of_a_camera_is_found(ssd, oracle):
    """Two cameras, four frames each (other seeds, 1 - 3 mm of noise) of the 3-step 256 x 192 scene.  Camera 0's table entry is the
    true pose, camera 1's the true pose pitched by 1 degree and lowered by 2 cm; detection (the oracle) runs under the table's entries.
    fit.tilt and fit.height_delta against what the scene generator's pose says they are: within three times the worst figures
    tools/camera_drift_accuracy.py recorded over its entries (profiles/camera_drift_accuracy.txt; the margin is for other seeds - the
    ground's points reach the first riser's foot, as in tests/test_surface_fit.py), and a folded fit no worse than the worst of its
    frames alone."""
    rec = cdm.recorded_accuracy()
    assert 0 < rec["worst_tilt_error_rad"] < 0.01 and 0 < rec["worst_height_error_m"] < 0.005
    cases = [cdm.camera_case(ssd, oracle, cdm.ENTRIES[k][1]) for k in (0, 1)]
    n = len(cdm.FRAMES)
    moments = [cases[k][2][i] for i in range(n) for k in (0, 1)]        # interleaved: frame 2 i of camera 0, 2 i + 1 of camera 1
    cam_of = [0, 1] * n
    table = [cases[0][1], cases[1][1]]
    assert bytes(cases[0][0]) == bytes(cases[1][0]) == bytes(table[0]) != bytes(table[1])
    drift = ssd.camera_drift_fold(moments, cam_of, table, min_points=cdm.MIN_POINTS)
    want_tilt = [0.0, gm.angle(gm.plane_of(cases[1][0])[0], gm.plane_of(table[1])[0])]
    assert abs(want_tilt[1] - np.radians(1.0)) < 1e-6
    for k, d in enumerate(drift):
        truth, entry, own = cases[k]
        assert (d.frames, d.frames_ground, d.frames_left, d.fit.status) == (n, n, 0, ssd.GF_OK)
        et, eh, ea = cdm.drift_errors(d.fit, truth, entry)
        print("camera %d: tilt %.4e (want %.4e), height_delta %+.4e; errors %.3e rad, %.3e m, normal %.3e rad"
              % (k, d.fit.tilt, want_tilt[k], d.fit.height_delta, et, eh, ea))
        assert et <= 3 * rec["worst_tilt_error_rad"] and eh <= 3 * rec["worst_height_error_m"], (k, et, eh)
        single = [cdm.drift_errors(ssd.camera_drift_fold([m], [0], [entry], min_points=cdm.MIN_POINTS)[0].fit, truth, entry) for m in own]
        print("camera %d alone: %s" % (k, ", ".join("%.3e rad %.3e m" % (s[2], s[1]) for s in single)))
        assert ea <= max(s[2] for s in single) and eh <= max(s[1] for s in single), (k, ea, eh, single)
    # camera 1 reads its degree and its two centimetres, camera 0 reads nothing: within the same error
    assert abs(drift[1].fit.tilt - np.radians(1.0)) <= 3 * rec["worst_tilt_error_rad"]
    assert abs(drift[1].fit.height_delta - 0.02) <= 3 * rec["worst_height_error_m"]
    assert drift[0].fit.tilt <= 3 * rec["worst_tilt_error_rad"] and abs(drift[0].fit.height_delta) <= 3 * rec["worst_height_error_m"]
    # the refined entry is the true pose to the same error
    assert gm.errors(drift[1].fit, cases[1][0])[0] <= 3 * rec["worst_tilt_error_rad"]
    assert gm.angle(gm.plane_of(drift[1].fit.cal)[0], gm.plane_of(cases[1][0])[0]) <= 3 * rec["worst_tilt_error_rad"]
