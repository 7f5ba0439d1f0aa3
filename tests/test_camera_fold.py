"""Camera fold on the device (include/ssd_hip.h), CPU tier: the ABI and the record, ssd_camera_drift_from_fold
against ssd_camera_drift_fold byte for byte, its refusals, and the fold's rule - moved to csrc/ssd_fold.h for the device to share -
against Python integers on the overflow records, a mixed-sign prefix among them.  The device is held to these host functions byte for
byte in tests/test_gpu_camera_fold.py.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

import camera_drift_model as cdm
import ground_model as gm

NAMES = ["ssd_enqueue_camera_fold", "ssd_enqueue_camera_ground_gates", "ssd_enqueue_cameras_surface_refit_folded", "ssd_camera_drift_from_fold",
         "ssd_process_host_cameras_drift"]
E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 62
SMALL = [10, 1, 2, 3, 4, 5, 6, 7, 8, 9]


def record(ssd, ground_sums=None, n_far=0, ground=1, n_surfaces=2, other=5):
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


def cams(ssd, n):
    return [ssd.transformation_for_scene(gm.scene(ssd, "floor", pitch_deg=40.0 + i)).constants for i in range(n)]


def overflow_cases(ssd):
    """[(name, records, camera_of_frame, ncams, (frames, folded, left) per camera)]: the crafted records of tests/test_camera_surfaces.py - a
    frame left and a later, smaller one taken; n_far at INT64_MAX; -2^63 fits and one less does not - and a mixed-sign triple whose total
    fits while its prefix does not"""
    a = [1000, 5, -6, 7, BIG - 10, 11, 12, 13, 14, 15]
    b = [2000, -50, 60, 70, 5, 21, -22, 23, 24, BIG - 1]
    c = [3000, 1, 1, 1, 100, 1, 1, 1, 1, BIG]
    neg = [5, -BIG, 0, 0, 1, 1, 1, 1, 1, 1]
    far = record(ssd, SMALL, n_far=(1 << 63) - 1)
    up = [7, 0, 0, 0, 1, 1, 1, 1, 1, BIG]
    down = [7, 0, 0, 0, 1, 1, 1, 1, 1, -BIG]
    return [
        ("left-then-smaller", [record(ssd, a, n_far=1), record(ssd, b, n_far=2), record(ssd, c, n_far=4), record(ssd, SMALL, n_far=8)], [0, 0, 0, 0], 1,
         [(4, 3, 1)]),
        ("n_far-and-negative", [far, record(ssd, SMALL, n_far=1), record(ssd, neg), record(ssd, neg), record(ssd, [5, -1, 0, 0, 1, 1, 1, 1, 1, 1])],
         [1, 1, 0, 0, 0], 2, [(3, 2, 1), (2, 1, 1)]),
        # +2^62, +2^62, -2^62: the sum is 2^62, the second prefix 2^63 - the second frame is left and the third taken
        ("mixed-sign", [record(ssd, up), record(ssd, up), record(ssd, down)], [0, 0, 0], 1, [(3, 2, 1)]),
    ]


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n), n
    for m in ("enqueue_camera_fold", "enqueue_camera_ground_gates", "enqueue_cameras_surface_refit_folded", "camera_drift_resident", "camera_drift"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.camera_drift_from_fold)
    text = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    assert all(re.search(r"\bint %s\(" % n, text) for n in NAMES)
    assert "stays on the host (it needs the fold)" not in text
    assert "stays on the host (it needs the fold)" not in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_the_record_is_the_head_of_the_drift_record(ssd, tmp_path):
    src = tmp_path / "sizeof_fold.c"
    fields = ["camera", "frames", "frames_ground", "frames_left", "m", "n_far"]
    src.write_text('#include "ssd_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void)\n{\n  printf("%d", (int)sizeof(ssd_camera_fold));\n'
                   + "".join('  printf(" %%d %%d", (int)offsetof(ssd_camera_fold, %s), (int)offsetof(ssd_camera_drift, %s));\n' % (f, f) for f in fields)
                   + '  printf(" %d\\n", (int)offsetof(ssd_camera_drift, fit));\n  return 0;\n}\n')
    exe = tmp_path / "sizeof_fold"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == 104 == C.sizeof(ssd.CameraFold) and out[-1] == 104
    for k, f in enumerate(fields):
        assert out[1 + 2 * k] == out[2 + 2 * k] == getattr(ssd.CameraFold, f).offset == getattr(ssd.CameraDrift, f).offset, f


def heads(ssd, drift):
    return [ssd.CameraFold.from_buffer_copy(bytes(d)[:104]) for d in drift]


def test_drift_from_fold_is_the_fold_byte_for_byte(ssd, oracle):
    # camera_drift_model's cameras: a true entry and one a degree and two centimetres off, their frames interleaved, one camera nobody names
    cases = [cdm.camera_case(ssd, oracle, cdm.ENTRIES[k][1]) for k in (0, 1)]
    n = len(cdm.FRAMES)
    moments = [cases[k][2][i] for i in range(n) for k in (0, 1)]
    table = [cases[0][1], cases[1][1], cams(ssd, 1)[0]]
    want = ssd.camera_drift_fold(moments, [0, 1] * n, table, min_points=cdm.MIN_POINTS)
    assert [d.fit.status for d in want] == [ssd.GF_OK, ssd.GF_OK, ssd.GF_FEW] and want[1].fit.tilt > 0.01
    got = ssd.camera_drift_from_fold(heads(ssd, want), table, min_points=cdm.MIN_POINTS)
    assert [bytes(g) for g in got] == [bytes(w) for w in want]
    assert [bytes(g) for g in ssd.camera_drift_from_fold(heads(ssd, want), table, min_points=1 << 30)] != [bytes(w) for w in want], "min_points is used"
    # the crafted overflow records
    for name, recs, idx, ncams, counts in overflow_cases(ssd):
        table = cams(ssd, ncams)
        want = ssd.camera_drift_fold(recs, idx, table, min_points=1)
        assert [(d.frames, d.frames_ground, d.frames_left) for d in want] == counts, name
        got = ssd.camera_drift_from_fold(heads(ssd, want), table, min_points=1)
        assert [bytes(g) for g in got] == [bytes(w) for w in want], name


def test_the_moved_rule_against_python_integers(ssd):
    for name, recs, idx, ncams, counts in overflow_cases(ssd):
        got = ssd.camera_drift_fold(recs, idx, cams(ssd, ncams), min_points=1)
        want = cdm.fold_py(recs, idx, ncams)
        assert [cdm.drift_tuple(d) for d in got] == want, name
        assert [w[:3] for w in want] == counts, name
    mixed = ssd.camera_drift_fold(*overflow_cases(ssd)[2][1:3], cams(ssd, 1), min_points=1)[0]
    assert mixed.m.ss[5] == 0 and mixed.m.n == 14 and mixed.m.ss[0] == 2, "frames 0 and 2: +2^62 - 2^62; nothing of frame 1"
    lo = ssd.camera_drift_fold(*overflow_cases(ssd)[1][1:3], cams(ssd, 2), min_points=1)[0]
    assert lo.m.s[0] == -(1 << 63), "-2^63 itself fits"
    # frames without a ground, without a surface: counted, never read
    junk = record(ssd, [BIG] * 10, n_far=BIG, ground=0)
    none = record(ssd, [BIG] * 10, n_far=BIG, n_surfaces=0)
    got = ssd.camera_drift_fold([junk, record(ssd, [BIG] * 10), none, junk], [0] * 4, cams(ssd, 1), min_points=1)[0]
    assert (got.frames, got.frames_ground, got.frames_left, got.m.n, got.n_far) == (4, 1, 0, BIG, 0)


def test_the_refusals_of_drift_from_fold(ssd):
    L = ssd.lib()
    arr = (ssd.Camera * 2)()
    for i, c in enumerate(cams(ssd, 2)):
        arr[i].cal = c
    fold = (ssd.CameraFold * 2)()
    fold[1].camera = 1
    out = (ssd.CameraDrift * 2)()
    C.memset(out, 0xA5, C.sizeof(out))
    before = bytes(out)
    for args in ((None, arr, 2, 1, out), (fold, None, 2, 1, out), (fold, arr, 2, 1, None), (fold, arr, 0, 1, out), (fold, arr, -1, 1, out),
                 (fold, arr, ssd.MAX_CAMERAS + 1, 1, out)):
        assert L.ssd_camera_drift_from_fold(*args) == E_ARG, args[2:4]
        assert L.ssd_last_error() and bytes(out) == before
    fold[1].camera = 0
    assert L.ssd_camera_drift_from_fold(fold, arr, 2, 1, out) == E_ARG
    assert b"record 1 names camera 0" in L.ssd_last_error() and bytes(out) == before
    fold[1].camera = 1
    assert L.ssd_camera_drift_from_fold(fold, arr, 2, 1, out) == 0
    assert [(d.camera, d.frames, d.fit.status) for d in out] == [(0, 0, ssd.GF_FEW), (1, 0, ssd.GF_FEW)]
    assert bytes(out[1].fit.cal) == bytes(arr[1].cal)
    with pytest.raises(ssd.SsdError, match="one CameraFold per camera"):
        ssd.camera_drift_from_fold(list(fold), cams(ssd, 1))
    # null handles are refused by the device entry points before anything else
    dummy = C.c_void_p(4096)
    assert L.ssd_enqueue_camera_fold(None, dummy, dummy, 1, 1, 0, None, dummy) == E_ARG and b"null" in L.ssd_last_error()
    assert L.ssd_enqueue_camera_ground_gates(None, dummy, dummy, 1, dummy, 1, 1, 2.5, 0.0, None, dummy) == E_ARG and b"null" in L.ssd_last_error()
    assert L.ssd_enqueue_cameras_surface_refit_folded(None, dummy, 12, 1, None, 0, dummy, 1, 2.5, 0.0, 1, dummy) == E_ARG and b"null" in L.ssd_last_error()
    idx = (C.c_uint16 * 1)(0)
    assert L.ssd_process_host_cameras_drift(None, dummy, 1, idx, 0, (ssd.FrameResult * 1)(), 1, 2.5, 0.0, 0, 1, out) == E_ARG and L.ssd_last_error()
