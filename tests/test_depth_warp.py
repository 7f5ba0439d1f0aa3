"""The depth warp's host functions (ssd_depth_warp_host, ssd_depth_warp_view_between; include/ssd_hip.h) on the CPU:
against tests/warp_model.py, the rule in numpy written from its text, byte for byte on frame and record; on frames made by hand, one per
class, with what the text says must come out; the view between two cameras against numpy; and the conditions the figures of
profiles/depth_warp_accuracy.txt meet.  No GPU is needed: tests/test_gpu_depth_warp.py holds the kernel to this statement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import warp_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ssd_depth_warp_view_between", "ssd_depth_warp_host", "ssd_enqueue_depth_warp", "ssd_fetch_depth_warp", "ssd_get_depth_warp_time",
         "ssd_process_depth_host_warp_fused")


def _intr(ssd, fx, fy, ppx, ppy, units):
    i = ssd.Intrinsics()
    i.fx, i.fy, i.ppx, i.ppy, i.depth_units = fx, fy, ppx, ppy, units
    return i


def _both(ssd, frame, view, dst):
    """the host statement, held to the model and to the record's sums -> (warped frame, its record as a dict)"""
    out, st = ssd.depth_warp_host(frame, view, dst)
    want, want_st = wm.warp_np(frame, view, dst)
    got = wm.stats_dict(st)
    assert (out == want).all() and got == want_st, (got, want_st)
    assert sum(got[k] for k in wm.STATS[:5]) == frame.size and got["n_filled"] == int((out != 0).sum()) <= got["n_landed"]
    assert list(st.reserved) == [0, 0]
    return out, got


def test_exports_and_structure_sizes(ssd):
    assert all(n in ssd.EXPORTS and hasattr(ssd.lib(), n) for n in NAMES)
    assert C.sizeof(ssd.WarpView) == 120 and C.sizeof(ssd.WarpStats) == 64
    assert [f for f, _ in ssd.WarpStats._fields_][:6] == list(wm.STATS)
    assert ssd.WarpView.src.offset == 96 and ssd.WarpView.t.offset == 72


def test_every_refusal_of_the_host_statement(ssd):
    L = ssd.lib()
    src = _intr(ssd, 8, 8, 1, 1, 0.001)
    f, out, st = np.full((2, 3), 100, np.uint16), np.zeros(6, np.uint16), ssd.WarpStats()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                                   # noqa: E731
    good = wm.identity_view(ssd, src)

    def view(**kw):
        v = ssd.WarpView.from_buffer_copy(good)
        for k, (i, x) in kw.items():
            if k == "src":
                setattr(v.src, i, x)
            else:
                getattr(v, k)[i] = x
        return v

    def call(w=3, h=2, frame=p(f), v=good, dst=src, o=p(out), stats=C.byref(st)):
        return L.ssd_depth_warp_host(w, h, frame, None if v is None else C.byref(v), None if dst is None else C.byref(dst), o, stats)
    nan, inf = float("nan"), float("inf")
    refused = [call(frame=None), call(v=None), call(dst=None), call(o=None), call(stats=None), call(w=0), call(h=0), call(w=-3),
               call(dst=_intr(ssd, 0, 8, 1, 1, 0.001)), call(dst=_intr(ssd, 8, 0, 1, 1, 0.001)), call(dst=_intr(ssd, 8, 8, 1, 1, 0.0)),
               call(dst=_intr(ssd, 8, 8, 1, 1, -0.001)), call(v=view(src=("fx", 0.0))), call(v=view(src=("fy", 0.0))),
               call(v=view(src=("depth_units", 0.0)))]
    refused += [call(v=view(r=(k, bad))) for k in range(9) for bad in (nan, inf)] + [call(v=view(t=(k, bad))) for k in range(3) for bad in (nan, -inf)]
    assert refused == [-1] * len(refused)
    assert b"ssd_depth_warp_host" in L.ssd_last_error()
    assert call() == 0 and st.n_landed == 6 and (out == 100).all()


@pytest.fixture(scope="module")
def scenes(ssd):
    return wm.scene_frames(ssd), wm.scene_src(ssd, 64, 48)


@pytest.mark.parametrize("k", range(8))
def test_the_host_statement_equals_the_model_under_the_seeded_views(ssd, scenes, k):
    frames, src = scenes
    view = wm.seeded_views(ssd, src)[k]
    for f in frames:
        _, st = _both(ssd, f, view, src)
        assert st["n_landed"] > 1500 and st["n_outside"] > 0, "the view moves the scene, and not out of sight"
    # another target: other intrinsics and another depth unit
    _both(ssd, frames[1], view, _intr(ssd, 50.0, 47.0, 30.25, 25.5, 0.0005))


def test_a_view_that_pushes_away_and_one_that_pulls_near(ssd, scenes):
    frames, src = scenes
    for f in frames:
        _, far = _both(ssd, f, wm.push_away_view(ssd, src), src)
        assert far["n_landed"] > 5 * far["n_filled"], "many samples per target pixel"
        out, near = _both(ssd, f, wm.pull_near_view(ssd, src), src)
        assert near["n_outside"] > 1000
        inner = out[8:-8, 8:-8]
        assert 0.2 < float((inner == 0).mean()) < 0.9, "holes between the samples"


def test_the_classes_by_hand(ssd):
    """what the rule's text says must come out, one frame per class, stated here and not taken from any implementation"""
    W, H = 8, 6
    src = _intr(ssd, 8, 8, 4, 3, 0.001)                               # the pixel (4, 3) looks along the axis; 1000 raw units are 1 m
    one = np.zeros((H, W), np.uint16)
    one[3, 4] = 1000

    def run(frame=one, r=np.eye(3), t=(0, 0, 0), dst=src):
        return _both(ssd, frame, wm.make_view(ssd, r, t, src), dst)
    out, st = run()
    assert (out == one).all() and st == dict(n_empty=47, n_behind=0, n_range=0, n_outside=0, n_landed=1, n_filled=1)
    # BEHIND: a half turn about the y axis
    out, st = run(r=np.diag([-1.0, 1.0, -1.0]))
    assert not out.any() and (st["n_behind"], st["n_landed"], st["n_filled"]) == (1, 0, 0)
    out, st = run(t=(0, 0, -1.0))
    assert st["n_behind"] == 1, "Z == 0 is behind"
    # RANGE: below 1 and above 65535 by t[2] - and the last values inside
    assert run(t=(0, 0, -0.9996))[1]["n_range"] == 1, "Z = 0.4 units rounds to 0"
    out, st = run(t=(0, 0, -0.9994))
    assert st["n_landed"] == 1 and out[3, 4] == 1, "Z = 0.6 units rounds to 1"
    assert run(t=(0, 0, 64.5356))[1]["n_range"] == 1, "65535.6 units round to 65536"
    out, st = run(t=(0, 0, 64.535))
    assert st["n_landed"] == 1 and out[3, 4] == 65535
    # OUTSIDE on each of the four sides: half a metre at one metre is four pixels
    for t, at in (((0.5, 0, 0), None), ((-0.5, 0, 0), (3, 0)), ((-0.625, 0, 0), None), ((0.375, 0, 0), (3, 7)), ((0, 0.375, 0), None), ((0, 0.25, 0), (5, 4)),
                  ((0, -0.375, 0), (0, 4)), ((0, -0.5, 0), None)):
        out, st = run(t=t)
        if at is None:
            assert st["n_outside"] == 1 and not out.any(), t
        else:
            assert st["n_landed"] == 1 and out[at] == 1000 and int((out != 0).sum()) == 1, t
    # two samples on one pixel: a target whose focal lengths send everything to (2, 1); the smaller wins in either order
    flat = _intr(ssd, 1e-6, 1e-6, 2, 1, 0.001)
    for a, b in ((3000, 2000), (2000, 3000)):
        two = np.zeros((H, W), np.uint16)
        two[0, 1], two[5, 6] = a, b
        out, st = run(frame=two, dst=flat)
        assert out[1, 2] == 2000 and (st["n_landed"], st["n_filled"]) == (2, 1) and int((out != 0).sum()) == 1
    # samples of 1 and 65535
    ends = np.zeros((H, W), np.uint16)
    ends[0, 0], ends[5, 7], ends[2, 2] = 1, 65535, 65535
    out, st = run(frame=ends)
    assert (out == ends).all() and st["n_landed"] == 3
    # a NaN fails the inside test: finite entries whose row sum is inf - inf give X = NaN, and the sample is OUTSIDE, never LANDED
    far = np.zeros((H, W), np.uint16)
    far[5, 7] = 65535                                                 # x and y both positive
    r = np.eye(3)
    r[0, 0], r[0, 1] = 1e308, -1e308
    out, st = run(frame=far, r=r)
    assert (st["n_outside"], st["n_landed"]) == (1, 0) and not out.any()


@pytest.mark.parametrize("shape", [(1, 2), (2, 1)])
def test_the_smallest_frames(ssd, shape):
    src = _intr(ssd, 2, 2, 0, 0, 0.001)
    f = np.array([1000, 65535], np.uint16).reshape(shape)
    out, st = _both(ssd, f, wm.identity_view(ssd, src), src)
    assert (out == f).all()
    out, st = _both(ssd, f, wm.make_view(ssd, np.eye(3), (-200.0, -200.0, 0), src), src)
    assert st["n_outside"] == 2 and not out.any()


def test_the_identity_is_an_exact_copy(ssd, scenes):
    frames, src = scenes
    for f in frames:
        out, st = _both(ssd, f, wm.identity_view(ssd, src), src)
        assert (out == f).all() and st["n_landed"] == st["n_filled"] == int((f != 0).sum())
    # every depth once, at a width where the float rounding of a pixel is largest among the frames a test can afford: 1024 x 64 holds
    # 0 .. 65535 (two rows of 1024 hold 2048 values)
    src = wm.scene_src(ssd, 1024, 64)
    every = np.random.default_rng(3).permutation(65536).astype(np.uint16).reshape(64, 1024)
    out, st = _both(ssd, every, wm.identity_view(ssd, src), src)
    assert (out == every).all() and (st["n_empty"], st["n_landed"], st["n_filled"]) == (1, 65535, 65535)
    two_rows = every[:2].copy()
    out, _ = _both(ssd, two_rows, wm.identity_view(ssd, wm.scene_src(ssd, 1024, 2)), wm.scene_src(ssd, 1024, 2))
    assert (out == two_rows).all()


# ---- ssd_depth_warp_view_between --------------------------------------------------------------------------------------------------------
def _camera(ssd, pose, w=64, h=48):
    sc = wm.pose_scene(ssd, pose, w=w, h=h)
    return ssd._as_camera(ssd.transformation_for_scene(sc), ssd.intrinsics_for_scene(sc))


def _rt(view):
    return np.array(list(view.r)).reshape(3, 3), np.array(list(view.t))


def test_the_view_between_two_cameras(ssd):
    poses = wm.ACC_POSES
    cams = [_camera(ssd, p) for p in poses]
    for s in range(len(cams)):
        for d in range(len(cams)):
            v = ssd.depth_warp_view_between(cams[s], cams[d])
            r, t = _rt(v)
            want_r, want_t = wm.view_between_np(cams[s].cal, cams[d].cal)
            # a few dozen double operations on numbers of order 1
            assert np.abs(r - want_r).max() < 1e-12 and np.abs(t - want_t).max() < 1e-12
            assert bytes(v.src) == bytes(cams[s].intr) and list(v.reserved) == [0]
            if s == d:
                assert np.abs(r - np.eye(3)).max() < 1e-12 and np.abs(t).max() < 1e-12, "equal cameras: the identity"
    # composition: src -> mid -> dst against src -> dst
    (r1, t1), (r2, t2), (r3, t3) = (_rt(ssd.depth_warp_view_between(cams[a], cams[b])) for a, b in ((1, 2), (2, 3), (1, 3)))
    assert np.abs(r2 @ r1 - r3).max() < 1e-12 and np.abs(r2 @ t1 + t2 - t3).max() < 1e-12
    # the calibrations come from three marks on the floor; the poses differ in pitch, roll and height and not along the floor (the
    # generator's camera does not move along it), so the view must be the one the scenes' axes give
    flat = [(p[0], p[1], p[2], 0.0) for p in poses]
    cams = [_camera(ssd, p) for p in flat]
    for s in range(1, len(flat)):
        r, t = _rt(ssd.depth_warp_view_between(cams[s], cams[0]))
        wr, wt = _rt(wm.pose_view(ssd, flat[s], flat[0], 64, 48))
        assert np.abs(r - wr).max() < 1e-9 and np.abs(t - wt).max() < 1e-9


def test_every_refusal_of_the_view_between(ssd):
    L = ssd.lib()
    a = _camera(ssd, wm.ACC_POSES[0])
    out = ssd.WarpView()

    def cam(**kw):
        c = ssd.Camera.from_buffer_copy(a)
        for k, v in kw.items():
            if k == "a":
                c.cal.a[v[0]] = v[1]
            elif k == "zero":
                for i in range(9):
                    c.cal.a[i] = 0.0
            elif k == "fx":
                c.intr.fx = v
            else:
                setattr(c, k, v)
        return c

    def call(s=a, d=a, o=out):
        return L.ssd_depth_warp_view_between(None if s is None else C.byref(s), None if d is None else C.byref(d), None if o is None else C.byref(o))
    refused = [call(s=None), call(d=None), call(o=None), call(s=cam(has_intrinsics=0)), call(s=cam(fx=0.0)), call(s=cam(a=(4, float("nan")))),
               call(d=cam(a=(0, float("inf")))), call(d=cam(zero=True))]
    assert refused == [-1] * len(refused)
    assert b"ssd_depth_warp_view_between" in L.ssd_last_error()
    assert call() == 0 and call(d=cam(has_intrinsics=0)) == 0, "dst needs no intrinsics"


# ---- what the warp achieves -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def figures(ssd):
    return wm.accuracy_figures(ssd)


def test_the_tables_numbers_as_conditions(ssd, figures):
    """256 x 192, five poses (up to 1 degree of pitch, 0.5 of roll, 2 cm of height, 3 cm along the floor), seeds 1000 .. 1004, sigma 2 mm,
    5 % outliers, 2 % invalid, against the clean frame of the target pose.  Measured (profiles/depth_warp_accuracy.txt): each clean warped
    frame fills 96.2 - 97.7 % of the target's valid pixels with 0.09 - 0.14 % far; warped and fused 98.67 % valid, 0.033 % far, rms 5.43
    against the single frame's 8.04; fused as they are 51.0 % valid"""
    a = figures
    print({k: a[k] for k in ("single", "unwarped", "warped_fused", "clean", "clean_unwarped")})
    for valid, far, _ in a["clean"]:
        assert valid >= 0.95, "each clean warped frame fills at least 95 % of the target's valid pixels"
        assert far <= 0.005, "... with at most 0.5 % of them more than 40 units off"
    assert all(far > 0.15 for _, far, _ in a["clean_unwarped"]), "(unwarped, the moved frames are far off)"
    valid, far, rms = a["warped_fused"]
    assert valid >= 0.95
    assert far <= 0.001, "the fusion test's own cap"
    assert rms <= a["single"][2], "the rms of the rest is at most the single frame's"
    assert a["unwarped"][0] < 0.80, "the recipe moves enough to matter"


def test_views_from_the_stair_poses_calibrations(ssd, oracle, figures):
    """end to end through what the stair pose hands back: every pose's noisy frame located against the target's map from the prior "the
    camera has not moved", the views from ssd_depth_warp_view_between over the solved cameras - motion along the floor included, which
    calibrations made from floor marks cannot carry.  The bounds are a tenth of the recipe's motion (1 degree, 3 cm), which moves a
    sample by about a third of a pixel at this size; the pixel conditions are the table's own.  Measured: at most 0.020 degrees and
    0.9 mm; 98.72 % valid, 0.033 % far, rms 5.45; the oracle's step heights within 2.5e-5 m"""
    s = wm.solved_figures(ssd, oracle, figures)
    print(s)
    assert s["status"] == [ssd.GF_OK] * 5 and s["passes"] == [3] * 5
    assert all(deg <= 0.1 and m <= 0.003 for deg, m in s["view_error"])
    valid, far, rms = s["pixels"]
    assert valid >= 0.95 and far <= 0.001 and rms <= figures["single"][2]
    assert s["detection"]["fused_steps"] == s["detection"]["clean_steps"] == 3


def test_the_recorded_accuracy_is_this_codes(ssd, figures):
    """profiles/depth_warp_accuracy.txt's rows with a condition, computed again"""
    rows = [l for l in open(os.path.join(ROOT, "profiles", "depth_warp_accuracy.txt")).read().splitlines() if l and l[0] == " "]
    a = figures
    got = [a["single"], a["unwarped"], a["warped_fused"]] + a["clean"]
    assert len(rows) >= len(got)
    for line, (valid, far, rms) in zip(rows, got):
        cells = [c.strip() for c in line.split("|")]
        assert cells[1:4] == ["%.2f" % (100 * valid), "%.3f" % (100 * far), "%.2f" % rms], line


def test_the_sanitizer_program_runs_clean():
    """tools/host_sanitize.sh depth_warp: csrc/ssd_host.cpp and a stand-alone program under AddressSanitizer and UBSan, on the CPU"""
    import shutil
    if shutil.which("hipconfig") is None:
        pytest.skip("hipconfig is not installed")
    run = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_sanitize.sh"), "depth_warp"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "depth warp host functions: clean" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
