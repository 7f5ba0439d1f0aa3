"""The depth fill's host statement (ssd_depth_fill_default_rule, ssd_depth_fill_host; include/ssd_hip.h) on the CPU:
against tests/fill_model.py, the rule in numpy written from its text, byte for byte on frame, class map and record; on small frames stated
by hand, one per edge of the rule, with what the text says must come out; on the three properties that follow from the text; and on the
conditions the figures of profiles/depth_fill_accuracy.txt meet.  No GPU is needed: tests/test_gpu_depth_fill.py holds the kernel to this
statement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fill_model as fm
import warp_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ssd_depth_fill_default_rule", "ssd_depth_fill_host", "ssd_enqueue_depth_fill", "ssd_fetch_depth_fill", "ssd_get_depth_fill_time",
         "ssd_process_depth_host_fill", "ssd_process_depth_host_warp_fill_fused")
HAND = fm.hand_frames()
BORDER = fm.border_frames()


def test_exports_and_structure_sizes(ssd):
    assert all(n in ssd.EXPORTS and hasattr(ssd.lib(), n) for n in NAMES)
    assert C.sizeof(ssd.FillRule) == 16 and C.sizeof(ssd.FillStats) == 64
    assert [f for f, _ in ssd.FillRule._fields_] == ["min_pairs", "cover", "tol", "slope"]
    assert [f for f, _ in ssd.FillStats._fields_] == list(fm.STATS) + ["reserved"]
    assert (ssd.FILL_KEPT, ssd.FILL_EMPTY, ssd.FILL_FILLED, ssd.FILL_COVERED) == (fm.KEPT, fm.EMPTY, fm.FILLED, fm.COVERED) == (0, 1, 2, 3)
    for name in ("depth_fill_host", "depth_fill_default_rule"):
        assert callable(getattr(ssd, name))
    for name in ("enqueue_depth_fill", "fetch_depth_fill", "depth_fill_time_ms", "process_depth_host_fill", "process_depth_host_warp_fill_fused"):
        assert callable(getattr(ssd.Detector, name))


def test_the_default_rule(ssd):
    r = ssd.depth_fill_default_rule()
    assert dict(min_pairs=r.min_pairs, cover=r.cover, tol=r.tol, slope=r.slope) == dict(min_pairs=1, cover=1, tol=ssd.FUSE_TOL, slope=0) == fm.DEFAULT
    assert ssd.lib().ssd_depth_fill_default_rule(None) == -1


def test_every_refusal_of_the_host_statement(ssd):
    L = ssd.lib()
    f = np.full((2, 3), 100, np.uint16)
    out, cls, st = np.zeros(6, np.uint16), np.zeros(6, np.uint8), ssd.FillStats()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                                   # noqa: E731

    def call(w=3, h=2, frame=p(f), rule=None, o=p(out), c=p(cls), stats=C.byref(st)):
        return L.ssd_depth_fill_host(w, h, frame, None if rule is None else C.byref(rule), o, c, stats)
    R = ssd.FillRule
    refused = [call(frame=None), call(o=None), call(stats=None), call(w=0), call(h=0), call(w=-3), call(h=-1), call(rule=R(0, 1, 40, 0)),
               call(rule=R(5, 1, 40, 0)), call(rule=R(-1, 1, 40, 0)), call(rule=R(1, -1, 40, 0)), call(rule=R(1, 5, 40, 0)),
               call(rule=R(1, 1, -1, 0)), call(rule=R(1, 1, 65536, 0)), call(rule=R(1, 1, 40, -1)), call(rule=R(1, 1, 40, 4097))]
    assert refused == [-1] * len(refused)
    assert b"ssd_depth_fill_host" in L.ssd_last_error()
    assert call() == 0 and call(c=None) == 0 and call(rule=R(1, 0, 0, 0)) == 0 and call(rule=R(4, 4, 65535, 4096)) == 0
    assert call(rule=R(1, 1, 40, 0)) == 0 and st.n_kept == 6 and (out == 100).all() and (cls == 0).all() and st.sum_pairs == st.sum_spread == 0


@pytest.fixture(scope="module")
def frames(ssd):
    """the clean, the stress and the 10 %-invalid scene at 64 x 48, each as it is, under the seeded views and pulled near"""
    scenes, src = wm.scene_frames(ssd), wm.scene_src(ssd, 64, 48)
    out = {"scene %d" % i: f for i, f in enumerate(scenes)}
    for k, v in enumerate(wm.seeded_views(ssd, src)):
        out["seeded view %d" % k] = ssd.depth_warp_host(scenes[k % 3], v, src)[0]
    for i, f in enumerate(scenes):
        out["pulled near %d" % i] = ssd.depth_warp_host(f, wm.pull_near_view(ssd, src), src)[0]
    out["pulled 0.1"] = ssd.depth_warp_host(scenes[0], wm.pull_near_view(ssd, src, 0.1), src)[0]
    return out


@pytest.mark.parametrize("rule", fm.RULES, ids=[str(sorted(r.items())) for r in fm.RULES])
def test_the_host_statement_equals_the_model_on_the_scenes(ssd, frames, rule):
    seen = np.zeros(4, np.int64)
    for name, f in frames.items():
        out, cls, st = fm.host(ssd, f, rule)
        out2, st2 = ssd.depth_fill_host(f, fm.make_rule(ssd, rule))                  # the class map NULL
        assert (out2 == out).all() and fm.stats_dict(st2) == st, name
        seen += np.bincount(cls.reshape(-1), minlength=4)
    assert seen[fm.KEPT] > 0 and seen[fm.EMPTY] > 0 and seen[fm.FILLED] > 0, "the frames exercise the classes"
    assert seen[fm.COVERED] == 0 if rule["cover"] == 0 else seen[fm.COVERED] > 0 or rule["cover"] > 2, "... COVERED where the rule has it within reach"


def test_the_rules_of_the_sweep(ssd):
    assert {r["min_pairs"] for r in fm.RULES} == {1, 2, 3, 4} and {0, 1, 2} <= {r["cover"] for r in fm.RULES}
    assert {0, 32} <= {r["slope"] for r in fm.RULES} and 0 in {r["tol"] for r in fm.RULES} and len(fm.RULES) >= 6


def test_the_seeded_frames_equal_the_model(ssd):
    for zeros in (0.1, 0.6):
        for rule in fm.RULES:
            _, cls, st = fm.host(ssd, fm.seeded_frame(72, 40, zeros, seed=11), rule)
        _, cls, st = fm.host(ssd, fm.seeded_frame(72, 40, zeros, seed=11))
        assert st["n_filled"] > 50 and st["n_covered"] > 20 and st["n_empty"] > 0


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_the_frames_stated_by_hand(ssd, case):
    name, rule, f, want, want_cls = case
    # turned by half a turn every pair keeps its place in the rule's order with its two ends swapped: the same must come out
    for g in (f, f[::-1, ::-1].copy()):
        out, cls, st = fm.host(ssd, g, rule)
        assert (int(out[1, 1]), int(cls[1, 1])) == (want, want_cls), (name, out, cls)
        if want_cls in (fm.FILLED, fm.COVERED):
            assert 1 <= st["sum_pairs"] <= 4 * (st["n_filled"] + st["n_covered"])
    fm.host(ssd, f.T.copy(), rule)                                   # (transposed, W/E and N/S change places: held to the model only)


def test_a_tie_goes_to_the_first_pair_in_the_rules_order(ssd):
    """all four pairs with one spread, each pair's middle its own: the W/E pair's comes out; without it the N/S pair's; and so on"""
    ends = dict(w=1000, e=1010, n=2000, s=2010, nw=3000, se=3010, ne=4000, sw=4010)
    mids = (1005, 2005, 3005, 4005)
    for first in range(4):
        keep = {k: v for i, pair in enumerate(fm.PAIR_ENDS) if i >= first for k, v in ends.items() if k in pair}
        out, cls, st = fm.host(ssd, fm._around(0, **keep))
        assert int(out[1, 1]) == mids[first] and st["sum_pairs"] == 4 - first and st["sum_spread"] == 10
        out, cls, st = fm.host(ssd, fm._around(9000, **keep))
        assert (int(out[1, 1]), int(cls[1, 1])) == (mids[first], fm.COVERED)


@pytest.mark.parametrize("case", BORDER, ids=[c[0] for c in BORDER])
def test_borders_corners_and_the_smallest_frames(ssd, case):
    name, f, want = case
    for rule in fm.RULES:
        out, cls, st = fm.host(ssd, f, rule)
        if rule == fm.DEFAULT:
            assert (out == want).all(), (name, rule, out)
    if 1 in f.shape:
        t = f.reshape(-1)
        out, cls, st = fm.host(ssd, f)
        for i in np.flatnonzero(cls.reshape(-1) == fm.FILLED):
            assert 0 < i < t.size - 1 and t[i - 1] != 0 and t[i + 1] != 0, "only the pair along the line exists"
    if f.size == 1:
        assert st["n_filled"] == st["n_covered"] == 0, "nothing can fill in 1 x 1"


def test_one_row_and_one_column_of_every_kind(ssd):
    rng = np.random.default_rng(3)
    line = np.where(rng.random(97) < 0.4, 0, 1000 + rng.integers(-25, 26, 97)).astype(np.uint16)
    line[[9, 10, 11, 49, 50, 51]] = 1000, 40000, 1005, 1010, 40000, 990
    for f in (line.reshape(1, -1), line.reshape(-1, 1)):
        out, cls, st = fm.host(ssd, f)
        assert st["n_filled"] > 5 and st["n_covered"] >= 1 and st["sum_pairs"] == st["n_filled"] + st["n_covered"]


# ---- the three properties ---------------------------------------------------------------------------------------------------------------
def test_property_i_a_frame_without_zeros_comes_back_with_cover_off(ssd, frames):
    rng = np.random.default_rng(8)
    for f in [np.maximum(f, 1) for f in frames.values()] + [rng.integers(1, 65536, (37, 53)).astype(np.uint16), fm.seeded_frame(72, 40, 0.0, 4, seams=False)]:
        assert (f != 0).all()
        for rule in fm.RULES:
            out, st, cls = ssd.depth_fill_host(f, fm.make_rule(ssd, dict(rule, cover=0)), classes=True)
            assert out.tobytes() == f.tobytes() and (cls == fm.KEPT).all() and st.n_kept == f.size


def test_property_ii_every_written_value_lies_between_an_agreeing_pair(ssd, frames):
    """nothing is ever written nearer than both, or farther than both, of the two samples it stands between"""
    pool = list(frames.values()) + [fm.seeded_frame(72, 40, z, s) for z, s in ((0.1, 1), (0.6, 2))]
    written = 0
    for rule in fm.RULES:
        for f in pool:
            out, st, cls = ssd.depth_fill_host(f, fm.make_rule(ssd, rule), classes=True)
            g = f.astype(np.int64)
            inside = np.zeros(f.shape, bool)
            for pa, pb in fm.PAIRS:
                a, b = fm.shift(g, *pa), fm.shift(g, *pb)
                lo, hi = np.minimum(a, b), np.maximum(a, b)
                t = np.minimum(65535, rule["tol"] + ((lo * rule["slope"]) >> 12))
                inside |= (a != 0) & (b != 0) & (hi - lo <= t) & (out >= lo) & (out <= hi)
            new = (cls == fm.FILLED) | (cls == fm.COVERED)
            assert inside[new].all() and (out[~new] == f[~new]).all()
            assert (out[cls == fm.COVERED] < f[cls == fm.COVERED]).all(), "a covered sample only ever comes nearer"
            written += int(new.sum())
    assert written > 10000


def test_property_iii_a_hole_on_a_step_stays_empty(ssd):
    """a hole whose four pairs each straddle a step of t + 1 stays EMPTY, whichever end of each pair is the near one; at a step of t
    every pair agrees and it fills"""
    checked = 0
    for tol, slope in ((40, 0), (0, 0), (10, 32), (65535, 0), (7, 4096)):
        for near in (1, 4096, 30000):
            t = min(65535, tol + ((near * slope) >> 12))
            for step, fills in ((t + 1, False), (t, True)):
                if near + step > 65535:
                    continue
                for sides in range(16):
                    ends = {}
                    for i, (a, b) in enumerate(fm.PAIR_ENDS):
                        ends[a], ends[b] = (near, near + step) if (sides >> i) & 1 else (near + step, near)
                    out, cls, st = fm.host(ssd, fm._around(0, **ends), dict(tol=tol, slope=slope, cover=0))
                    assert int(cls[1, 1]) == (fm.FILLED if fills else fm.EMPTY) and (int(out[1, 1]) != 0) == fills, (tol, slope, near, step, sides)
                    checked += 1
    assert checked >= 300


def test_the_classes_counts_sum_to_the_pixel_count(ssd, frames):
    for f in list(frames.values()) + [np.zeros((5, 7), np.uint16), np.full((5, 7), 65535, np.uint16)]:
        for rule in fm.RULES:
            _, st = ssd.depth_fill_host(f, fm.make_rule(ssd, rule))
            assert st.n_kept + st.n_empty + st.n_filled + st.n_covered == f.size
            assert st.n_filled + st.n_covered <= st.sum_pairs <= 4 * (st.n_filled + st.n_covered)
            assert st.n_kept + st.n_covered == int((f != 0).sum()) and 0 <= st.sum_spread <= 65534 * (st.n_filled + st.n_covered)


# ---- what the fill achieves -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def figures(ssd):
    return fm.accuracy_figures(ssd)


def test_the_accuracy_conditions(ssd, figures):
    """host statements only, tests/warp_model.py's recipes unchanged, the default rule, one pass, 256 x 192, against the clean frame of the
    target pose.  Measured (profiles/depth_fill_accuracy.txt): pull_near_view 0.1 / 0.2 / 0.4 m 83.36 / 68.03 / 43.38 % non-zero before,
    99.64 / 99.39 / 98.93 % after; the 30 cm approach 57.51 % valid and 1.231 % far before, 87.35 % and 0.228 % after (0.862 % with cover
    off); clean poses 1 .. 4 96.58 / 97.26 / 97.65 / 96.24 % valid before, 96.59 / 98.45 / 99.13 / 99.31 % after; noisy, fused, n = 3
    95.79 % valid, 0.062 % far, rms 7.18 before, 98.28 %, 0.064 %, 6.90 after; n = 5 98.67 %, 0.033 %, 5.43 before, 99.61 %, 0.039 %,
    5.22 after; 2 of the clean target frame's 49,152 pixels change"""
    a = figures
    for row in fm.accuracy_rows(a):
        print(row)
    for before, after in a["pull"]:
        assert after >= 0.98, "a magnified view: at least 98 % of the pixels are non-zero after the fill"
        assert before < 0.90, "(the recipe leaves holes to fill)"
    ap = a["approach"]
    assert ap["after"][0] >= 0.85, "the 30 cm approach: at least 85 % valid"
    assert ap["after"][1] <= 0.5 * ap["no_cover"][1], "the far share with the default rule is at most half of that with cover 0"
    assert ap["after"][1] < ap["before"][1] and ap["no_cover"][1] < ap["before"][1], "both far shares are below the unfilled frame's"
    for i, (before, after) in enumerate(a["clean"]):
        assert after[0] >= before[0], "valid never falls"
        assert i == 0 or after[0] >= before[0] + 0.01, "valid rises by at least one point for poses 2 .. 4"
        assert after[1] <= before[1] + 0.0001, "the far share is at most 0.01 points above the unfilled frame's"
    for key, rise in (("fused3", 0.02), ("fused5", 0.005)):
        before, after = a[key]
        assert after[0] >= before[0] + rise, "valid rises by at least 2 points at n = 3 and 0.5 points at n = 5"
        assert after[1] <= 0.001, "the far share is at most 0.1 %, the warp's own condition"
        assert after[2] <= before[2], "the rms is at most the unfilled chain's"
    changed, size = a["changed"]
    assert changed <= 0.0001 * size, "the clean target frame: at most 0.01 % of its pixels change"


def test_the_recorded_accuracy_is_this_codes(ssd, figures):
    """profiles/depth_fill_accuracy.txt's rows, computed again"""
    rows = [l for l in open(os.path.join(ROOT, "profiles", "depth_fill_accuracy.txt")).read().splitlines() if l and l[0] == " "]
    got = fm.accuracy_rows(figures)
    assert len(rows) >= len(got)
    for line, (label, before, after) in zip(rows, got):
        cells = [c.strip() for c in line.split("|")]
        assert cells[0] == label and cells[1].split() == before and cells[2].split() == after, line


def test_the_sanitizer_program_runs_clean():
    """tools/host_sanitize.sh depth_fill: csrc/ssd_host.cpp and a stand-alone program under AddressSanitizer and UBSan, on the CPU"""
    import shutil
    if shutil.which("hipconfig") is None:
        pytest.skip("hipconfig is not installed")
    run = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_sanitize.sh"), "depth_fill"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "depth fill host functions: clean" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
