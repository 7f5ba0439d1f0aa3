"""The depth edge filter's host statement (ssd_depth_edge_default_rule, ssd_depth_edges_host; include/ssd_hip.h) on the
CPU: against tests/edges_model.py, the rule in numpy written from its text, byte for byte on frame, class map and record; on small frames
stated by hand, one per edge of the rule, with what the text says must come out; on the two properties that follow from the text; and
on the directions the figures of profiles/depth_edges_accuracy.txt show.  No GPU is needed: tests/test_gpu_depth_edges.py holds the
kernel to this statement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import edges_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = em.hand_frames()


def test_exports_and_structure_sizes(ssd):
    names = ("ssd_depth_edge_default_rule", "ssd_depth_edges_host", "ssd_enqueue_depth_edges", "ssd_fetch_depth_edges", "ssd_get_depth_edges_time",
             "ssd_process_depth_host_edges")
    assert all(n in ssd.EXPORTS and hasattr(ssd.lib(), n) for n in names)
    assert C.sizeof(ssd.EdgeRule) == 16 and C.sizeof(ssd.EdgeStats) == 64
    assert [f for f, _ in ssd.EdgeStats._fields_] == list(em.STATS) + ["reserved"]
    assert (ssd.EDGE_KEPT, ssd.EDGE_EMPTY, ssd.EDGE_LONE, ssd.EDGE_BRIDGE) == (em.KEPT, em.EMPTY, em.LONE, em.BRIDGE) == (0, 1, 2, 3)
    for name in ("depth_edges_host", "depth_edges_default_rule"):
        assert callable(getattr(ssd, name))
    for name in ("enqueue_depth_edges", "fetch_depth_edges", "depth_edges_time", "process_depth_host_edges"):
        assert callable(getattr(ssd.Detector, name))


def test_the_default_rule(ssd):
    r = ssd.depth_edges_default_rule()
    assert (r.min_support, r.bridge, r.tol, r.slope) == (2, 1, ssd.FUSE_TOL, ssd.EDGE_SLOPE) == em.DEFAULT
    assert r.slope in em.SLOPES
    assert ssd.lib().ssd_depth_edge_default_rule(None) == -1


def test_every_refusal_of_the_host_statement(ssd):
    L = ssd.lib()
    f = np.full((2, 3), 100, np.uint16)
    out, cls, st = np.zeros(6, np.uint16), np.zeros(6, np.uint8), ssd.EdgeStats()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                                   # noqa: E731

    def call(w=3, h=2, frame=p(f), rule=None, o=p(out), c=p(cls), stats=C.byref(st)):
        return L.ssd_depth_edges_host(w, h, frame, None if rule is None else C.byref(rule), o, c, stats)
    R = ssd.EdgeRule
    refused = [call(frame=None), call(o=None), call(stats=None), call(w=0), call(h=0), call(w=-3), call(h=-1), call(rule=R(-1, 1, 40, 0)),
               call(rule=R(9, 1, 40, 0)), call(rule=R(2, 1, -1, 0)), call(rule=R(2, 1, 65536, 0)), call(rule=R(2, 1, 40, -1)),
               call(rule=R(2, 1, 40, 4097))]
    assert refused == [-1] * len(refused)
    assert b"ssd_depth_edges_host" in L.ssd_last_error()
    assert call() == 0 and call(c=None) == 0 and call(rule=R(0, 0, 0, 0)) == 0 and call(rule=R(8, -7, 65535, 4096)) == 0
    assert call(rule=R(2, 1, 40, 0)) == 0 and st.n_kept == 6 and (out == 100).all() and st.sum_support == 4 * 3 + 2 * 5


@pytest.fixture(scope="module")
def frames(ssd):
    clean = em.clean_frame(ssd, 64, 48)
    return {"clean": clean, "stress": em.stress_frame(ssd, 64, 48), "mixed": em.plant_mixed(clean)[0]}


@pytest.mark.parametrize("rule", em.RULES, ids=[str(r) for r in em.RULES])
@pytest.mark.parametrize("which", ["clean", "stress", "mixed"])
def test_the_host_statement_equals_the_model_on_the_scene(ssd, frames, which, rule):
    f = frames[which]
    want_o, want_c, want_st = em.edges_np(f, rule)
    out, st, cls = ssd.depth_edges_host(f, em.rule_of(ssd, rule), classes=True)
    assert (out == want_o).all() and (cls == want_c).all() and em.stats_dict(st) == want_st
    out2, st2 = ssd.depth_edges_host(f, em.rule_of(ssd, rule))                  # the class map NULL
    assert (out2 == out).all() and bytes(st2) == bytes(st)
    assert st.n_kept + st.n_empty + st.n_lone + st.n_bridge == f.size
    if which != "clean" and rule is None:
        assert st.n_lone > 0 and (which == "stress" or st.n_bridge > 0), "the frame exercises the classes"


def test_the_rules_of_the_sweep_include_the_switches():
    rules = [r for r in em.RULES if r is not None]
    assert len(em.RULES) >= 4 and any(r[0] == 0 for r in rules) and any(r[1] == 0 for r in rules) and any(r[3] == 0 for r in rules) and \
        any(r[2] == 0 for r in rules)


@pytest.mark.parametrize("case", range(len(HAND)), ids=[h[0] for h in HAND])
def test_the_rules_edges_by_hand(ssd, case):
    """what the rule's text says must come out, one small frame per case, stated in edges_model.hand_frames and taken from no
    implementation; the model is held to the same statements"""
    name, f, rule, want = HAND[case]
    out, st, cls = ssd.depth_edges_host(f, em.rule_of(ssd, rule), classes=True)
    mo, mc, mst = em.edges_np(f, rule)
    for (y, x), (o, c) in want.items():
        assert (int(out[y, x]), int(cls[y, x])) == (o, c), "%s: pixel (%d, %d)" % (name, y, x)
        assert (int(mo[y, x]), int(mc[y, x])) == (o, c), "%s: the model at (%d, %d)" % (name, y, x)
    assert (out == mo).all() and (cls == mc).all() and em.stats_dict(st) == mst
    assert ((out == f) | (out == 0)).all() and ((cls == em.KEPT) == ((out != 0))).all()


def test_the_hand_frames_cover_the_issues_list():
    names = " | ".join(h[0] for h in HAND)
    for piece in ("corner", "edge at min_support", "exactly t", "t + 1", "3 beside 65500", "saturates", "W/E", "N/S", "NW/SE", "NE/SW",
                  "outside the frame", "invalid", "lone and bridged", "1 x 1", "1 x N", "N x 1"):
        assert piece in names, piece
    assert {h[1].shape for h in HAND} >= {(1, 1), (1, 7), (5, 1)}


def test_a_mixed_pixel_between_two_sides_is_always_removed(ssd):
    """property 1: every pixel of the model's truth subset (more than t from valid pixels on opposite sides of it, on opposite sides in
    depth) is removed, under the defaults and with t growing with the depth"""
    for w, h, rule in ((64, 48, None), (256, 192, None), (256, 192, (2, 1, 40, 64)), (256, 192, (0, 1, 10, 0))):
        f, planted, truth = em.plant_mixed(em.clean_frame(ssd, w, h), rule=rule)
        out, _, cls = ssd.depth_edges_host(f, em.rule_of(ssd, rule), classes=True)
        assert truth.sum() >= 50 and (truth <= planted).all()
        assert (out[truth] == 0).all() and np.isin(cls[truth], (em.LONE, em.BRIDGE)).all()
        if rule is not None and rule[0] == 0:
            assert (cls[truth] == em.BRIDGE).all(), "with the LONE test off it is BRIDGE that takes them"


def test_a_ramp_stepping_by_t_loses_nothing_to_bridge_and_by_more_its_interior(ssd):
    """property 2, on ramps whose step from pixel to pixel is exactly t and t + 1 (slope 0: t is the same everywhere)"""
    for tol in (0, 1, 40, 333):
        rule = ssd.EdgeRule(0, 1, tol, 0)
        for flip in (False, True):
            at = em.ramp(40, 5, tol)
            at = at[:, ::-1].copy() if flip else at
            out, st, cls = ssd.depth_edges_host(at, rule, classes=True)
            assert st.n_bridge == 0 and (out == at).all()
            over = em.ramp(40, 5, tol + 1)
            over = over[:, ::-1].copy() if flip else over
            out, st, cls = ssd.depth_edges_host(over, rule, classes=True)
            assert (cls[:, 1:-1] == em.BRIDGE).all() and (cls[:, 0] == em.KEPT).all() and (cls[:, -1] == em.KEPT).all()
            assert st.n_bridge == 38 * 5
    # with a slope, a ramp whose every step is t of the LOWER pixel of the step (t does not fall with the depth) loses nothing either
    rule = (0, 1, 40, 128)
    row = [1000]
    for _ in range(39):
        row.append(row[-1] + em.t_of(row[-1], rule))
    f = np.array([row] * 3, np.uint16)
    assert ssd.depth_edges_host(f, ssd.EdgeRule(*rule))[1].n_bridge == 0


@pytest.fixture(scope="module")
def figures(ssd, oracle):
    return em.accuracy(ssd, oracle)


def test_the_directions_of_the_accuracy_record(ssd, oracle, figures):
    """Measured (profiles/depth_edges_accuracy.txt): the whole truth subset goes, no clean surface pixel does, 99 % of the stress
    configuration's outliers go beside 12 % of its inliers.  The plain scene's planted pixels are nobody's occupants (its treads lie below the camera: the pixels
    at its jumps hang beside the staircase), so the occupants are counted with a box on every surface as well."""
    a = figures
    print(a)
    assert a["truth"] > 100 and a["truth_removed"] == a["truth"], "the whole truth subset with valid sides is removed"
    assert a["surface"] > 10000 and a["surface_removed"] <= em.LOSS_CAP * a["surface"], "the clean frame's loss within the cap"
    assert a["outliers"] > 1000 and a["outliers_removed"] * a["inliers"] > 4 * a["inliers_removed"] * a["outliers"], \
        "the outliers' share that goes is more than four times the inliers'"
    for before, after in list(zip(a["occupants_before"], a["occupants_after"])) + list(zip(a["box_before"], a["box_after"])):
        assert after < before or before == 0, "fewer occupants after than before on every tread that had any"
    assert all(n > 0 for n in a["box_before"]) and len(a["box_before"]) == 3


def test_the_default_slope_is_the_measured_one(ssd, oracle):
    """the smallest candidate at which the noise-free frames of tests/sweep_scenes.py lose at most 0.1 % of the pixels the oracle's labels
    assign to a reported surface"""
    slope, rows = em.chosen_slope(ssd, oracle)
    print(rows)
    assert slope == ssd.EDGE_SLOPE == ssd.depth_edges_default_rule().slope
    assert all(n > 100000 for _, _, n in rows)
    removed = dict((s, r) for s, r, _ in rows)
    assert all(removed[a] >= removed[b] for a, b in zip(em.SLOPES, em.SLOPES[1:])), "a wider t loses no more"


def test_the_recorded_accuracy_is_this_codes(ssd, oracle):
    """profiles/depth_edges_accuracy.txt, computed again"""
    path = os.path.join(ROOT, "profiles", "depth_edges_accuracy.txt")
    assert open(path).read().splitlines() == em.accuracy_lines(ssd, oracle)


def test_the_sanitizer_program_runs_clean():
    """tools/host_sanitize.sh depth_edges: csrc/ssd_host.cpp and a stand-alone program under AddressSanitizer and UBSan, on the CPU"""
    import shutil
    if shutil.which("hipconfig") is None:
        pytest.skip("hipconfig is not installed")
    run = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_sanitize.sh"), "depth_edges"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "depth edge filter host functions: clean" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
