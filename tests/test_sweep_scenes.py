"""The follow-on sweep on the host (tests/sweep_scenes.py): the list's variety as a CONDITION on the oracle's results alone, and every
host statement of a follow-on pass held to its numpy restatement on every frame of the list - the half that catches an error in a
shared header, which the device-against-host comparison of tests/test_gpu_sweep.py cannot see.  Everything compared is integers or
the outcome of one text of correctly rounded double operations: no tolerance anywhere, but for the riser's mean offset, which the
oracle sums in another order (1e-12 m, as tests/test_riser_fit.py).  Thrown and empty frames are cases, not exclusions: their
records are the all-zero or header-only records the host statement gives.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import clearance_model as cm
import ground_model as gm
import oracle_binding as ob
import refit_model as rfm
import riser_model as rm
import stair_pose_model as spm
import surface_model as sm
import sweep_scenes as ss
import tread_grid_model as tg
from test_labels import surfaces

RECORD = os.path.join(gm.ROOT, "profiles", "follow_on_sweep.txt")
CLEAR_RULES = (cm.RULE, (0.0, 0.02, 0.5))                     # the default; no margin and a low band: the riser faces leak in
CELLS = (tg.RULE[3], 0.005, 1.0)                              # the default and both ends of the cell's range
POSE_RULES = (spm.RULE, (0.05, 0.02, 0.05, 0.02))
RISER_TOLS, RISER_SUPPORT = (0.03, 0.008), 600                # a support some risers of the list reach and some do not
POSE_OFF = ((0.0, 0.0, 2.0 * spm.DEG), (0.0, 0.03, 0.0))      # a target's prior: the view's calibration turned by 2 degrees of yaw, moved 3 cm
INPUTS = pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])


def pose_prior(ssd, cal):
    return spm.moved(ssd, cal, *POSE_OFF)


def off_prior(ssd, sw, v):
    """view v's calibration as a rough prior has it: the pose moved by ground_model.PRIOR_OFF"""
    kw = dict(ss.camera_keywords()[v])
    kw["pitch_deg"] += gm.PRIOR_OFF[0]
    kw["roll_deg"] += gm.PRIOR_OFF[1]
    kw["cam_height"] += gm.PRIOR_OFF[2]
    return ssd.transformation_for_scene(ssd.make_scene(sw.w, sw.h, n_steps=0, **kw)).constants


def both(ssd, oracle, depth):
    """the list and its ragged part"""
    return [ss.sweep(ssd, oracle, depth), ss.sweep(ssd, oracle, depth, ragged=True)]


# ---- a. the variety, by the oracle alone ----------------------------------------------------------------------------------------------
def test_the_list_is_a_pure_function_of_its_seed():
    a, b = ss.scene_list(), ss.scene_list()
    assert a == b and a is not b and len(a) == ss.G * ss.V and ss.scene_list(ss.SEED + 1) != a
    assert sorted({kw["n_steps"] for _, _, kw in a}) == sorted(ss.STEPS) and (ss.W, ss.H) in ss.RESOLUTIONS
    for g in range(ss.G):
        mine = [kw for gg, _, kw in a if gg == g]
        for key in ("n_steps", "tread", "rise", "stair_width", "first_riser_y", "yaw_deg"):
            assert len({kw[key] for kw in mine}) == 1, "a staircase fixes " + key
        assert len({kw["seed"] for kw in mine}) == ss.V
    poses = ss.camera_keywords()
    assert len({tuple(sorted(p.items())) for p in poses}) == ss.V, "as many calibrations as views"
    for p in poses[1:]:
        assert abs(p["pitch_deg"] - poses[0]["pitch_deg"]) <= 2.0 and abs(p["roll_deg"] - poses[0]["roll_deg"]) <= 2.0 \
            and abs(p["cam_height"] - poses[0]["cam_height"]) <= 0.03
    assert {kw["outlier_frac"] for _, _, kw in a} <= set(ss.OUTLIERS) and {kw["invalid_frac"] for _, _, kw in a} <= set(ss.INVALID)
    for w, h in ss.RAGGED.values():
        assert (w * h) % 64 != 0
    assert ss.RAGGED[True][0] % 4 == 0 and ss.RAGGED[False][0] % 4 != 0


def test_the_oracle_finds_the_variety_the_sweep_stands_on(ssd, oracle):
    """a thrown frame, a live frame without steps, 1, 2, 3, 4 and 6 or more steps, a quarter of the frames live with two steps or more
    at 15 degrees of yaw or more, a live frame at 15 % outliers and one at 20 % invalid pixels - or the seed is the wrong one"""
    sw = ss.sweep(ssd, oracle)
    assert sw.n == ss.G * ss.V
    missing = [name for name, holds in ss.variety(sw).items() if not holds]
    assert not missing, (missing, sw.histogram())
    # what the issue names as never fed to a follow-on kernel: quadrilaterals turned by 20 to 40 degrees on live frames
    assert any(sw.live[i] and sw.records[i].n_steps >= 2 and 20.0 <= abs(sw.kws[i]["yaw_deg"]) <= 40.0 for i in range(sw.n))
    # ... and what the seed brought besides: live frames WITHOUT a ground (one reported surface, a step), whose records carry ground = 0
    assert any(sw.live[i] and sw.records[i].ground_ind < 0 for i in range(sw.n))
    # the depth form of the list is the same list to the oracle
    assert ss.variety(ss.sweep(ssd, oracle, True)) == ss.variety(sw)


def test_the_record_file_names_this_list(ssd, oracle):
    """profiles/follow_on_sweep.txt holds the seed, the resolution and the oracle's histogram of step counts of THIS list"""
    sw = ss.sweep(ssd, oracle)
    text = open(RECORD).read()
    hist = sw.histogram()
    line = ", ".join("%s: %d" % (k, hist[k]) for k in sorted(hist, key=str))
    for want in ("seed = %d" % ss.SEED, "resolution = %d x %d" % (ss.W, ss.H), "step histogram = " + line):
        assert want in text, want


# ---- b. host statement against numpy model, every frame ---------------------------------------------------------------------------------
@INPUTS
def test_ground_moments_equal_the_model(ssd, oracle, depth):
    """three tolerances; the view's own calibration and the one moved by PRIOR_OFF"""
    seen = 0
    for sw in both(ssd, oracle, depth):
        offs = [off_prior(ssd, sw, v) for v in range(ss.V)]
        for i in range(sw.n):
            for cal in (sw.cal_of(i), offs[sw.view[i]]):
                for tol in gm.TOLERANCES:
                    got = gm.moments_tuple(ssd.ground_moments_host(sw.cfg, (cal, sw.intr) if depth else cal, sw.frames[i], tol, depth=depth))
                    assert got == gm.moments_np(sw.cfg, cal, sw.pts[i], tol), (i, tol)
                    seen += got[0] > 200
    assert seen > ss.G * ss.V, "the frames show floor"


def _first(ssd, sw, i):
    """frame i's first-pass record over the oracle's labels: (n_surfaces, ground, FrameMoments)"""
    surf = surfaces(sw.records[i])
    n, ground = len(surf), 1 if surf and surf[0][2] else 0
    return n, ground, ssd.surface_moments_host(sw.cfg, sw.frames[i], sw.labels[i], n, ground, intr=sw.intr)


@INPUTS
def test_surface_moments_equal_the_model(ssd, oracle, depth):
    """ssd_surface_moments_host over expected_labels: surface_model.moments_py (Python integers) and moments_np on every frame"""
    for sw in both(ssd, oracle, depth):
        for i in range(sw.n):
            n, ground, fm = _first(ssd, sw, i)
            assert n == (0 if sw.thrown[i] else sw.records[i].n_steps)
            assert sm.frame_tuple(fm) == (n, ground, sm.pad(sm.moments_np(sw.pts[i], sw.labels[i], n), ssd.MAX_STEPS)), i
            if n == 0:
                assert bytes(fm) == bytes(C.sizeof(ssd.FrameMoments)), "a thrown or empty frame: the all-zero record"
            assert sm.frame_tuple(fm)[2] == sm.pad(sm.moments_py(sw.pts[i], sw.labels[i], n), ssd.MAX_STEPS), i


@INPUTS
def test_refit_moments_equal_the_model_through_two_passes(ssd, oracle, depth):
    """ssd_surface_refit_moments_host against refit_model under the gates of ssd_surface_gates_from_moments, each pass gated by the one
    before (the gates' own solve is held to its golden records by tests/test_solve_shared.py)"""
    trimmed = 0
    for sw in both(ssd, oracle, depth):
        for i in range(sw.n):
            n, ground, cur = _first(ssd, sw, i)
            for _ in range(rfm.PASSES):
                gates = ssd.surface_gates_from_moments(cur, sm.MIN_POINTS, 2.5, 0.0)
                nxt = ssd.surface_refit_moments_host(sw.cfg, sw.frames[i], sw.labels[i], gates, n, ground, intr=sw.intr)
                assert sm.frame_tuple(nxt) == (n, ground, sm.pad(rfm.refit_np(sw.pts[i], sw.labels[i], gates, n), ssd.MAX_STEPS)), i
                trimmed += sum(int(cur.s[k].m.n) - int(nxt.s[k].m.n) for k in range(n))
                cur = nxt
    assert trimmed > 0


@INPUTS
def test_riser_evidence_and_moments_equal_the_model(ssd, oracle, depth):
    """riser_model on the oracle's record: per riser the oracle's count, exactly, and its mean offset; the riser moments are
    ssd_surface_moments_host over the model's labels, held to surface_model's sums"""
    with_evidence = without = 0
    for sw in both(ssd, oracle, depth):
        ocfg = ob.to_oracle_config(sw.cfg)
        for i in range(sw.n):
            cal = sw.cal_of(i)
            for tol in RISER_TOLS:
                ora = oracle.risers(ocfg, ob.to_oracle_calibration(cal), sw.pts[i], tol, 1)
                labels, off = rm.evidence(sw.cfg, cal, sw.records[i], sw.pts[i], tol)
                assert len(ora) == max((0 if sw.thrown[i] else sw.records[i].n_steps) - 1, 0) and int(labels.max(initial=0)) <= len(ora), i
                for k, (o, (cnt, mean)) in enumerate(zip(ora, rm.counts_and_offsets(labels, off, len(ora)))):
                    assert cnt == o.n_points and abs(mean - o.mean_offset) <= 1e-12, (i, k, cnt, o.n_points)
                    with_evidence += cnt >= RISER_SUPPORT
                    without += cnt < RISER_SUPPORT
                fm = ssd.surface_moments_host(sw.cfg, sw.frames[i], labels, len(ora), 0, intr=sw.intr)
                assert sm.frame_tuple(fm) == (len(ora), 0, sm.pad(sm.moments_np(sw.pts[i], labels, len(ora)), ssd.MAX_STEPS)), i
    assert with_evidence > 10 and without > 10, "risers with evidence and risers without"


@INPUTS
@pytest.mark.parametrize("rule", CLEAR_RULES, ids=["default", "no-margin"])
def test_clearance_equals_the_model(ssd, oracle, depth, rule):
    kept = 0
    for sw in both(ssd, oracle, depth):
        for i in range(sw.n):
            fr, cal = sw.results[i], sw.cal_of(i)
            rec, mask = ssd.clearance_host(sw.cfg, cal, sw.frames[i], fr, 1, cm.rule_of(ssd, rule), intr=sw.intr)
            want = cm.occupants(sw.cfg, cal, fr, sw.pts[i], rule)
            assert np.array_equal(mask.reshape(-1), want), i
            n = 0 if sw.thrown[i] else fr.n_steps
            assert (rec.n_surfaces, rec.ground) == (n, 1 if n else 0)
            assert cm.sums_of_record(rec, ssd.MAX_STEPS) == cm.sums(sw.pts[i], want, ssd.MAX_STEPS), i
            if n == 0:
                assert bytes(rec) == bytes(C.sizeof(ssd.FrameMoments)) and not mask.any()
            kept += int(np.count_nonzero(want))
    assert kept > 1000, "outliers above treads, and the faces where there is no margin"


@INPUTS
@pytest.mark.parametrize("cell", CELLS)
def test_the_tread_grid_equals_the_model(ssd, oracle, depth, cell):
    rule = tg.RULE[:3] + (cell,)
    seen = out = 0
    for sw in both(ssd, oracle, depth):
        for i in range(sw.n):
            fr, cal = sw.results[i], sw.cal_of(i)
            rec = ssd.tread_grid_host(sw.cfg, cal, sw.frames[i], fr, 1, tg.rule_of(ssd, rule), intr=sw.intr)
            n = 0 if sw.thrown[i] else fr.n_steps
            tg.assert_record(ssd, rec, tg.grids(sw.cfg, cal, fr, sw.pts[i], rule), n, 1 if n else 0)
            clear, _ = ssd.clearance_host(sw.cfg, cal, sw.frames[i], fr, 1, cm.rule_of(ssd, rule[:3]), intr=sw.intr, mask=False)
            for k in range(ssd.MAX_STEPS):
                g = tg.grid_of_record(rec, k)
                assert int(g["occ"].sum()) + g["n_occ_out"] == int(clear.s[k].m.n + clear.s[k].n_far), (i, k)
                seen += int(g["seen"].sum())
                out += g["n_seen_out"]
            if n == 0:
                assert bytes(rec) == bytes(C.sizeof(ssd.FrameTreadGrid))
    assert seen > 1000 and (out > 0 or cell == 1.0)


@INPUTS
@pytest.mark.parametrize("rule", POSE_RULES, ids=["default", "tight"])
def test_the_stair_pose_record_equals_the_model(ssd, oracle, depth, rule):
    """every frame against its staircase's map under a prior that is the view's calibration turned by 2 degrees and moved 3 cm"""
    treads = risers = 0
    for sw in both(ssd, oracle, depth):
        maps = sw.stair_maps(ssd)
        priors = [pose_prior(ssd, cal) for cal in sw.cals]
        for i in range(sw.n):
            m, prior = maps[sw.group[i]], priors[sw.view[i]]
            got = spm.record_tuple(ssd.stair_pose_host(sw.cfg, spm.target(ssd, prior, m, sw.intr), sw.frames[i], spm.rule_of(ssd, rule), depth=depth))
            assert got == spm.record_np(sw.cfg, prior, m, sw.pts[i], rule), i
            if m.stairs.n_steps == 0:
                assert got[0] == (0, 0, 0, 0) and not any(v for row in got[1] + got[2] for v in row), "a staircase no view finds: all zero"
            treads += sum(row[0] for row in got[1])
            risers += sum(row[0] for row in got[2])
    assert treads > 10000 and risers > 1000


# ---- the rules' edges: a point exactly on an inequality, made by the rule (tests/sweep_scenes.py) ---------------------------------------------
def _edge_sweeps(ssd, oracle):
    return [ss.sweep(ssd, oracle, depth, ragged) for depth in (False, True) for ragged in (False, True)]


def test_clearance_with_an_occupant_exactly_margin_inside_a_side(ssd, oracle):
    """a margin at which an occupant's squared cross product EQUALS margin^2 times the side's squared length: kept, by both texts"""
    for sw in _edge_sweeps(ssd, oracle):
        at, (margin, p) = ss.first_edge(sw, lambda i: ss.edge_margin(sw.cfg, sw.cal_of(i), sw.results[i], sw.pts[i], *cm.RULE[1:]))
        for rule, kept in (((margin,) + cm.RULE[1:], True), ((float(np.nextafter(margin, 2.0)),) + cm.RULE[1:], False)):
            for i in range(sw.n):
                rec, mask = ssd.clearance_host(sw.cfg, sw.cal_of(i), sw.frames[i], sw.results[i], 1, cm.rule_of(ssd, rule), intr=sw.intr)
                want = cm.occupants(sw.cfg, sw.cal_of(i), sw.results[i], sw.pts[i], rule)
                assert np.array_equal(mask.reshape(-1), want), (i, rule)
                assert cm.sums_of_record(rec, ssd.MAX_STEPS) == cm.sums(sw.pts[i], want, ssd.MAX_STEPS), (i, rule)
                if i == at:
                    assert (want[p] > 0) == kept, "the point on the edge"


def test_the_tread_grid_with_a_point_exactly_lo_from_its_tread_and_on_a_rows_edge(ssd, oracle):
    """a lo that IS a tread point's distance from its surface's height (in its slab: !(d > lo)), and a cell at which v / cell and
    v * (1 / cell) are different rows"""
    for sw in _edge_sweeps(ssd, oracle):
        at_lo, (lo, _) = ss.first_edge(sw, lambda i: ss.edge_lo(sw.cfg, sw.cal_of(i), sw.results[i], sw.pts[i], tg.RULE))
        at_cell, (cell, _) = ss.first_edge(sw, lambda i: ss.edge_cell(sw.cfg, sw.cal_of(i), sw.results[i], sw.pts[i], tg.RULE))
        for rule in ((tg.RULE[0], lo) + tg.RULE[2:], tg.RULE[:3] + (cell,)):
            for i in range(sw.n):
                fr, cal = sw.results[i], sw.cal_of(i)
                rec = ssd.tread_grid_host(sw.cfg, cal, sw.frames[i], fr, 1, tg.rule_of(ssd, rule), intr=sw.intr)
                n = 0 if sw.thrown[i] else fr.n_steps
                tg.assert_record(ssd, rec, tg.grids(sw.cfg, cal, fr, sw.pts[i], rule), n, 1 if n else 0)


@pytest.mark.parametrize("rule", POSE_RULES, ids=["default", "tight"])
def test_the_stair_pose_with_a_point_exactly_reach_from_its_riser(ssd, oracle, rule):
    """a reach at which a riser point's squared cross product EQUALS reach^2 times the edge's squared length: kept, by both texts"""
    for sw in _edge_sweeps(ssd, oracle):
        maps = sw.stair_maps(ssd)
        priors = [pose_prior(ssd, cal) for cal in sw.cals]
        at, (reach, p) = ss.first_edge(sw, lambda i: ss.edge_reach(sw.cfg, priors[sw.view[i]], maps[sw.group[i]], sw.pts[i], rule)
                                       if maps[sw.group[i]].stairs.n_steps else None)
        for r, kept in ((rule[:3] + (reach,), True), (rule[:3] + (float(np.nextafter(reach, 0.0)),), False)):
            for i in range(sw.n):
                m, prior = maps[sw.group[i]], priors[sw.view[i]]
                got = spm.record_tuple(ssd.stair_pose_host(sw.cfg, spm.target(ssd, prior, m, sw.intr), sw.frames[i], spm.rule_of(ssd, r), depth=sw.depth))
                assert got == spm.record_np(sw.cfg, prior, m, sw.pts[i], r), (i, r)
            assert (spm.classes(sw.cfg, priors[sw.view[at]], maps[sw.group[at]].stairs, sw.pts[at], r)[p] >= spm.TREADS) == kept, "the point on the edge"
