"""The stair map on the host (include/ssd_hip.h): the exports and sizes, ssd_tread_grid_add and
ssd_stair_map_from_results on hand-made records, ssd_tread_grid_host against a FOREIGN result - another frame's, and the median map -
held to the numpy restatement of tests/tread_grid_model.py cell by cell, what folding the frames of one camera does to the unseen cells,
and every refusal that needs no GPU.  Judged here, on the host functions, because the device is held to them byte for byte
(tests/test_gpu_stair_map.py).  No GPU needed; no tolerance anywhere."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import camera_drift_model as cd
import clearance_model as cm
import full_width as fw
import ground_model as gm
import oracle_binding as ob
import tread_grid_model as tg
from test_gpu_clearance import _scene_batch

NAMES = ["ssd_tread_grid_add", "ssd_stair_map_from_results", "ssd_enqueue_stair_map", "ssd_enqueue_cameras_stair_map", "ssd_fetch_stair_map",
         "ssd_get_stair_map_time", "ssd_process_host_stair_map", "ssd_process_host_cameras_stair_map"]
U32 = 0xffffffff
SQUARE = [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_stair_map", "enqueue_cameras_stair_map", "fetch_stair_map", "stair_map_time_ms", "process_host_stair_map",
              "process_host_cameras_stair_map"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.tread_grid_add) and callable(ssd.stair_map_from_results)
    assert (ssd.MAX_STAIR_MAPS, ssd.STAIR_MAP_NONE) == (64, 0xffff)
    assert C.sizeof(ssd.StairMap) == 1240 == C.sizeof(ssd.FrameResult) + 8 and ssd.StairMap.ground.offset == 1232
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssd_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in header
    assert "#define SSD_MAX_STAIR_MAPS 64" in header and "#define SSD_STAIR_MAP_NONE 0xffff" in header
    assert "ACROSS accumulating calls that bound is the caller's to keep" in header


# ---- ssd_tread_grid_add ------------------------------------------------------------------------------------------------------------------
def _planes(seed, top_scale=1000):
    rng = np.random.default_rng(seed)
    return dict(seen=rng.integers(0, 5000, (tg.ROWS, tg.COLS)), occ=rng.integers(0, 40, (tg.ROWS, tg.COLS)),
                top=rng.integers(0, top_scale, (tg.ROWS, tg.COLS)), n_seen_out=int(rng.integers(0, 99)), n_occ_out=int(rng.integers(0, 9)),
                top_out=int(rng.integers(0, top_scale)))


def test_add_sums_the_counts_raises_the_tops_and_copies_the_header(ssd):
    a = tg.record_of(ssd, [_planes(1), _planes(2, 50), {}, _planes(3)], 4, ground=1)
    b = tg.record_of(ssd, [_planes(4), _planes(5), _planes(6)], 3, ground=0)
    acc = ssd.FrameTreadGrid()
    assert ssd.tread_grid_add(a, acc) is acc and bytes(acc) == bytes(a), "onto zeros: the record itself"
    ssd.tread_grid_add(b, acc)
    assert (acc.n_surfaces, acc.ground) == (3, 0), "the header is the last record's"
    for k in range(ssd.MAX_STEPS):
        ga, gb, g = tg.grid_of_record(a, k), tg.grid_of_record(b, k), tg.grid_of_record(acc, k)
        for f in ("seen", "occ"):
            assert np.array_equal(g[f], ga[f] + gb[f])
        assert np.array_equal(g["top"], np.maximum(ga["top"], gb["top"]))
        assert (g["n_seen_out"], g["n_occ_out"], g["top_out"]) == (ga["n_seen_out"] + gb["n_seen_out"], ga["n_occ_out"] + gb["n_occ_out"],
                                                                    max(ga["top_out"], gb["top_out"]))
        assert acc.s[k].reserved == 0
    # any order: the counts and tops of a + b + c are those of c + a + b
    c = tg.record_of(ssd, [_planes(7), _planes(8), _planes(9)], 3, ground=0)
    folds = []
    for order in itertools.permutations((a, b, c)):
        acc = ssd.FrameTreadGrid()
        for r in order:
            ssd.tread_grid_add(r, acc)
        folds.append(bytes(acc)[8:])
    assert len(set(folds)) == 1
    # a top below zero never lowers one: the planes start at 0 and are maximised
    low = tg.record_of(ssd, [dict(top=np.full((tg.ROWS, tg.COLS), -5), top_out=-7)], 1)
    acc = ssd.FrameTreadGrid()
    ssd.tread_grid_add(low, acc)
    assert tg.grid_of_record(acc, 0)["top"].max() == 0 and acc.s[0].top_out == 0


@pytest.mark.parametrize("where", ["seen", "occ", "n_seen_out", "n_occ_out"])
def test_add_refuses_a_count_that_would_pass_the_word_and_leaves_acc_untouched(ssd, where):
    L = ssd.lib()
    full, one = _planes(11), {}
    if where in ("seen", "occ"):
        full[where] = full[where].copy()
        full[where][tg.ROWS - 1, tg.COLS - 1] = U32
        one[where] = np.zeros((tg.ROWS, tg.COLS), np.int64)
        one[where][tg.ROWS - 1, tg.COLS - 1] = 1
    else:
        full[where], one[where] = U32, 1
    k = ssd.MAX_STEPS - 1                                                  # the last surface: everything in front of it has been checked
    acc = tg.record_of(ssd, [_planes(12)] * k + [full], ssd.MAX_STEPS, ground=1)
    inc = tg.record_of(ssd, [_planes(13)] * k + [one], 2, ground=0)
    kept = bytes(acc)
    assert L.ssd_tread_grid_add(C.byref(inc), C.byref(acc)) == -5 and b"2^32" in L.ssd_last_error()
    assert bytes(acc) == kept, "a record whole or not at all"
    with pytest.raises(ssd.SsdError):
        ssd.tread_grid_add(inc, acc)
    # exactly 2^32 - 1 is a count like any other
    zero = tg.record_of(ssd, [{}] * ssd.MAX_STEPS, 2, ground=0)
    assert L.ssd_tread_grid_add(C.byref(zero), C.byref(acc)) == 0 and bytes(acc)[8:] == kept[8:]
    assert L.ssd_tread_grid_add(None, C.byref(acc)) == -1 and L.ssd_tread_grid_add(C.byref(inc), None) == -1 and b"null" in L.ssd_last_error()


# ---- ssd_stair_map_from_results ---------------------------------------------------------------------------------------------------------
def _result(ssd, values, status=0):
    """a result of len(values) steps; step k's height and all eight coordinates are values[k] + 16 k + j (exact in a double)"""
    r = cm.hand_result(ssd, [(v + 16.0 * k, [v + 16.0 * k + j for j in range(1, 9)]) for k, v in enumerate(values)], status=status)
    return r


def _fields(m, k):
    return [m.stairs.steps[k].height] + list(m.stairs.steps[k].quad)


def test_the_map_takes_the_mode_of_n_steps_and_the_lower_median_of_every_field(ssd):
    # n_steps 2 three times, 3 twice, 1 once: the mode is 2.  The values of step 0 among the kept: 5, 1, 3 -> the median 3 (odd count)
    rs = [_result(ssd, [5.0, 0.5]), _result(ssd, [9.0, 9.0, 9.0]), _result(ssd, [1.0, 0.25]), _result(ssd, [7.0]),
          _result(ssd, [8.0, 8.0, 8.0]), _result(ssd, [3.0, 0.75])]
    m, used = ssd.stair_map_from_results(rs, ground=7)
    assert (m.stairs.n_steps, m.stairs.status, m.ground, m.reserved, used) == (2, 0, 7, 0, 3)
    assert _fields(m, 0) == [3.0 + j for j in range(9)] and _fields(m, 1) == [16.5 + j for j in range(9)]
    assert bytes(m)[8 + 2 * 72:1232] == bytes(1232 - 8 - 2 * 72), "steps at k >= n_steps are zero"
    # a tie between 2 and 3 goes to the larger; an even count takes the LOWER of the two middle values
    rs.append(_result(ssd, [6.0, 6.0, 6.0]))
    rs.append(_result(ssd, [2.0, 2.0, 2.0]))
    rs.append(_result(ssd, [4.0, 0.0]))
    m, used = ssd.stair_map_from_results(rs)
    assert (m.stairs.n_steps, used, m.ground) == (3, 4, 1)
    assert _fields(m, 0) == [6.0 + j for j in range(9)], "of 2, 6, 8, 9 the lower median is 6"
    # the median is taken field by field: no frame need hold all of a step's medians
    a, b, c = _result(ssd, [1.0]), _result(ssd, [2.0]), _result(ssd, [3.0])
    a.steps[0].height, c.steps[0].quad[7] = 100.0, -100.0
    m, used = ssd.stair_map_from_results([a, b, c])
    assert used == 3 and _fields(m, 0) == [3.0] + [2.0 + j for j in range(1, 8)] + [9.0]
    # any order gives the same bytes
    want = bytes(ssd.stair_map_from_results(rs)[0])
    rng = np.random.default_rng(3)
    for _ in range(6):
        assert bytes(ssd.stair_map_from_results([rs[i] for i in rng.permutation(len(rs))])[0]) == want


def test_the_map_leaves_out_frames_that_threw_overflowed_are_empty_or_not_finite(ssd):
    good = [_result(ssd, [1.0, 1.0]), _result(ssd, [2.0, 2.0]), _result(ssd, [3.0, 3.0])]
    bad = [_result(ssd, [50.0, 50.0], status=ssd.ST_THROW), _result(ssd, [51.0, 51.0], status=ssd.ST_OVERFLOW), ssd.FrameResult(),
           cm.hand_result(ssd, [], n_steps=-1), cm.hand_result(ssd, [], n_steps=ssd.MAX_STEPS + 1)]
    for where in range(9):
        for v in (math.nan, math.inf, -math.inf):
            r = _result(ssd, [52.0, 52.0])
            if where == 0:
                r.steps[1].height = v
            else:
                r.steps[1].quad[where - 1] = v
            bad.append(r)
    m, used = ssd.stair_map_from_results(bad + good + bad)
    assert used == 3 and bytes(m) == bytes(ssd.stair_map_from_results(good)[0]) and _fields(m, 0)[0] == 2.0
    # the other status bits do not disqualify a frame, and a field past n_steps is not read
    odd = _result(ssd, [2.0, 2.0], status=ssd.ST_OOB_PIXEL | ssd.ST_ASSERT)
    odd.steps[2].height = math.nan
    assert ssd.stair_map_from_results([odd])[1] == 1
    # no usable frame
    for rs in ([], bad):
        m, used = ssd.stair_map_from_results(rs, ground=3)
        assert used == 0 and m.stairs.n_steps == 0 and m.ground == 3 and bytes(m)[:1232] == bytes(1232)
    L = ssd.lib()
    out, n = ssd.StairMap(), C.c_int32(5)
    arr = (ssd.FrameResult * 1)()
    assert L.ssd_stair_map_from_results(None, 1, 1, C.byref(out), C.byref(n)) == -1
    assert L.ssd_stair_map_from_results(arr, 1, 1, None, C.byref(n)) == -1
    assert L.ssd_stair_map_from_results(arr, -1, 1, C.byref(out), C.byref(n)) == -1
    assert L.ssd_stair_map_from_results(arr, 1, 1, C.byref(out), None) == 0, "n_used may be left out"


# ---- ssd_tread_grid_host against a foreign result ---------------------------------------------------------------------------------------
def _host_equals_model(ssd, cfg, cal, frame, stairs, rule, ground=1):
    rec = ssd.tread_grid_host(cfg, cal, frame, stairs, ground, tg.rule_of(ssd, rule))
    n = 0 if (stairs.status & 1) else stairs.n_steps
    tg.assert_record(ssd, rec, tg.grids(cfg, cal, stairs, frame, rule), n, 1 if (n and ground) else 0)
    return rec


def _oracle_results(ssd, oracle, cfg, cal, frames):
    return [cm.result_of_oracle(ssd, oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), f)[0]) for f in frames]


def test_the_scene_frames_against_another_frames_result_and_the_median_map(ssd, oracle):
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    cal = trans.constants
    own = _oracle_results(ssd, oracle, cfg, cal, frames)
    assert all(r.n_steps == 3 and r.status == 0 for r in own)
    median, used = ssd.stair_map_from_results(own)
    assert used == 5 and median.stairs.n_steps == 3
    for i, f in enumerate(frames):
        other = own[(i + 1) % len(frames)]
        assert bytes(other) != bytes(own[i]), "the quadrilaterals move from frame to frame"
        rec = _host_equals_model(ssd, cfg, cal, f, other, tg.RULE)
        assert all(tg.grid_of_record(rec, k)["seen"].sum() > 1000 for k in range(3))
        rec = _host_equals_model(ssd, cfg, cal, f, median.stairs, tg.RULE)
        occ = int(tg.grid_of_record(rec, 1)["occ"].sum())
        assert (occ >= 200) if pulled[i][0] == 1 else (occ == 0), "the box on tread 1 is there under the median map as well"
    # a map that threw or has no step: an all-zero record
    thrown = ssd.FrameResult.from_buffer_copy(bytes(own[0]))
    thrown.status |= ssd.ST_THROW
    for dead in (thrown, ssd.FrameResult()):
        assert bytes(ssd.tread_grid_host(cfg, cal, frames[0], dead, 1, tg.rule_of(ssd, tg.RULE))) == bytes(C.sizeof(ssd.FrameTreadGrid))


def test_the_17_surface_frames_against_another_layouts_result(ssd, oracle):
    refs = [fw.reference(ssd, oracle, layout) for layout in fw.FULL_LAYOUTS[:2]]
    frames = [cm.raised(ref)[0] for ref in refs] + [np.array(fw.frame("scatter", 8)), np.array(fw.frame("ordered", 0))]
    cfg, cal = refs[0].cfg, refs[0].cal
    own = _oracle_results(ssd, oracle, cfg, cal, frames)
    assert [r.n_steps for r in own[:3]] == [17, 17, 9] and own[3].n_steps <= 1
    m17, used = ssd.stair_map_from_results(own)
    assert (m17.stairs.n_steps, used) == (17, 2)
    for f in frames:                                                       # the 9-surface frame and the bare ground among them
        rec = _host_equals_model(ssd, cfg, cal, f, m17.stairs, tg.WIDE_RULE)
        assert sum(int(tg.grid_of_record(rec, k)["seen"].sum()) + rec.s[k].n_seen_out for k in range(17)) > 0
    _host_equals_model(ssd, cfg, cal, frames[0], own[2], tg.WIDE_RULE, ground=0)


# ---- folding the frames of one camera ------------------------------------------------------------------------------------------------------
def test_folding_a_cameras_frames_never_adds_an_unseen_cell(ssd, oracle):
    """camera_drift_model.FRAMES (one camera, four seeds and noises) against their median map: a cell's counts in the fold are no less than
    in any single frame, so a cell UNSEEN in the fold is UNSEEN in every frame - a condition that holds by construction, not a measurement"""
    cfg = ssd.default_config(cd.W, cd.H)
    frames, cal = [], None
    for seed, sigma in cd.FRAMES:
        sc = gm.scene(ssd, "steps", seed=seed, sigma=sigma)
        cal = cal or ssd.transformation_for_scene(sc).constants
        frames.append(ssd.synth_host([sc])[0])
    own = _oracle_results(ssd, oracle, cfg, cal, frames)
    m, used = ssd.stair_map_from_results(own)
    assert used == len(frames) and m.stairs.n_steps == 3
    rule = tg.rule_of(ssd, tg.RULE)
    singles = [ssd.tread_grid_host(cfg, cal, f, m.stairs, m.ground, rule) for f in frames]
    folded = ssd.FrameTreadGrid()
    for g in singles:
        ssd.tread_grid_add(g, folded)
    for order in ((3, 1, 0, 2), (2, 3, 1, 0)):
        again = ssd.FrameTreadGrid()
        for i in order:
            ssd.tread_grid_add(singles[i], again)
        assert bytes(again) == bytes(folded)
    for support in (1, tg.RECIPE_MIN_SEEN):
        sol = ssd.tread_grid_solve(folded, m.stairs, rule, support, support)
        each = [ssd.tread_grid_solve(g, m.stairs, rule, support, support) for g in singles]
        for k in range(3):
            assert sol.s[k].n_unseen <= min(e.s[k].n_unseen for e in each), (support, k)
            fs = np.ctypeslib.as_array(sol.s[k].state)
            for e in each:
                assert not np.any((fs == tg.UNSEEN) & (np.ctypeslib.as_array(e.s[k].state) != tg.UNSEEN))
            tg.assert_solved(sol.s[k], tg.solve(tg.grid_of_record(folded, k), m.stairs.steps[k].quad, tg.RULE, support, support))
    for k in range(3):
        gf = tg.grid_of_record(folded, k)
        assert gf["seen"].sum() + gf["n_seen_out"] == sum(tg.grid_of_record(g, k)["seen"].sum() + g.s[k].n_seen_out for g in singles)
        assert gf["seen"].sum() > 4 * 2000


def _recorded(name):
    """'NAME = a alone, b folded, c folded with scaled supports' of profiles/stair_map_accuracy.txt -> (a, b, c)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "stair_map_accuracy.txt")
    for line in open(path):
        if line.startswith(name + " = "):
            return tuple(int(part.split()[0]) for part in line.split(" = ")[1].split(","))
    raise AssertionError(name)


def test_the_cells_hidden_behind_the_box_are_seen_in_the_fold(ssd, oracle):
    """the recorded recipe (tools/stair_map_accuracy.py, profiles/stair_map_accuracy.txt), four frames of one camera of which frame 0
    carries the box on tread 1: alone, under its own result, frame 0 leaves cells of tread 1 UNSEEN behind the box; folded over the four
    frames against their median map no cell of tread 1 is UNSEEN, the box is still OCCUPIED, and the other treads are as they were"""
    from test_labels import expected_labels
    cfg = ssd.default_config(cd.W, cd.H)
    frames, own, cal = [], [], None
    for i, (seed, sigma) in enumerate(cd.FRAMES):
        sc = gm.scene(ssd, "steps", seed=seed, sigma=sigma)
        cal = cal or ssd.transformation_for_scene(sc).constants
        frame = ssd.synth_host([sc])[0]
        if i == 0:
            res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), frame)[0]
            frame = cm.patched(cfg, cal, cm.result_of_oracle(ssd, res), frame, expected_labels(oracle, cfg, cal, res, frame), 1)[0]
        frames.append(frame)
    own = _oracle_results(ssd, oracle, cfg, cal, frames)
    m, used = ssd.stair_map_from_results(own)
    rule, s = tg.rule_of(ssd, cm.RULE + (tg.RECIPE_CELL,)), tg.RECIPE_MIN_SEEN
    folded = ssd.FrameTreadGrid()
    for f in frames:
        ssd.tread_grid_add(ssd.tread_grid_host(cfg, cal, f, m.stairs, m.ground, rule), folded)
    alone = ssd.tread_grid_solve(ssd.tread_grid_host(cfg, cal, frames[0], own[0], 1, rule), own[0], rule, s, s)
    plain = ssd.tread_grid_solve(folded, m.stairs, rule, s, s)
    scaled = ssd.tread_grid_solve(folded, m.stairs, rule, 4 * s, 4 * s)
    assert (alone.s[1].n_unseen, plain.s[1].n_unseen, scaled.s[1].n_unseen) == _recorded("one_camera_4_unseen_tread_1")
    assert (alone.s[1].n_occupied, plain.s[1].n_occupied, scaled.s[1].n_occupied) == _recorded("one_camera_4_occupied_tread_1")
    assert alone.s[1].n_unseen > 0 and plain.s[1].n_unseen == 0 and scaled.s[1].n_unseen == 0
    assert plain.s[1].n_occupied >= 1 and scaled.s[1].n_occupied >= 1 and plain.s[1].foothold == 1
    for k in (0, 2):
        assert bytes(plain.s[k].state) == bytes(alone.s[k].state) == bytes(scaled.s[k].state) and plain.s[k].n_occupied == 0


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------------------------
def test_the_device_entry_points_without_a_handle(ssd):
    L = ssd.lib()
    dummy, rule = C.c_void_p(4096), ssd.TreadGridRule()
    m = (ssd.StairMap * 1)()
    assert L.ssd_enqueue_stair_map(None, dummy, 12 * 8, 1, None, 0, m, 1, None, C.byref(rule), 0, dummy) == -1 and b"null" in L.ssd_last_error()
    assert L.ssd_enqueue_cameras_stair_map(None, dummy, 12 * 8, 1, None, 0, m, 1, None, C.byref(rule), 0, dummy) == -1
    assert L.ssd_fetch_stair_map(None, None) == -1
    assert L.ssd_get_stair_map_time(None, C.byref(C.c_float(0.0))) == -1
    r1, o1 = (ssd.FrameResult * 1)(), (ssd.FrameFootholds * 1)()
    assert L.ssd_process_host_stair_map(None, dummy, 1, 0, m, 1, None, C.byref(rule), 1, 1, 0.0, 0.0, r1, None, o1) == -1
    assert L.ssd_process_host_cameras_stair_map(None, dummy, 1, None, 0, m, 1, None, C.byref(rule), 1, 1, 0.0, 0.0, r1, None, o1) == -1
