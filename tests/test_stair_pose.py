"""The stair pose on the host (include/ssd_hip.h): the exports and sizes, ssd_stair_pose_host held to the numpy
restatement of tests/stair_pose_model.py byte for byte - on the scene frames, the 17-surface frames, maps that give nothing, a point on
either side of every inequality, a far point -, ssd_stair_pose_add in Python integers, ssd_stair_pose_solve on hand-built clouds whose
points lie exactly on the map's planes, and the recorded recipe (profiles/stair_pose_accuracy.txt).  Judged here, on the host functions,
because the device is held to them byte for byte (tests/test_gpu_stair_pose.py).  No GPU needed."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import clearance_model as cm
import clouds
import full_width as fw
import ground_model as gm
import oracle_binding as ob
import stair_pose_model as spm
from test_gpu_clearance import _scene_batch

NAMES = ["ssd_stair_pose_host", "ssd_stair_pose_add", "ssd_stair_pose_solve", "ssd_enqueue_stair_pose", "ssd_fetch_stair_pose_moments",
         "ssd_fetch_stair_pose", "ssd_get_stair_pose_time", "ssd_process_host_stair_pose"]
WIDE_RULE = (0.03, 0.01, 0.02, 0.01)          # the full-width frames': their steps rise 0.06 m, their faces are 2 mm thick


def test_the_entry_points_are_exported_and_wrapped(ssd):
    for n in NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_stair_pose", "fetch_stair_pose_moments", "fetch_stair_pose", "stair_pose_time_ms", "process_host_stair_pose", "locate_camera"):
        assert callable(getattr(ssd.Detector, m))
    assert callable(ssd.stair_pose_host) and callable(ssd.stair_pose_add) and callable(ssd.stair_pose_solve)
    assert C.sizeof(ssd.StairPoseRule) == 32 and C.sizeof(ssd.StairPoseMoments) == 3008 == 2 * C.sizeof(ssd.FrameMoments)
    assert C.sizeof(ssd.StairPoseTarget) == C.sizeof(ssd.Camera) + 1240 and ssd.StairPoseTarget.map.offset == C.sizeof(ssd.Camera)
    assert C.sizeof(ssd.StairPose) == 8 + 8 + 16 + 8 * 17 + C.sizeof(ssd.Calibration) and ssd.StairPose.cal.offset == 168
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssd_hip.h")).read()
    for n in NAMES:
        assert "int %s(" % n in header
    assert "#define SSD_SP_OBSERVABLE %s" % repr(ssd.SP_OBSERVABLE).replace("e-0", "e-") in header
    for name, v in zip(("MARGIN", "BAND", "CLEAR", "REACH"), spm.RULE):
        assert "#define SSD_SP_%s %g" % (name, v) in header
    r = ssd.StairPoseRule()
    assert (r.margin, r.band, r.clear, r.reach) == spm.RULE == (ssd.SP_MARGIN, ssd.SP_BAND, ssd.SP_CLEAR, ssd.SP_REACH)
    assert "the expected dof is 5" in header


# ---- ssd_stair_pose_host against the model ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_sets(ssd, oracle):
    """the five scene frames as vertices and as depth, the median map of the oracle's results, the true prior and an offset one"""
    out = {}
    for depth in (False, True):
        cfg, trans, intr, frames, _ = _scene_batch(ssd, oracle, depth)
        cal = trans.constants
        pts = [ssd.deproject_host(intr, f) if depth else f for f in frames]
        res = [cm.result_of_oracle(ssd, oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), p)[0]) for p in pts]
        stair_map, used = ssd.stair_map_from_results(res)
        assert used == 5 and stair_map.stairs.n_steps == 3
        off = spm.moved(ssd, cal, (0.5 * spm.DEG, 0.0, 1.0 * spm.DEG), (0.0, 0.015, 0.01), (0.0, 0.6, 0.2))
        out[depth] = dict(cfg=cfg, intr=intr, frames=frames, pts=pts, map=stair_map, priors=[cal, off])
    return out


@pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])
def test_the_scene_frames_against_the_median_map_equal_the_model(ssd, scene_sets, depth):
    d = scene_sets[depth]
    seen = set()
    for which, cal in enumerate(d["priors"]):
        t = spm.target(ssd, cal, d["map"], d["intr"] if depth else None)
        for f, p in zip(d["frames"], d["pts"]):
            got = spm.record_tuple(ssd.stair_pose_host(d["cfg"], t, f, depth=depth))
            assert got == spm.record_np(d["cfg"], cal, d["map"], p), which
            assert got[0] == (3, 1, 2, 0)
            assert all(got[1][k][0] > 1000 for k in range(3)) and all(got[2][i][0] > 500 for i in range(2)), "every tread and riser is seen"
            assert got[1][3:] == [[0] * 11] * 14 and got[2][2:] == [[0] * 11] * 15, "classes past the counts are zero"
            seen.add(repr(got))
    assert len(seen) >= 8, "the frames and the priors give different records"


@pytest.fixture(scope="module")
def wide(ssd, oracle):
    """the 17-surface frame of tests/full_width.py (every layout places the same points), its oracle record as the 17-surface map"""
    ref = fw.reference(ssd, oracle, "scatter")
    assert not ref.unlimited and ref.res.n_steps == ssd.MAX_STEPS
    stair_map = ssd.StairMap()
    C.memmove(C.byref(stair_map.stairs), C.byref(cm.result_of_oracle(ssd, ref.res)), C.sizeof(ssd.FrameResult))
    stair_map.ground = ref.ground
    return ref, stair_map


def test_the_full_width_frames_fill_all_17_treads_and_16_risers(ssd, oracle, wide):
    ref, stair_map = wide
    t = spm.target(ssd, ref.cal, stair_map)
    want = spm.record_np(ref.cfg, ref.cal, stair_map, ref.xyz, WIDE_RULE)
    assert want[0] == (17, 1, 16, 0)
    assert all(want[1][k][0] > 0 for k in range(17)) and all(want[2][i][0] > 0 for i in range(16)), "the model alone: no class is empty"
    assert want[2][16] == [0] * 11
    for layout in ("scatter", "ordered"):
        xyz = fw.reference(ssd, oracle, layout).xyz
        assert spm.record_tuple(ssd.stair_pose_host(ref.cfg, t, xyz, spm.rule_of(ssd, WIDE_RULE))) == want, layout


def test_a_thrown_an_empty_and_a_one_step_map(ssd, scene_sets):
    d = scene_sets[False]
    cal, frame = d["priors"][0], d["frames"][4]
    thrown, empty, one = (ssd.StairMap.from_buffer_copy(d["map"]) for _ in range(3))
    thrown.stairs.status |= ssd.ST_THROW
    empty.stairs.n_steps = 0
    one.stairs.n_steps = 1
    for m in (thrown, empty):
        rec = ssd.stair_pose_host(d["cfg"], spm.target(ssd, cal, m), frame)
        assert bytes(rec) == bytes(C.sizeof(ssd.StairPoseMoments)), "all zero, the headers too"
        assert spm.record_tuple(rec) == spm.record_np(d["cfg"], cal, m, frame)
    got = spm.record_tuple(ssd.stair_pose_host(d["cfg"], spm.target(ssd, cal, one), frame))
    assert got == spm.record_np(d["cfg"], cal, one, frame) and got[0] == (1, 1, 0, 0)
    assert got[1][0][0] > 1000 and got[2] == [[0] * 11] * 17, "one step: a tread, no riser"
    one.ground = 0
    assert spm.record_tuple(ssd.stair_pose_host(d["cfg"], spm.target(ssd, cal, one), frame))[0] == (1, 0, 0, 0)
    one.ground = -7
    assert spm.record_tuple(ssd.stair_pose_host(d["cfg"], spm.target(ssd, cal, one), frame))[0] == (1, 1, 0, 0)


def _unit_case(ssd, base=1.0):
    """identity calibration, the camera at the world's origin: ex = x, ey = y, ez = z, exactly.  Step 0 at height `base` over (0, 0) ..
    (1, 1), step 1 at base + 1 over (0, 1) .. (1, 2); riser 0 under the edge (0, 1) -> (1, 1).  The rule in binary fractions: margin,
    band, clear 1/8, reach 1/4."""
    cfg = ssd.default_config(4, 4)
    cfg.x_min, cfg.x_max, cfg.y_min, cfg.y_max = -0.25, 4.0, -4.0, 4.0
    cal = clouds.calibration(ssd, 0.0).constants
    st = cm.hand_result(ssd, [(base, [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0]), (base + 1.0, [0.0, 1.0, 1.0, 1.0, 0.0, 2.0, 1.0, 2.0])])
    stair_map = ssd.StairMap()
    C.memmove(C.byref(stair_map.stairs), C.byref(st), C.sizeof(ssd.FrameResult))
    stair_map.ground = 1
    return cfg, cal, stair_map, (0.125, 0.125, 0.125, 0.25)


def _up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def _down(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


# (x, y, z, the class the rule's text gives: tread k, 17 + riser i, -1 none) - a point on each inequality's edge and its neighbour
EDGES = [
    (0.5, 0.5, 1.125, 0), (0.5, 0.5, _up(1.125), -1), (0.5, 0.5, 0.875, 0), (0.5, 0.5, _down(0.875), -1),            # !(|ez - h| > band)
    (0.5, 0.125, 1.0, 0), (0.5, _down(0.125), 1.0, -1), (0.5, 0.875, 1.0, 0), (0.5, _up(0.875), 1.0, -1),           # c c >= margin^2 L2
    (0.125, 0.5, 1.0, 0), (_down(0.125), 0.5, 1.0, -1), (0.875, 0.5, 1.0, 0), (_up(0.875), 0.5, 1.0, -1),
    (0.5, 1.5, 2.0, 1), (0.5, 1.5, 2.125, 1), (0.5, 1.5, _up(2.125), -1),                                           # the upper tread
    (0.5, 1.0, 1.125, -1), (0.5, 1.0, _up(1.125), 17), (0.5, 1.0, 1.875, -1), (0.5, 1.0, _down(1.875), 17),          # ez > h_i + clear && ez < h_(i+1) - clear
    (0.5, 1.25, 1.5, 17), (0.5, _up(1.25), 1.5, -1), (0.5, 0.75, 1.5, 17), (0.5, _down(0.75), 1.5, -1),              # c c <= reach^2 L2
    (0.0, 1.0, 1.5, 17), (_down(0.0), 1.0, 1.5, -1), (1.0, 1.0, 1.5, 17), (_up(1.0), 1.0, 1.5, -1),                   # t >= 0 && t <= L2
    (-0.25, 1.0, 1.5, -1),                                                                                        # on the measuring range's edge
    (0.5, 0.875, 1.125, 0), (0.5, 0.875, _up(1.125), 17),                                                          # a tread goes before a riser
]


def test_a_point_on_each_inequalitys_edge_in_both_directions(ssd):
    cfg, cal, stair_map, rule = _unit_case(ssd)
    t = spm.target(ssd, cal, stair_map)
    for x, y, z, want in EDGES:
        frame = np.zeros((4, 4, 3), np.float32)
        frame[1, 2] = (x, y, z)
        assert [float(v) for v in frame[1, 2]] == [x, y, z], "the case's values are float32 values"
        model = spm.classes(cfg, cal, stair_map.stairs, frame, rule)
        assert sorted(set(model.tolist())) == sorted({-1, want}), (x, y, z)
        got = spm.record_tuple(ssd.stair_pose_host(cfg, t, frame, spm.rule_of(ssd, rule)))
        assert got == spm.record_np(cfg, cal, stair_map, frame, rule), (x, y, z)
        counts = {k: got[1][k][0] for k in range(17)}
        counts.update({17 + i: got[2][i][0] for i in range(16)})
        assert {c for c, n in counts.items() if n} == ({want} if want >= 0 else set()), (x, y, z)
    # the measuring range is open: just inside its edge a riser point counts
    frame = np.zeros((4, 4, 3), np.float32)
    frame[0, 0] = (_up(-0.25), 1.0, 1.5)
    wide_map = ssd.StairMap.from_buffer_copy(stair_map)
    wide_map.stairs.steps[1].quad[0] = -1.0
    got = spm.record_tuple(ssd.stair_pose_host(cfg, spm.target(ssd, cal, wide_map), frame, spm.rule_of(ssd, rule)))
    assert got == spm.record_np(cfg, cal, wide_map, frame, rule) and got[2][0][0] == 1
    frame[0, 0, 0] = -0.25
    assert spm.record_tuple(ssd.stair_pose_host(cfg, spm.target(ssd, cal, wide_map), frame, spm.rule_of(ssd, rule)))[2][0][0] == 0
    # z > 0: with the ground AT the camera's height its band holds z = +tiny, and z = 0 is no point
    cfg0, cal0, map0, rule0 = _unit_case(ssd, 0.0)
    for z, n in ((1e-30, 1), (0.0, 0), (-1e-30, 0)):
        frame = np.zeros((4, 4, 3), np.float32)
        frame[3, 3] = (0.5, 0.5, z)
        got = spm.record_tuple(ssd.stair_pose_host(cfg0, spm.target(ssd, cal0, map0), frame, spm.rule_of(ssd, rule0)))
        assert got == spm.record_np(cfg0, cal0, map0, frame, rule0) and got[1][0][0] == n, z
    # a zero-length edge and a NaN corner take nothing
    for bad in (1.0, float("nan")):
        broken = ssd.StairMap.from_buffer_copy(stair_map)
        broken.stairs.steps[1].quad[0] = bad
        broken.stairs.steps[1].quad[2] = bad if bad == bad else 1.0
        frame = np.zeros((4, 4, 3), np.float32)
        frame[2, 2] = (1.0, 1.0, 1.5)
        got = spm.record_tuple(ssd.stair_pose_host(cfg, spm.target(ssd, cal, broken), frame, spm.rule_of(ssd, rule)))
        assert got == spm.record_np(cfg, cal, broken, frame, rule) and got[2][0][0] == 0, bad


def test_a_far_point_goes_into_n_far(ssd):
    cfg, cal, stair_map, rule = _unit_case(ssd)
    cfg.x_max = 64.0
    for k in range(2):                                              # both treads and the edge reach out to x = 32
        for j in (2, 6):
            stair_map.stairs.steps[k].quad[j] = 32.0
    frame = np.zeros((4, 4, 3), np.float32)
    frame[0, 0] = (16.0, 0.5, 1.0)                                  # q = 2^20 exactly: far, on tread 0
    frame[0, 1] = (16.0 - 2.0 ** -16, 0.5, 1.0)                      # q = 2^20 - 1: the last near value
    frame[1, 0] = (20.0, 1.0, 1.5)                                  # far, on riser 0
    frame[1, 1] = (2.0, 1.5, 2.0)                                   # near, on tread 1
    got = spm.record_tuple(ssd.stair_pose_host(cfg, spm.target(ssd, cal, stair_map), frame, spm.rule_of(ssd, rule)))
    assert got == spm.record_np(cfg, cal, stair_map, frame, rule)
    assert (got[1][0][0], got[1][0][10]) == (1, 1) and got[1][0][1] == 2 ** 20 - 1
    assert (got[2][0][0], got[2][0][10]) == (0, 1) and got[2][0][1:10] == [0] * 9, "a far point is counted, not summed"
    assert (got[1][1][0], got[1][1][10]) == (1, 0)


def test_the_host_statements_refusals(ssd, scene_sets):
    L = ssd.lib()
    d = scene_sets[False]
    t = spm.target(ssd, d["priors"][0], d["map"])
    out = ssd.StairPoseMoments()
    frame = np.ascontiguousarray(d["frames"][0])
    ptr = frame.ctypes.data_as(C.c_void_p)

    def call(cfg=d["cfg"], target=t, inp=0, f=ptr, rule=ssd.StairPoseRule(), o=out):
        return L.ssd_stair_pose_host(C.byref(cfg) if cfg else None, C.byref(target) if target else None, inp, f, C.byref(rule) if rule else None,
                                     C.byref(o) if o else None)
    assert call() == 0
    assert call(cfg=None) == call(target=None) == call(f=None) == call(o=None) == call(rule=None) == call(inp=2) == -1
    nan = float("nan")
    for bad in ((-0.01, 0.03, 0.03, 0.04), (1.5, 0.03, 0.03, 0.04), (0.03, 0.0, 0.03, 0.04), (0.03, 1.5, 0.03, 0.04), (0.03, 0.03, 0.0, 0.04),
                (0.03, 0.03, 1.5, 0.04), (0.03, 0.03, 0.03, 0.0), (0.03, 0.03, 0.03, 1.5), (nan, 0.03, 0.03, 0.04), (0.03, nan, 0.03, 0.04),
                (0.03, 0.03, nan, 0.04), (0.03, 0.03, 0.03, nan)):
        assert call(rule=ssd.StairPoseRule(*bad)) == -1, bad
    for good in ((0.0, 1.0, 1.0, 1.0), (1.0, 0.5, 0.5, 0.5)):
        assert call(rule=ssd.StairPoseRule(*good)) == 0, good
    for n in (-1, ssd.MAX_STEPS + 1):
        bad_map = ssd.StairMap.from_buffer_copy(d["map"])
        bad_map.stairs.n_steps = n
        assert call(target=spm.target(ssd, d["priors"][0], bad_map)) == -1
        assert L.ssd_stair_pose_solve(C.byref(out), C.byref(spm.target(ssd, d["priors"][0], bad_map)), 1, 0.0, C.byref(ssd.StairPose())) == -1
    assert call(inp=1) == -1 and b"intrinsics" in L.ssd_last_error(), "depth input without the prior's intrinsics"
    assert L.ssd_stair_pose_solve(None, C.byref(t), 1, 0.0, C.byref(ssd.StairPose())) == -1
    assert L.ssd_stair_pose_solve(C.byref(out), None, 1, 0.0, C.byref(ssd.StairPose())) == -1
    assert L.ssd_stair_pose_solve(C.byref(out), C.byref(t), 1, 0.0, None) == -1
    assert L.ssd_stair_pose_solve(C.byref(out), C.byref(t), 1, nan, C.byref(ssd.StairPose())) == -1


# ---- ssd_stair_pose_add -----------------------------------------------------------------------------------------------------------------
def _random_record(ssd, seed, n_steps=4, ground=1):
    rng = np.random.default_rng(seed)
    rows = lambda n: [[int(v) for v in rng.integers(-2 ** 40, 2 ** 40, 11)] for _ in range(n)]
    return spm.record_of(ssd, (n_steps, ground, n_steps - 1, 0), rows(n_steps), rows(n_steps - 1))


def test_add_sums_every_word_and_copies_the_headers_in_every_order(ssd):
    recs = [_random_record(ssd, 1), _random_record(ssd, 2, 17, 0), _random_record(ssd, 3, 2)]
    acc = ssd.StairPoseMoments()
    assert ssd.stair_pose_add(recs[0], acc) is acc and bytes(acc) == bytes(recs[0]), "onto zeros: the record itself"
    sums = set()
    for order in itertools.permutations(recs):
        acc = ssd.StairPoseMoments()
        for r in order:
            ssd.stair_pose_add(r, acc)
        assert spm.record_tuple(acc) == spm.fold_py([spm.record_tuple(r) for r in order])
        assert spm.record_tuple(acc)[0] == spm.record_tuple(order[-1])[0], "the headers are the last record's"
        sums.add(repr(spm.record_tuple(acc)[1:]))
    assert len(sums) == 1, "the sums do not depend on the order"


@pytest.mark.parametrize("half, word", [("treads", 0), ("treads", 3), ("treads", 9), ("treads", 10), ("risers", 0), ("risers", 2), ("risers", 6),
                                        ("risers", 10)])
def test_add_refuses_a_sum_that_would_leave_int64_and_leaves_acc_untouched(ssd, half, word):
    L = ssd.lib()
    k = 16 if half == "treads" else 15                              # the last class: everything in front of it has been checked
    for sign in (1, -1):
        acc, inc = _random_record(ssd, 5, 17), _random_record(ssd, 6, 3, 0)
        for rec, v in ((acc, spm.INT64_MAX if sign > 0 else spm.INT64_MIN), (inc, sign)):
            sm = getattr(rec, half).s[k]
            if word == 0:
                sm.m.n = v
            elif word < 4:
                sm.m.s[word - 1] = v
            elif word < 10:
                sm.m.ss[word - 4] = v
            else:
                sm.n_far = v
        kept = bytes(acc)
        assert spm.fold_py([spm.record_tuple(acc), spm.record_tuple(inc)]) is None
        assert L.ssd_stair_pose_add(C.byref(inc), C.byref(acc)) == -5 and b"int64" in L.ssd_last_error()
        assert bytes(acc) == kept, "a record whole or not at all"
        with pytest.raises(ssd.SsdError):
            ssd.stair_pose_add(inc, acc)
        zero = ssd.StairPoseMoments()                               # the extreme value itself is a sum like any other
        assert L.ssd_stair_pose_add(C.byref(zero), C.byref(acc)) == 0 and bytes(acc)[8:1504] == kept[8:1504] and bytes(acc)[1512:] == kept[1512:]
    assert L.ssd_stair_pose_add(None, C.byref(acc)) == -1 and L.ssd_stair_pose_add(C.byref(inc), None) == -1 and b"null" in L.ssd_last_error()


# ---- ssd_stair_pose_solve on hand-built, noise-free clouds --------------------------------------------------------------------------------
CW, CH = 160, 120
RISE = 0.16
# Every coordinate is summed as q = rint(v * 2^16): off by at most half a quantum, 2^-17 m.  A residual n . e with |n| = 1 is then off by
# at most sqrt(3) 2^-17 m, a fitted plane offset - a mean of residuals - by no more, and a point's recovered place compounds at most the
# three families of planes that fix it (the treads' height, the risers' place, the rotation over the cloud's half-extent):
# 3 sqrt(3) 2^-17 = 3.96e-5 m.  Derived, not tuned.  1e-7 m on top: the float32 frame holds a point of a plane within 6e-8 m of it.
QUANT = 3.0 * math.sqrt(3.0) * 2.0 ** -17 + 1e-7


def _straight(ssd, second_edge=None):
    """a 3-step map on exact planes and the cloud on it: treads 0.3 m deep over x -0.4 .. 0.4, risers under the front edges of steps 1
    and 2 (second_edge: another front edge FL, FR for step 2, and the face under it) -> (cfg, true calibration, map, frame)"""
    steps, planes, faces = [], [], []
    for k in range(3):
        y0 = 0.2 + 0.3 * k
        steps.append((RISE * k, [-0.4, y0, 0.4, y0, -0.4, y0 + 0.3, 0.4, y0 + 0.3]))
        planes.append((RISE * k, 1500, (-0.38, 0.38), (y0 + 0.04, y0 + 0.26)))
    if second_edge is not None:
        (flx, fly), (frx, fry) = second_edge
        steps[2] = (RISE * 2, [flx, fly, frx, fry, -0.4, 1.1, 0.4, 1.1])
    for i in range(2):
        q = steps[i + 1][1]
        s, z = np.meshgrid(np.linspace(0.05, 0.95, 40), np.linspace(RISE * i + 0.05, RISE * (i + 1) - 0.05, 12))
        faces.append(np.stack([q[0] + s.ravel() * (q[2] - q[0]), q[1] + s.ravel() * (q[3] - q[1]), z.ravel()], 1))
    cfg = ssd.default_config(CW, CH)
    # the cloud in the external world (tests/clouds.py places it on the frame's pixels), then into the camera of the 3-step scene's pose -
    # 1 m up, pitched 50 degrees: p = A^T (w - b), w = e - (t2, world_z), r2 the identity
    truth = ssd.transformation_for_scene(gm.scene(ssd, "steps")).constants
    assert list(truth.r2) == [1.0, 0.0, 0.0, 1.0]
    world = clouds.cloud(planes, CW, CH, extra=np.concatenate(faces), seed=3, z_shift=0.0).astype(np.float64).reshape(-1, 3)
    held = np.any(world != 0.0, axis=1)
    A, b = np.array(list(truth.a)).reshape(3, 3), np.array(list(truth.b))
    cam = (world - np.array([truth.t2[0], truth.t2[1], truth.world_z]) - b) @ A
    assert cam[held, 2].min() > 0.3
    frame = np.where(held[:, None], cam, 0.0).astype(np.float32).reshape(CH, CW, 3)
    st = cm.hand_result(ssd, steps)
    stair_map = ssd.StairMap()
    C.memmove(C.byref(stair_map.stairs), C.byref(st), C.sizeof(ssd.FrameResult))
    stair_map.ground = 1
    return cfg, truth, stair_map, frame


def _apply(cal, pts):
    T, c = spm.affine_of(cal)
    return pts @ T.T + c


def _recovered(cal, truth, frame):
    """the recovered calibration against the truth over the cloud's points: (the largest error along the going and in height, the
    spread of the error along the edges - a straight staircase leaves a common shift along them open)"""
    pts = frame.reshape(-1, 3).astype(np.float64)
    pts = pts[pts[:, 2] > 0]
    d = _apply(cal, pts) - _apply(truth, pts)
    return float(np.abs(d[:, 1:]).max()), float(d[:, 0].max() - d[:, 0].min())


def test_a_translation_along_the_riser_normal_and_in_height_is_recovered_in_one_pass(ssd):
    cfg, truth, stair_map, frame = _straight(ssd)
    prior = spm.moved(ssd, truth, (0.0, 0.0, 0.0), (0.0, 0.02, 0.015))
    assert _recovered(prior, truth, frame)[0] > 0.019
    cals, poses = spm.chain_host(ssd, cfg, [frame], prior, stair_map, passes=1, min_points=100)
    p = poses[0]
    assert (p.status, p.dof, p.treads_used, p.risers_used) == (ssd.GF_OK, 5, 0b111, 0b11)
    err, spread = _recovered(cals[0], truth, frame)
    print("one pass: error %.3e m, spread along the edges %.3e m, bound %.3e m" % (err, spread, QUANT))
    assert err <= QUANT and spread <= QUANT
    assert abs(p.translation[1] + 0.02) <= QUANT and abs(p.translation[2] + 0.015) <= QUANT and p.translation[0] == 0.0
    assert p.rms_before > 0.015 and p.rms_after <= QUANT


def test_yaw_and_pitch_are_recovered_in_three_chained_passes(ssd):
    cfg, truth, stair_map, frame = _straight(ssd)
    centre = (0.0, 0.65, 0.16)
    prior = spm.moved(ssd, truth, (1.0 * spm.DEG, 0.0, 2.0 * spm.DEG), (0.0, 0.0, 0.0), centre)
    assert _recovered(prior, truth, frame)[0] > 0.01
    cals, poses = spm.chain_host(ssd, cfg, [frame], prior, stair_map, passes=3, min_points=100)
    assert [p.status for p in poses] == [ssd.GF_OK] * 3 and [p.dof for p in poses] == [5] * 3
    errs = [_recovered(c, truth, frame) for c in cals]
    print("three passes: errors %s m, bound %.3e m" % (", ".join("%.3e / %.3e" % e for e in errs), QUANT))
    assert errs[2][0] <= QUANT and errs[2][1] <= QUANT, "to the quantisation over the cloud's half-extent"
    assert errs[0][0] < 0.25 * _recovered(prior, truth, frame)[0], "the first pass does most of it"


def test_the_degrees_of_freedom(ssd):
    cfg, truth, stair_map, frame = _straight(ssd)
    t = spm.target(ssd, truth, stair_map)
    rec = ssd.stair_pose_host(cfg, t, frame)
    p = ssd.stair_pose_solve(rec, t, 100)
    assert (p.status, p.dof) == (ssd.GF_OK, 5), "parallel risers: the shift along the edges stays open"
    assert p.eig[0] <= spm.ROUNDING * p.eig[5] and p.eig[1] > 1e-3 * p.eig[5]
    assert list(p.eig) == sorted(p.eig)
    # treads only: the risers' classes emptied
    flat = ssd.StairPoseMoments.from_buffer_copy(rec)
    C.memset(C.byref(flat.risers.s), 0, C.sizeof(flat.risers.s))
    p = ssd.stair_pose_solve(flat, t, 100)
    assert (p.status, p.dof, p.treads_used, p.risers_used) == (ssd.GF_OK, 3, 0b111, 0)
    # two perpendicular risers: step 2's front edge runs along the going
    cfg2, truth2, map2, frame2 = _straight(ssd, second_edge=((0.0, 1.05), (0.0, 0.85)))
    t2 = spm.target(ssd, truth2, map2)
    rec2 = ssd.stair_pose_host(cfg2, t2, frame2)
    assert rec2.risers.s[0].m.n >= 100 and rec2.risers.s[1].m.n >= 100
    p = ssd.stair_pose_solve(rec2, t2, 100)
    assert (p.status, p.dof, p.risers_used) == (ssd.GF_OK, 6, 0b11)
    # FEW below min_points: cal is the prior, the doubles are 0
    p = ssd.stair_pose_solve(rec, t, 100000)
    assert (p.status, p.dof, p.treads_used, p.risers_used, p.n) == (ssd.GF_FEW, 0, 0, 0, 0)
    assert bytes(p.cal) == bytes(truth) and list(p.rotation) + list(p.translation) + list(p.eig) == [0.0] * 12
    # a class takes part from min_points on, exactly
    n1 = int(rec.risers.s[1].m.n)
    assert ssd.stair_pose_solve(rec, t, n1).risers_used & 2 and not ssd.stair_pose_solve(rec, t, n1 + 1).risers_used & 2


def test_cal_is_the_rigid_correction_of_the_priors_affine_map(ssd):
    cfg, truth, stair_map, frame = _straight(ssd)
    prior = spm.moved(ssd, truth, (1.0 * spm.DEG, 0.3 * spm.DEG, 2.0 * spm.DEG), (0.0, 0.01, 0.01), (0.0, 0.65, 0.16))
    _, poses = spm.chain_host(ssd, cfg, [frame], prior, stair_map, passes=1, min_points=100)
    p = poses[0]
    assert p.status == ssd.GF_OK and np.linalg.norm(list(p.rotation)) > 0.02
    pts = np.random.default_rng(5).uniform(-8.0, 8.0, (1000, 3))
    centre, tau = np.array(list(p.centre)), np.array(list(p.translation))
    want = (_apply(prior, pts) - centre) @ spm.rot(list(p.rotation)).T + centre + tau
    got = _apply(p.cal, pts)
    assert np.abs(want).max() < 16.0
    assert np.abs(got - want).max() <= 1e-9, "algebra: only rounding"
    assert p.cal.world_z == prior.world_z and list(p.cal.b[:2]) == [0.0, 0.0]


# ---- the recorded recipe ------------------------------------------------------------------------------------------------------------------
def test_the_recorded_recipe(ssd, oracle):
    """tools/stair_pose_accuracy.py's figures, computed again: each one as recorded (to the three digits the file holds), the default
    taken from them, and the condition - every offset prior ends nearer to (a)'s pose than it began, in each observed component"""
    rec = spm.recorded_accuracy()
    r = spm.recipe(ssd, oracle)
    same = lambda got, want: abs(abs(got) - want) <= 1e-3 * want + 1e-12
    for name, v in zip(("pitch_rad", "roll_rad", "yaw_rad", "going_m", "height_m"), r["bias"]):
        assert same(v, rec["bias_" + name]), name
    assert r["unobserved_max"] == rec["unobserved_max"] == 0.0 and same(r["observed_min"], rec["observed_min"])
    assert rec["observable"] == ssd.SP_OBSERVABLE
    assert float("%.1e" % math.sqrt(max(rec["unobserved_max"], spm.ROUNDING) * rec["observed_min"])) == rec["observable"], "the geometric mean"
    assert all(s[0] <= spm.ROUNDING < ssd.SP_OBSERVABLE < s[1] for c in r["cases"].values() for s in c["spectra"])
    worst = [0.0] * 5
    for name, c in r["cases"].items():
        assert c["status"] == [ssd.GF_OK] * spm.PASSES and c["dof"] == [5] * spm.PASSES, name
        for k, (b, e) in enumerate(zip(c["begin"], c["after"][-1])):
            assert abs(e) < abs(b), "%s: %s ends at %.3e, began at %.3e" % (name, spm.COMPONENTS[k], e, b)
        worst = [max(a, abs(b)) for a, b in zip(worst, c["after"][-1])]
    for name, v in zip(("pitch_rad", "roll_rad", "yaw_rad", "going_m", "height_m"), worst):
        assert same(v, rec["worst_end_" + name]), name
