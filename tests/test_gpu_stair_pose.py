"""The stair pose on the GPU (ssd_enqueue_stair_pose / ssd_fetch_stair_pose_moments / ssd_fetch_stair_pose / ssd_process_host_stair_pose;
include/ssd_hip.h).  Every comparison is bytes: a frame's record against ssd_stair_pose_host (which
tests/test_stair_pose.py holds to the numpy restatement), a target's pose against the host solve of the host fold.  Small shapes - the
kernel's paths depend on the input, the alignment and the tails, not on the size: the five 256 x 192 scene frames, the 640 x 480
17-surface frames, and the smallest frame whose point count divides neither load unit."""
import ctypes as C

import numpy as np
import pytest

import full_width as fw
import stair_pose_model as spm
from test_gpu_follow_passes import two_streams  # noqa: F401  (a fixture)
from test_stair_pose import WIDE_RULE, scene_sets, wide  # noqa: F401  (fixtures)

NONE = 0xffff


class Frames:
    """frames resident on the device behind one detector, at a stride that is a multiple of 16 bytes (the wide loads) or not (the
    narrow ones: every frame but the first starts off the boundary)"""

    def __init__(self, ssd, device, cfg, cal, frames, depth=False, intr=None, aligned=True, batch=None):
        self.ssd, self.depth, self.n = ssd, depth, len(frames)
        cfg = type(cfg).from_buffer_copy(cfg)
        cfg.max_frames_per_batch = batch or max(self.n, 2)
        self.cfg = cfg
        self.det = ssd.Detector(cfg, cal, device)
        if depth and intr is not None:
            self.det.set_intrinsics(intr)
        fb = np.ascontiguousarray(frames[0]).nbytes
        self.stride = (fb + 15) // 16 * 16 + (16 if aligned else (2 if depth else 4))
        assert (self.stride % 16 == 0) == aligned
        # the first frame of the narrow case starts off the boundary too
        self.lead = 0 if aligned else (2 if depth else 4)
        self.src = ssd.DeviceBuffer(self.lead + self.stride * self.n, device)
        for i, f in enumerate(frames):
            self.src.upload(np.ascontiguousarray(f), offset=self.lead + i * self.stride)
        self.ptr = self.src.ptr + self.lead

    def pose(self, targets, index=None, rule=None, stream=None, n=None):
        self.det.enqueue_stair_pose(self.ptr, n or self.n, targets, index, rule, depth=self.depth, stride_bytes=self.stride, stream=stream)

    def close(self):
        self.src.free()
        self.det.close()


def _want(ssd, cfg, targets, index, frames, rule, depth):
    """the host's word: per frame the record of ssd_stair_pose_host under the frame's target (all zero for NONE), per target the fold"""
    zero = bytes(C.sizeof(ssd.StairPoseMoments))
    recs = [zero if t == NONE else bytes(ssd.stair_pose_host(cfg, targets[t], f, rule, depth=depth)) for f, t in zip(frames, index)]
    folds = [ssd.StairPoseMoments() for _ in targets]
    for r, t in zip(recs, index):
        if t != NONE:
            ssd.stair_pose_add(ssd.StairPoseMoments.from_buffer_copy(r), folds[t])
    return recs, folds


def _check(ssd, r, targets, index, frames, rule=None, min_points=200):
    rule = rule or ssd.StairPoseRule()
    r.pose(targets, index, rule)
    index = index or [0] * r.n
    got = [bytes(m) for m in r.det.fetch_stair_pose_moments(r.n)]
    recs, folds = _want(ssd, r.cfg, targets, index, frames, rule, r.depth)
    assert [g == w for g, w in zip(got, recs)] == [True] * r.n
    poses = r.det.fetch_stair_pose(min_points)
    assert len(poses) == len(targets)
    for t, (p, fold) in enumerate(zip(poses, folds)):
        assert bytes(p) == bytes(ssd.stair_pose_solve(fold, targets[t], min_points)), "target %d: the host solve of the host fold" % t
    return [ssd.StairPoseMoments.from_buffer_copy(g) for g in got], poses


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [False, True], ids=["stride-odd", "stride-16B-multiple"])
@pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])
def test_the_scene_frames_equal_the_host(ssd, gpu_device, scene_sets, depth, aligned):
    d = scene_sets[depth]
    intr = d["intr"] if depth else None
    true, off = (spm.target(ssd, cal, d["map"], intr) for cal in d["priors"])
    r = Frames(ssd, gpu_device, d["cfg"], d["priors"][0], d["frames"], depth, intr, aligned)
    try:
        recs, poses = _check(ssd, r, [true], None, d["frames"])
        assert all(m.treads.n_surfaces == 3 and m.risers.n_surfaces == 2 and m.risers.s[1].m.n > 500 for m in recs)
        assert (poses[0].status, poses[0].dof) == (ssd.GF_OK, 5)
        # three targets: one frame names none, and nobody names target 2
        recs, poses = _check(ssd, r, [true, off, true], [0, NONE, 1, 0, 1], d["frames"])
        assert bytes(recs[1]) == bytes(C.sizeof(ssd.StairPoseMoments)) and bytes(recs[0]) != bytes(recs[2])
        assert [p.status for p in poses] == [ssd.GF_OK, ssd.GF_OK, ssd.GF_FEW]
        # a thrown map and an empty one beside a live one
        thrown, empty = (ssd.StairPoseTarget.from_buffer_copy(true) for _ in range(2))
        thrown.map.stairs.status |= ssd.ST_THROW
        empty.map.stairs.n_steps = 0
        recs, poses = _check(ssd, r, [thrown, empty, off], [0, 1, 2, 0, 1], d["frames"])
        assert [bytes(m) == bytes(C.sizeof(ssd.StairPoseMoments)) for m in recs] == [True, True, False, True, True]
        assert [p.status for p in poses] == [ssd.GF_FEW, ssd.GF_FEW, ssd.GF_OK]
    finally:
        r.close()


@pytest.mark.gpu
def test_the_full_width_frames_equal_the_host(ssd, oracle, gpu_device, wide):
    ref, stair_map = wide
    frames = [fw.reference(ssd, oracle, layout).xyz for layout in ("scatter", "ordered", "lanes")]
    t = spm.target(ssd, ref.cal, stair_map)
    for aligned in (True, False):
        r = Frames(ssd, gpu_device, ref.cfg, ref.cal, frames, aligned=aligned)
        try:
            recs, poses = _check(ssd, r, [t], None, frames, spm.rule_of(ssd, WIDE_RULE), min_points=100)
            assert all(m.treads.s[k].m.n > 0 for m in recs for k in range(17)) and all(m.risers.s[i].m.n > 0 for m in recs for i in range(16))
            assert len({bytes(m) for m in recs}) == 1, "the layouts place the same points"
            # every class takes part; the frames' camera looks along the world's z axis from below it, which no floor plane stands
            # for (ssd_calibration_from_plane refuses it): the step is found, the calibration cannot be formed
            assert (poses[0].status, poses[0].treads_used, poses[0].risers_used) == (ssd.GF_DEGENERATE, 0x1ffff, 0xffff)
        finally:
            r.close()


def _small_case(ssd, w, h):
    """a frame of w x h depth values that reach every tread and riser of a 3-step map, far places among them, and nothing at all, and
    the vertices they deproject to: the camera at the world's origin looking along z with a focal length of 1000 pixels, so ez = z and
    (ex, ey) stay within millimetres of the axis.  Step 0 at 0.5 m spans 400 m around it; steps 1 (2 m) and 2 (20 m: every point there is
    a far one) lie behind the edge y = 0, whose plane carries both risers; band and clear 0.5, reach 1."""
    import clearance_model as cm
    cfg = ssd.default_config(w, h)
    cfg.x_min, cfg.x_max, cfg.y_min, cfg.y_max = -500.0, 500.0, -500.0, 500.0
    cal = ssd.GeometricTransformation().constants
    intr = ssd.Intrinsics(1000.0, 1000.0, (w - 1) / 2.0, (h - 1) / 2.0, 0.001)
    behind = [-200.0, 0.0, 200.0, 0.0, -200.0, 200.0, 200.0, 200.0]
    around = [-200.0, -200.0, 200.0, -200.0, -200.0, 200.0, 200.0, 200.0]
    stair_map = ssd.StairMap()
    C.memmove(C.byref(stair_map.stairs), C.byref(cm.hand_result(ssd, [(0.5, around), (2.0, behind), (20.0, behind)])), C.sizeof(ssd.FrameResult))
    stair_map.ground = 1
    values = np.array([0, 300, 500, 900, 1200, 1400, 1800, 2200, 3000, 17000, 20000, 30000, 65535], dtype=np.uint16)
    depth = values[np.random.default_rng(w * 100 + h).integers(0, len(values), (h, w))]
    depth[h - 1, w - 1], depth[h - 1, w - 2], depth[0, 0], depth[1, 0] = 1300, 2200, 17000, 20000   # the tails: a riser point last, a tread point in front of it
    return cfg, cal, intr, stair_map, (0.0, 0.5, 0.5, 1.0), depth


@pytest.mark.gpu
def test_a_frame_whose_point_count_divides_neither_unit(ssd, gpu_device):
    """the smallest shape ssd_create accepts whose point count is a multiple of neither 4 nor 8: the wide loops' tails are taken, and a
    depth unit of 8 crosses a row end"""
    shape = None
    for w, h in ((3, 3), (5, 3), (3, 5), (5, 5), (7, 5), (9, 7), (13, 11), (31, 23)):
        assert (w * h) % 4 != 0 and w * h > 8 and w < 8
        cfg = ssd.default_config(w, h, max_frames_per_batch=2)
        try:
            ssd.Detector(cfg, ssd.GeometricTransformation().constants, gpu_device).close()
        except ssd.SsdError:
            continue
        shape = (w, h)
        break
    assert shape is not None, "ssd_create accepts no shape whose point count is a multiple of neither 4 nor 8 among the candidates"
    w, h = shape
    cfg, cal, intr, stair_map, rule, depth = _small_case(ssd, w, h)
    xyz = ssd.deproject_host(intr, depth)
    model = spm.record_np(cfg, cal, stair_map, xyz, rule)
    assert model[1][0][0] > 0 and model[1][1][0] > 0 and model[2][0][0] > 0, "treads and a riser hold near points"
    assert model[1][2][10] > 0 and model[2][1][10] > 0, "and a tread and a riser far ones"
    for dep, frame in ((False, xyz), (True, depth)):
        t = spm.target(ssd, cal, stair_map, intr if dep else None)
        assert spm.record_tuple(ssd.stair_pose_host(cfg, t, frame, spm.rule_of(ssd, rule), depth=dep)) == model
        for aligned in (True, False):
            r = Frames(ssd, gpu_device, cfg, cal, [frame, frame[::-1].copy()], dep, intr, aligned)
            try:
                _check(ssd, r, [t], None, [frame, frame[::-1].copy()], spm.rule_of(ssd, rule), min_points=1)
            finally:
                r.close()


@pytest.mark.gpu
def test_the_host_path_over_33_frames_equals_the_resident_pass(ssd, gpu_device, scene_sets):
    d = scene_sets[False]
    frames = [d["frames"][i % 5] for i in range(33)]
    true, off = (spm.target(ssd, cal, d["map"]) for cal in d["priors"])
    index = [(i * 7) % 3 for i in range(33)]
    index[5] = index[32] = NONE
    index = [NONE if t == 2 else t for t in index]
    r = Frames(ssd, gpu_device, d["cfg"], d["priors"][0], frames, batch=33)
    try:
        r.pose([true, off], index)
        resident = [bytes(m) for m in r.det.fetch_stair_pose_moments(33)]
        resident_poses = [bytes(p) for p in r.det.fetch_stair_pose()]
        poses, recs = r.det.process_host_stair_pose(np.stack(frames), [true, off], index, moments=True)
        assert [bytes(m) for m in recs] == resident, "two slices, one resident call"
        assert [bytes(p) for p in poses] == resident_poses
        assert bytes(r.det.process_host_stair_pose(np.stack(frames), [true, off], index)[1]) == resident_poses[1], "without the records"
        _, folds = _want(ssd, r.cfg, [true, off], index, frames, ssd.StairPoseRule(), False)
        assert [bytes(p) for p in poses] == [bytes(ssd.stair_pose_solve(f, t)) for f, t in zip(folds, (true, off))]
        # the chain of passes a caller would run: from the offset prior towards the true one
        last, chain = r.det.locate_camera(np.stack(frames[:5]), d["priors"][1], d["map"])
        cals, host_chain = spm.chain_host(ssd, r.cfg, frames[:5], d["priors"][1], d["map"])
        assert [bytes(p) for p in chain] == [bytes(p) for p in host_chain] and bytes(last.cal) == bytes(cals[-1])
    finally:
        r.close()


@pytest.mark.gpu
def test_two_calls_on_two_streams_with_no_host_wait(ssd, gpu_device, scene_sets, two_streams):  # noqa: F811
    d = scene_sets[False]
    a, b = two_streams
    true, off = (spm.target(ssd, cal, d["map"]) for cal in d["priors"])
    r = Frames(ssd, gpu_device, d["cfg"], d["priors"][0], d["frames"])
    try:
        tight = ssd.StairPoseRule(0.05, 0.02, 0.05, 0.02)
        r.pose([true], None, None, stream=a)
        r.pose([off, true], [1, 0, 1, 0, NONE], tight, stream=b)           # no host wait between them
        got = [bytes(m) for m in r.det.fetch_stair_pose_moments(5)]
        want, _ = _want(ssd, r.cfg, [off, true], [1, 0, 1, 0, NONE], d["frames"], tight, False)
        first, _ = _want(ssd, r.cfg, [true], [0] * 5, d["frames"], ssd.StairPoseRule(), False)
        assert got == want and got != first, "the records are the last call's"
        assert len(r.det.fetch_stair_pose()) == 2
    finally:
        r.close()


@pytest.mark.gpu
def test_refusals_workspace_detection_and_time(ssd, gpu_device, scene_sets):
    L = ssd.lib()
    d = scene_sets[False]
    t = spm.target(ssd, d["priors"][0], d["map"])
    r = Frames(ssd, gpu_device, d["cfg"], d["priors"][0], d["frames"])
    try:
        det = r.det
        det.enqueue(r.ptr, 5, stride_bytes=r.stride)
        before_results = [bytes(x) for x in det.fetch_list(5)]
        before = det.workspace_bytes
        rule, targets = ssd.StairPoseRule(), (ssd.StairPoseTarget * 2)(t, t)
        idx = (C.c_uint16 * 5)(0, 1, 0, 1, NONE)

        def call(h=det._h, ptr=r.ptr, stride=r.stride, n=5, inp=0, tg=targets, nt=2, index=idx, rl=rule):
            return L.ssd_enqueue_stair_pose(h, C.c_void_p(ptr), stride, n, None, inp, tg, nt, index, C.byref(rl) if rl is not None else None)
        bad_index, bad_map = (C.c_uint16 * 5)(0, 1, 2, 0, 0), (ssd.StairPoseTarget * 2)(t, t)
        bad_map[1].map.stairs.n_steps = ssd.MAX_STEPS + 1
        refused = [call(h=None), call(ptr=0), call(n=0), call(n=6), call(inp=2), call(ptr=r.ptr + 2), call(stride=r.stride - 32), call(rl=None),
                   call(rl=ssd.StairPoseRule(0.03, 0.0, 0.03, 0.04)), call(rl=ssd.StairPoseRule(0.03, 0.03, 0.03, float("nan"))), call(tg=None),
                   call(nt=0), call(nt=ssd.MAX_STAIR_MAPS + 1), call(tg=bad_map), call(index=bad_index), call(inp=1)]
        assert refused == [-1] * len(refused)
        assert det.workspace_bytes == before, "a refused call allocates nothing"
        with pytest.raises(ssd.SsdError):
            det.fetch_stair_pose_moments(5)                           # ... and launched nothing: there is no pass to wait for
        assert L.ssd_fetch_stair_pose(det._h, (ssd.StairPose * 2)(), 1, 0.0, None) == -1
        assert L.ssd_get_stair_pose_time(det._h, C.byref(C.c_float())) == -1
        assert call() == 0
        after = det.workspace_bytes
        assert after - before >= 2 * 5 * C.sizeof(ssd.StairPoseMoments), "the records, on the device and pinned, are counted"
        got = [bytes(m) for m in det.fetch_stair_pose_moments(5)]
        assert got == _want(ssd, r.cfg, [t, t], [0, 1, 0, 1, NONE], d["frames"], rule, False)[0]
        assert det.stair_pose_time_ms() == 0.0, "timing was off for it"
        det.set_timing(True)
        assert call() == 0 and det.workspace_bytes == after, "made once"
        assert [bytes(m) for m in det.fetch_stair_pose_moments(3)] == got[:3]
        assert 0.0 < det.stair_pose_time_ms() < 1000.0
        with pytest.raises(ssd.SsdError):
            det.fetch_stair_pose_moments(6)
        assert [bytes(x) for x in det.fetch_list(5)] == before_results, "the detection's results are untouched"
    finally:
        r.close()
