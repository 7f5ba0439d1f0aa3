"""What the four stand-alone frame passes - the ground fit, the stair pose, the depth fusion, the depth edge filter - share on the host
side: one record type with one fetch, one uploaded-table type, one host-fed depth pre-pass over one staging buffer.
Each pass's own file (test_gpu_ground_fit.py, test_gpu_stair_pose.py, test_gpu_depth_fuse.py, test_gpu_depth_edges.py) holds its kernel to
its host statement; here the passes stand side by side on the small still stairs scene (256 x 192 depth frames), every comparison is bytes
against the host functions or against a fresh handle, and the refusals are the library's strings, written out."""
import ctypes as C

import numpy as np
import pytest

import fuse_model as fm
import stair_pose_model as spm
from test_gpu_ground_fit import TOL, _moments, _prior_arg, _set, _upload
from test_gpu_ground_fit import _want as ground_want
from test_gpu_stair_pose import Frames
from test_gpu_stair_pose import _want as pose_want
from test_stair_pose import scene_sets  # noqa: F401  (a fixture)

W, H, F = 256, 192, 4
POSE_TARGET_BYTES = 4344                                              # sizeof(ssd::PoseTarget), csrc/ssd_pose.h: the targets as the kernel reads them


@pytest.fixture(scope="module")
def stairs(ssd):
    """18 depth frames of the still 256 x 192 scene and what detects them"""
    sc = ssd.make_scene(W, H, n_steps=3, seed=1000, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02)
    return dict(cal=ssd.transformation_for_scene(sc).constants, intr=ssd.intrinsics_for_scene(sc), frames=fm.scene_frames(ssd, W, H, 18))


def _detector(ssd, device, d):
    det = ssd.Detector(ssd.default_config(W, H, max_frames_per_batch=F), d["cal"], device)
    det.set_intrinsics(d["intr"])
    return det


def _bytes(records):
    return [bytes(r) for r in records]


# ---- the shared staging buffer of the host-fed depth pre-passes

def _host_calls(ssd, frames):
    """the calls of the staging test, in its order: (what, call(det) -> everything the call returns, as bytes)"""
    def fused(n, count):
        def call(det):
            res, out, stats = det.process_depth_host_fused(frames[:count], n, fused=True, stats=True)
            return _bytes(res), out.tobytes(), _bytes(stats)
        return call

    def edges(count):
        def call(det):
            res, out, stats = det.process_depth_host_edges(frames[:count], filtered=True, stats=True)
            return _bytes(res), out.tobytes(), _bytes(stats)
        return call
    return [("edges over 3 frames: one partial slice", edges(3)),
            ("fused, n = 2, over 18 frames: five slices", fused(2, 18)),
            ("edges over 9 frames: a partial last slice", edges(9)),
            ("fused, n = 3, over 9 frames: slices cut down to one group", fused(3, 9)),
            ("plain detection", lambda det: _bytes(det.process_depth_host(frames[:5])))]


@pytest.mark.gpu
def test_one_staging_buffer_serves_both_host_fed_pre_passes(ssd, gpu_device, stairs):
    """a slice is 4 frames: the filter stages 4 frames, the fusion 2 (n = 2) or 1 (n = 3, the slice cut down to 3 frames), so the later
    calls run in the buffer an earlier call of the OTHER pass made; each call equals the same call on a fresh handle"""
    calls = _host_calls(ssd, stairs["frames"])
    one = _detector(ssd, gpu_device, stairs)
    try:
        for what, call in calls:
            got = call(one)
            fresh = _detector(ssd, gpu_device, stairs)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert got == want, what
        res = [ssd.FrameResult.from_buffer_copy(x) for x in got]
        assert any(r.n_steps >= 3 for r in res), "the frames show the staircase"
    finally:
        one.close()


@pytest.mark.gpu
def test_the_staging_buffer_grows_between_the_pre_passes(ssd, gpu_device, stairs):
    """the fusion first (n = 2: 2 staged frames per slice), then the filter (4): the buffer the fusion made is too small for the filter"""
    frames = stairs["frames"]
    one, fresh = _detector(ssd, gpu_device, stairs), _detector(ssd, gpu_device, stairs)
    try:
        one.process_depth_host_fused(frames[:8], 2)
        got = one.process_depth_host_edges(frames[:9], filtered=True, stats=True)
        want = fresh.process_depth_host_edges(frames[:9], filtered=True, stats=True)
        assert _bytes(got[0]) == _bytes(want[0]) and (got[1] == want[1]).all() and _bytes(got[2]) == _bytes(want[2])
        assert (got[1] == np.array([ssd.depth_edges_host(f)[0] for f in frames[:9]])).all(), "and the host's"
    finally:
        one.close()
        fresh.close()


# ---- the four passes' records: fetch rules and workspace accounting

class Resident:
    """the first F depth frames of the scene on the device behind one detector, an output buffer beside them, and the stair pose's target"""

    def __init__(self, ssd, device, d):
        self.ssd, self.d = ssd, d
        self.det = _detector(ssd, device, d)
        self.frames = d["frames"][:F]
        self.src, self.out = _upload(ssd, self.frames, device), ssd.DeviceBuffer(F * W * H * 2, device)
        stair_map, used = ssd.stair_map_from_results(self.det.process_depth_host(self.frames))
        assert used >= 1 and stair_map.stairs.n_steps >= 3
        self.target = ssd.stair_pose_target(d["cal"], stair_map, d["intr"])

    def close(self):
        self.src.free()
        self.out.free()
        self.det.close()


class Pass:
    """enqueue(r, n): n records' worth of the pass over the resident frames; fetch(r, n) -> n records as bytes; host(r, i): record i, the
    host's; refusal: ssd_fetch_*'s, the string in csrc/ssd_capi.hip; added(F): the bytes the first call adds to the workspace"""

    def __init__(self, enqueue, fetch, host, refusal, added, bad):
        self.enqueue, self.fetch, self.host, self.refusal, self.added, self.bad = enqueue, fetch, host, refusal, added, bad


def _sizeof(ssd, name):
    return C.sizeof(getattr(ssd, name))


PASSES = {
    # the ground fit: the records and the priors on the device; its pinned sides are not counted
    "ground_fit": Pass(
        lambda r, n: r.det.enqueue_ground_fit(r.src.ptr, n, TOL, depth=True),
        lambda r, n: [bytes(f.m) for f in r.det.fetch_ground_fit(n, min_points=1)],
        lambda r, i: bytes(r.ssd.ground_moments_host(r.det.cfg, (r.d["cal"], r.d["intr"]), r.frames[i], TOL, depth=True)),
        "ssd_fetch_ground_fit: nframes must be 1..the frames of the last ssd_enqueue_ground_fit",
        lambda ssd: F * (_sizeof(ssd, "GroundMoments") + 128),
        lambda r: r.det.enqueue_ground_fit(r.src.ptr, F + 1, TOL, depth=True)),
    # the stair pose: the records, the targets and the index, each on the device and pinned
    "stair_pose": Pass(
        lambda r, n: r.det.enqueue_stair_pose(r.src.ptr, n, [r.target], depth=True),
        lambda r, n: _bytes(r.det.fetch_stair_pose_moments(n)),
        lambda r, i: bytes(r.ssd.stair_pose_host(r.det.cfg, r.target, r.frames[i], depth=True)),
        "ssd_fetch_stair_pose_moments: nframes must be 1..the frames of the last ssd_enqueue_stair_pose",
        lambda ssd: 2 * (F * _sizeof(ssd, "StairPoseMoments") + ssd.MAX_STAIR_MAPS * POSE_TARGET_BYTES + F * 4),
        lambda r: r.det.enqueue_stair_pose(r.src.ptr, F + 1, [r.target], depth=True)),
    # the fusion in groups of one frame, so that n counts groups as it counts frames elsewhere
    "depth_fuse": Pass(
        lambda r, n: r.det.enqueue_depth_fuse(r.src.ptr, n, 1, r.out.ptr),
        lambda r, n: _bytes(r.det.fetch_depth_fuse(n)),
        lambda r, i: bytes(r.ssd.depth_fuse_host(r.frames[i:i + 1])[1]),
        "ssd_fetch_depth_fuse: ngroups must be 1..the groups of the last ssd_enqueue_depth_fuse",
        lambda ssd: 2 * F * _sizeof(ssd, "FuseStats"),
        lambda r: r.det.enqueue_depth_fuse(r.src.ptr, F, 1, r.src.ptr)),
    "depth_edges": Pass(
        lambda r, n: r.det.enqueue_depth_edges(r.src.ptr, n, r.out.ptr),
        lambda r, n: _bytes(r.det.fetch_depth_edges(n)),
        lambda r, i: bytes(r.ssd.depth_edges_host(r.frames[i])[1]),
        "ssd_fetch_depth_edges: nframes must be 1..the frames of the last ssd_enqueue_depth_edges",
        lambda ssd: 2 * F * _sizeof(ssd, "EdgeStats"),
        lambda r: r.det.enqueue_depth_edges(r.src.ptr, F, r.src.ptr)),
}


@pytest.fixture(scope="module")
def host_records(ssd, gpu_device, stairs):
    """per pass the host's records of the F resident frames, computed once"""
    r = Resident(ssd, gpu_device, stairs)
    try:
        return {name: [p.host(r, i) for i in range(F)] for name, p in PASSES.items()}
    finally:
        r.close()


def _refused(ssd, p, r, n):
    with pytest.raises(ssd.SsdError) as e:
        p.fetch(r, n)
    assert str(e.value) == "libssd_hip error -1: " + p.refusal, "SSD_E_ARG and the library's words"


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PASSES))
def test_the_fetch_rules(ssd, gpu_device, stairs, host_records, name):
    p, want = PASSES[name], host_records[name]
    assert len(set(want)) == F, "the frames' records differ, so a fetch of the wrong ones shows"
    r = Resident(ssd, gpu_device, stairs)
    try:
        _refused(ssd, p, r, 1)                                        # before any enqueue
        p.enqueue(r, 3)
        _refused(ssd, p, r, 0)
        _refused(ssd, p, r, 4)                                        # one more than the last enqueue's, though the handle holds 4
        assert p.fetch(r, 3) == want[:3], "after the refusals"
        assert p.fetch(r, 2) == want[:2] and p.fetch(r, 1) == want[:1], "fewer than were enqueued: the first n"
        p.enqueue(r, 4)
        assert p.fetch(r, 4) == want
        p.enqueue(r, 1)
        _refused(ssd, p, r, 2)                                        # the count is the LAST call's
        assert p.fetch(r, 1) == want[:1]
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PASSES))
def test_the_workspace_accounting(ssd, gpu_device, stairs, host_records, name):
    p = PASSES[name]
    r, plain = Resident(ssd, gpu_device, stairs), _detector(ssd, gpu_device, stairs)
    try:
        plain.process_depth_host(r.frames)                            # what Resident ran for the target's map
        before = r.det.workspace_bytes
        assert before == plain.workspace_bytes, "a handle that never ran the pass holds nothing for it"
        with pytest.raises(ssd.SsdError):
            p.bad(r)
        assert r.det.workspace_bytes == before, "a refused call allocates nothing"
        p.enqueue(r, 2)
        assert r.det.workspace_bytes - before == p.added(ssd), "the first call: exactly its buffers"
        p.enqueue(r, F)
        assert r.det.workspace_bytes - before == p.added(ssd), "the second call adds nothing"
        assert p.fetch(r, F) == host_records[name]
        for other, q in PASSES.items():                               # every other pass adds its own and only its own
            if other != name:
                at = r.det.workspace_bytes
                q.enqueue(r, 1)
                assert r.det.workspace_bytes - at == q.added(ssd), other
    finally:
        plain.close()
        r.close()


# ---- the uploaded tables: the pinned side is rewritten only behind the previous call's copy

@pytest.mark.gpu
def test_two_ground_fits_back_to_back_with_different_priors(ssd, gpu_device):
    d = _set(ssd, 64, 50)
    det = ssd.Detector(d["cfg"], d["priors"][0], gpu_device)
    buf = _upload(ssd, d["xyz"], gpu_device)
    try:
        first, second = [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]
        det.enqueue_ground_fit(buf.ptr, 5, TOL, priors=_prior_arg(d, first, False))
        det.enqueue_ground_fit(buf.ptr, 5, TOL, priors=_prior_arg(d, second, False))      # the same stream, no host wait between them
        got = _moments(det.fetch_ground_fit(5, min_points=1))
        assert got == [ground_want(ssd, d, i, second[i], False) for i in range(5)], "the second call's priors"
        assert got != [ground_want(ssd, d, i, first[i], False) for i in range(5)]
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
def test_two_stair_poses_back_to_back_with_different_targets(ssd, gpu_device, scene_sets):  # noqa: F811
    d = scene_sets[False]
    true, off = (spm.target(ssd, cal, d["map"]) for cal in d["priors"])
    r = Frames(ssd, gpu_device, d["cfg"], d["priors"][0], d["frames"])
    try:
        r.pose([true, off], [0, 1, 0, 1, 0])
        r.pose([off, true], [0, 1, 1, 0, 0])                           # the same stream, no host wait between them
        got = _bytes(r.det.fetch_stair_pose_moments(5))
        want, folds = pose_want(ssd, r.cfg, [off, true], [0, 1, 1, 0, 0], d["frames"], ssd.StairPoseRule(), False)
        assert got == want, "the second call's targets and index"
        assert got != pose_want(ssd, r.cfg, [true, off], [0, 1, 0, 1, 0], d["frames"], ssd.StairPoseRule(), False)[0]
        poses = r.det.fetch_stair_pose()
        assert [bytes(p) for p in poses] == [bytes(ssd.stair_pose_solve(f, t)) for f, t in zip(folds, [off, true])]
    finally:
        r.close()
