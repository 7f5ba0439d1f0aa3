"""The depth warp on the GPU (ssd_enqueue_depth_warp / ssd_fetch_depth_warp / ssd_get_depth_warp_time / ssd_process_depth_host_warp_fused;
include/ssd_hip.h).  Every comparison is bytes against ssd_depth_warp_host, which tests/test_depth_warp.py holds to
the numpy restatement of the rule, and every byte of the output buffer outside the frames is checked untouched behind a fill pattern.

The shapes are those at which k_depth_warp (csrc/ssd_k_warp.h) takes another path: a lane's unit is 8 pixels (widths 8, 9 x 2), a wave's
64 units are 512 (511 x 2, 512, 513 x 2), a block's step 2048 (512 x 4, 513 x 4: exactly one step, and a second with a tail), the smallest
frames with an even pixel count, each with the
input at 16-byte alignment (the wide body) and at 2-byte alignment (the narrow one) and output strides wider than a frame; 64 x 48 and
256 x 192 where a scene is needed.  The scatter's own cases are the contention frames: every sample on one pixel, and on the two pixels of
one 32-bit word."""
import ctypes as C

import numpy as np
import pytest

import fuse_model as fm
import warp_model as wm
from test_gpu_follow_passes import two_streams  # noqa: F401  (a fixture)

FILL = 0xAB
SHAPES = [(8, 1), (9, 2), (511, 2), (512, 1), (513, 2), (512, 4), (513, 4), (2, 1), (1, 2)]


def _intr(ssd, fx, fy, ppx, ppy, units=0.00025):
    i = ssd.Intrinsics()
    i.fx, i.fy, i.ppx, i.ppy, i.depth_units = fx, fy, ppx, ppy, units
    return i


class Warper:
    """a batch of depth frames resident on the device behind one detector and the output buffer.  aligned: the input at pointers and
    strides that are multiples of 16 bytes (the wide body), else of 2 only (the narrow one); the output at multiples of 16, else of 4
    only.  The strides are wider than a frame either way"""

    def __init__(self, ssd, device, frames, aligned=True, batch=None, cfg=None, cal=None):
        self.ssd, self.total = ssd, len(frames)
        h, w = frames[0].shape
        if cfg is None:
            cfg = ssd.default_config(w, h, max_frames_per_batch=batch or max(self.total, 2))
        self.cfg, self.points, self.shape = cfg, w * h, (h, w)
        self.det = ssd.Detector(cfg, cal if cal is not None else ssd.GeometricTransformation().constants, device)
        fb = self.points * 2
        self.lead = 0 if aligned else 2
        self.out_lead = 0 if aligned else 4
        self.stride = (fb + 15) // 16 * 16 + (32 if aligned else 6)
        self.out_stride = (fb + 15) // 16 * 16 + (32 if aligned else 12)
        assert (self.stride % 16 == 0) == aligned and self.out_stride % 4 == 0
        self.src = ssd.DeviceBuffer(self.lead + self.stride * self.total, device)
        self.out = ssd.DeviceBuffer(self.out_lead + self.out_stride * self.total + 8, device)
        self.load(frames)

    def load(self, frames):
        self.frames = frames
        for i, f in enumerate(frames):
            self.src.upload(np.ascontiguousarray(f), offset=self.lead + i * self.stride)

    def frames_of(self, raw, nframes):
        return np.array([raw[self.out_lead + g * self.out_stride:self.out_lead + g * self.out_stride + 2 * self.points].view(np.uint16).reshape(self.shape)
                         for g in range(nframes)])

    def run(self, nframes, views, dst, stream=None):
        """-> (warped frames [n, H, W], stats); everything outside the frames' pixels is untouched"""
        self.out.upload(np.full(self.out.nbytes, FILL, np.uint8))
        self.det.enqueue_depth_warp(self.src.ptr + self.lead, nframes, views, dst, self.out.ptr + self.out_lead, self.stride, self.out_stride, stream)
        stats = self.det.fetch_depth_warp(nframes)
        raw = self.out.download(self.out.nbytes)
        touched = np.zeros(self.out.nbytes, bool)
        for g in range(nframes):
            at = self.out_lead + g * self.out_stride
            touched[at:at + 2 * self.points] = True
        assert (raw[~touched] == FILL).all(), "a byte outside the warped frames was written"
        return self.frames_of(raw, nframes).copy(), stats

    def close(self):
        for b in (self.src, self.out):
            b.free()
        self.det.close()


def _want(ssd, frames, views, dst):
    got = [ssd.depth_warp_host(f, v, dst) for f, v in zip(frames, views)]
    return np.array([o for o, _ in got]), [bytes(st) for _, st in got]


def _check(ssd, r, views, dst, what=""):
    n = len(views)
    outs, stats = r.run(n, views, dst)
    want_o, want_st = _want(ssd, r.frames[:n], views, dst)
    bad = np.argwhere(outs != want_o)
    assert len(bad) == 0, "%s: the warped frames differ at (frame, row, column) %s ... got %s want %s" % (
        what, bad[:5].tolist(), [int(outs[tuple(b)]) for b in bad[:5]], [int(want_o[tuple(b)]) for b in bad[:5]])
    assert [bytes(s) for s in stats] == want_st, "%s: the frames' records %s" % (what, [wm.stats_dict(s) for s in stats])
    assert all(s.n_empty + s.n_behind + s.n_range + s.n_outside + s.n_landed == r.points for s in stats)
    return outs, stats


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
def test_the_scenes_under_the_eight_views_equal_the_host(ssd, gpu_device, aligned):
    frames, src = wm.scene_frames(ssd), wm.scene_src(ssd, 64, 48)
    views = wm.seeded_views(ssd, src)
    r = Warper(ssd, gpu_device, [f for f in frames for _ in views], aligned)
    try:
        _check(ssd, r, views * 3, src, "the scenes under the eight views")
        _check(ssd, r, views[:5], _intr(ssd, 50.0, 47.0, 30.25, 25.5, 0.0005), "another target")
    finally:
        r.close()


def _shape_frames(w, h, seed):
    """seeded frames of a surface one to three metres away with holes, the ends of the range and a few near samples"""
    rng = np.random.default_rng(seed + 131 * w + h)
    f = rng.integers(4000, 12000, size=(3, h, w))
    f = np.where(rng.random((3, h, w)) < 0.1, 0, f)
    f = np.where(rng.random((3, h, w)) < 0.05, rng.choice(np.array([1, 2, 65535, 300]), size=(3, h, w)), f)
    return list(f.astype(np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_shapes_equal_the_host(ssd, gpu_device, shape, aligned):
    w, h = shape
    src = wm.scene_src(ssd, w, h)
    r = Warper(ssd, gpu_device, _shape_frames(w, h, 1), aligned)
    try:
        ident = wm.identity_view(ssd, src)
        outs, stats = _check(ssd, r, [ident] * 3, src, "the identity")
        assert (outs == np.array(r.frames)).all(), "the identity view is a copy"
        # three views in one batch: small motion, the scene pushed away (many samples per pixel), a tilt with a shift
        mixed = [wm.seeded_views(ssd, src, 1, seed=w, max_deg=1.0, max_shift=0.02)[0], wm.push_away_view(ssd, src, 2.0),
                 wm.make_view(ssd, wm.rotation(0.0, 0.0, 2.0), (0.0, 0.0, -0.5), src)]
        _check(ssd, r, mixed, src, "three views")
        _check(ssd, r, mixed[1:2], src, "one frame")
        r.load(_shape_frames(w, h, 2))
        _check(ssd, r, mixed[::-1], _intr(ssd, src.fx * 0.5, src.fy * 0.5, src.ppx, src.ppy, 0.0005), "a target of half the focal length")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
def test_the_scene_at_256_x_192_and_pushed_away(ssd, gpu_device, aligned):
    frames = wm.scene_frames(ssd, 256, 192)
    src = wm.scene_src(ssd, 256, 192)
    r = Warper(ssd, gpu_device, list(frames), aligned)
    try:
        views = [wm.seeded_views(ssd, src)[2], wm.push_away_view(ssd, src), wm.pull_near_view(ssd, src)]
        _, stats = _check(ssd, r, views, src, "256 x 192")
        assert stats[1].n_landed > 5 * stats[1].n_filled, "the contention case: many samples per target pixel"
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
def test_every_sample_on_one_pixel_and_on_the_two_of_a_word(ssd, gpu_device, aligned):
    """where a wrong swap loop, a wrong half or a last-writer store shows: values descending, ascending and shuffled in source order"""
    w, h = 64, 48
    src = wm.scene_src(ssd, w, h)
    n = w * h
    down = (60000 - 7 * np.arange(n)).astype(np.uint16).reshape(h, w)
    up = (60000 - 7 * np.arange(n))[::-1].astype(np.uint16).reshape(h, w)
    mixed = np.random.default_rng(9).permutation(60000 - 7 * np.arange(n)).astype(np.uint16).reshape(h, w)
    r = Warper(ssd, gpu_device, [down, up, mixed], aligned)
    ident = wm.identity_view(ssd, src)
    try:
        for ppx, half in ((2.0, "the low half"), (3.0, "the high half")):
            one = _intr(ssd, 1e-6, 1e-6, ppx, 1.0)
            outs, stats = _check(ssd, r, [ident] * 3, one, "one pixel, " + half)
            for o, s in zip(outs, stats):
                assert o[1, int(ppx)] == 60000 - 7 * (n - 1) and int((o != 0).sum()) == 1 and (s.n_landed, s.n_filled) == (n, 1)
        # x / z spans (-0.7, 0.7): with fx = 1 and ppx = 2.5 the samples left of the axis land on pixel 2 and the others on pixel 3
        two = _intr(ssd, 1.0, 1e-6, 2.5, 1.0)
        outs, stats = _check(ssd, r, [ident] * 3, two, "the two pixels of a word")
        for o, s in zip(outs, stats):
            assert o[1, 2] != 0 and o[1, 3] != 0 and int((o != 0).sum()) == 2 and (s.n_landed, s.n_filled) == (n, 2)
    finally:
        r.close()


@pytest.mark.gpu
def test_per_frame_views_and_a_batch_at_max_frames_per_batch_and_one_beyond(ssd, gpu_device):
    w, h = 72, 40
    src = wm.scene_src(ssd, w, h)
    base = _shape_frames(w, h, 4)
    r = Warper(ssd, gpu_device, [base[k % 3] for k in range(9)], batch=8)
    try:
        views = [wm.make_view(ssd, np.eye(3), (0.01 * k, -0.01 * k, 0.1 * k), src) for k in range(9)]     # every frame's view differs
        before = r.det.workspace_bytes
        with pytest.raises(ssd.SsdError):
            r.det.enqueue_depth_warp(r.src.ptr, 9, views, src, r.out.ptr, r.stride, r.out_stride)
        assert r.det.workspace_bytes == before
        with pytest.raises(ssd.SsdError):
            r.det.fetch_depth_warp(1)                                  # nothing was launched: there is no pass to wait for
        outs, _ = _check(ssd, r, views[:8], src, "a full batch")
        assert len({o.tobytes() for o in outs[0::3]}) == 3, "the same frame under three views gives three frames"
        _check(ssd, r, views[5:6], src, "one frame")
    finally:
        r.close()


@pytest.fixture(scope="module")
def walk(ssd):
    """24 noisy frames of the 256 x 192 scene from the recipe's first three poses in turn, their views into the first, what detects
    them, and the host's chain: warp, fusion of every three, filter"""
    w, h = wm.ACC_W, wm.ACC_H
    poses = wm.ACC_POSES[:3]
    target = wm.pose_scene(ssd, poses[0])
    frames = ssd.synth_depth_host([wm.pose_scene(ssd, poses[i % 3], seed=1000 + i, noisy=True) for i in range(24)])
    views = [wm.pose_view(ssd, poses[i % 3], poses[0]) for i in range(24)]
    for i, v in enumerate(views):                                     # every frame's view differs (0.1 mm a frame along the axis, a third of
        v.t[2] += 1e-4 * i                                            # a raw unit): a slice or a block that reads another frame's view is seen
    assert len({bytes(v) for v in views}) == 24
    dst = ssd.intrinsics_for_scene(target)
    host = [ssd.depth_warp_host(f, v, dst) for f, v in zip(frames, views)]
    warped = np.array([o for o, _ in host])
    fused = [ssd.depth_fuse_host(np.ascontiguousarray(warped[3 * g:3 * g + 3])) for g in range(8)]
    return dict(w=w, h=h, cal=ssd.transformation_for_scene(target).constants, intr=dst, frames=frames, views=views, warped=warped,
                warp_stats=[bytes(s) for _, s in host], fused=np.array([o for o, _ in fused]), fuse_stats=[bytes(s) for _, s in fused],
                fused_filtered=np.array([ssd.depth_edges_host(o)[0] for o, _ in fused]))


def _walker(ssd, device, d, frames, in_flight, batch):
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=batch, batches_in_flight=in_flight)
    r = Warper(ssd, device, list(frames), True, cfg=cfg, cal=d["cal"])
    r.det.set_intrinsics(d["intr"])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [0, 3])
def test_the_chain_warp_fuse_edges_detect_with_no_host_wait(ssd, gpu_device, walk, in_flight):
    d = walk
    r = _walker(ssd, gpu_device, d, d["frames"][:9], in_flight, 9)
    mid = ssd.DeviceBuffer(3 * r.stride, gpu_device)
    last = ssd.DeviceBuffer(3 * r.stride, gpu_device)
    try:
        det = r.det
        want = [bytes(x) for x in det.process_depth_host(d["fused_filtered"][:3])]
        assert any(ssd.FrameResult.from_buffer_copy(x).n_steps >= 3 for x in want), "the warped, fused and filtered frames show the staircase"
        for _ in range(2):                                            # the second round takes another workspace where there are several
            det.enqueue_depth_warp(r.src.ptr, 9, d["views"][:9], d["intr"], r.out.ptr, r.stride, r.out_stride)
            groups = det.enqueue_depth_fuse(r.out.ptr, 9, 3, mid.ptr, stride_bytes=r.out_stride, out_stride_bytes=r.stride)
            det.enqueue_depth_edges(mid.ptr, groups, last.ptr, stride_bytes=r.stride, out_stride_bytes=r.stride)
            det.enqueue_depth(last.ptr, groups, stride_bytes=r.stride)           # the same (null) stream, no host wait
            assert [bytes(x) for x in det.fetch_list(3)] == want
        raw = last.download(last.nbytes)
        got = np.array([raw[g * r.stride:g * r.stride + 2 * r.points].view(np.uint16).reshape(d["h"], d["w"]) for g in range(3)])
        assert (got == d["fused_filtered"][:3]).all()
        assert [bytes(s) for s in det.fetch_depth_warp(9)] == d["warp_stats"][:9]
        assert [bytes(s) for s in det.fetch_depth_fuse(3)] == d["fuse_stats"][:3]
    finally:
        last.free()
        mid.free()
        r.close()


@pytest.mark.gpu
def test_the_host_path_over_four_slices_equals_the_host_chain(ssd, gpu_device, walk):
    d = walk
    r = _walker(ssd, gpu_device, d, d["frames"][:2], 0, 8)            # slices of 8 frames cut down to 6: 24 frames are four slices
    try:
        det = r.det
        want = [bytes(x) for x in det.process_depth_host(d["fused"])]
        res, fused, ws, fs = det.process_depth_host_warp_fused(d["frames"], 3, d["views"], d["intr"], fused=True, warp_stats=True, fuse_stats=True)
        assert [bytes(x) for x in res] == want
        assert fused.shape == d["fused"].shape and (fused == d["fused"]).all()
        assert [bytes(s) for s in ws] == d["warp_stats"] and [bytes(s) for s in fs] == d["fuse_stats"]
        assert [bytes(x) for x in det.process_depth_host_warp_fused(d["frames"], 3, d["views"], d["intr"])] == want, "without the frames and the records"
        res = det.process_depth_host_warp_fused(d["frames"][:6], 2, d["views"][:6], d["intr"], fuse_rule=ssd.FuseRule(1, 1, 20, 0))
        two = np.array([ssd.depth_fuse_host(np.ascontiguousarray(d["warped"][2 * g:2 * g + 2]), ssd.FuseRule(1, 1, 20, 0))[0] for g in range(3)])
        assert [bytes(x) for x in res] == [bytes(x) for x in det.process_depth_host(two)]
        other = ssd.Intrinsics.from_buffer_copy(d["intr"])
        other.fx += 1.0
        bad = ssd.WarpView.from_buffer_copy(d["views"][0])
        bad.t[1] = float("nan")
        for args in ((d["frames"][:6], 3, d["views"][:6], other), (d["frames"][:5], 3, d["views"][:5], d["intr"]),
                     (d["frames"][:3], 3, [bad] * 3, d["intr"]), (d["frames"][:3], 3, d["views"][:3], None)):
            with pytest.raises(ssd.SsdError):
                det.process_depth_host_warp_fused(*args)
    finally:
        r.close()


@pytest.mark.gpu
def test_two_calls_on_two_streams_with_no_host_wait(ssd, gpu_device, two_streams):  # noqa: F811
    """the order guard of test_gpu_follow_passes.py: it guards the order of the two calls, it cannot prove it"""
    a, b = two_streams
    frames, src = list(wm.scene_frames(ssd)) * 2, wm.scene_src(ssd, 64, 48)
    r = Warper(ssd, gpu_device, frames)
    try:
        first, second = wm.seeded_views(ssd, src)[:6], wm.seeded_views(ssd, src, seed=5)[:6]
        args = (r.stride, r.out_stride)
        r.det.enqueue_depth_warp(r.src.ptr, 6, first, src, r.out.ptr, *args, stream=a)
        r.det.enqueue_depth_warp(r.src.ptr, 6, second, src, r.out.ptr, *args, stream=b)          # no host wait between them
        stats = r.det.fetch_depth_warp(6)
        want_o, want_st = _want(ssd, frames, second, src)
        got = r.frames_of(r.out.download(r.out.nbytes), 6)
        assert (got == want_o).all() and not (got == _want(ssd, frames, first, src)[0]).all(), "the buffer holds the second call's frames"
        assert [bytes(s) for s in stats] == want_st
    finally:
        r.close()


@pytest.mark.gpu
def test_refusals_workspace_detection_and_time(ssd, gpu_device, walk):
    L = ssd.lib()
    d = walk
    r = _walker(ssd, gpu_device, d, d["frames"][:7], 0, 6)            # (a frame more than a batch: every refused call's ranges lie inside the buffers)
    plain = ssd.Detector(r.cfg, d["cal"], gpu_device)
    plain.set_intrinsics(d["intr"])
    odd = ssd.Detector(ssd.default_config(3, 3, max_frames_per_batch=2), d["cal"], gpu_device)
    try:
        det = r.det
        assert det.workspace_bytes == plain.workspace_bytes, "a handle that never warped holds nothing for it"
        det.enqueue_depth(r.src.ptr, 6, stride_bytes=r.stride)
        before_results = [bytes(x) for x in det.fetch_list(6)]
        before = det.workspace_bytes
        fb = 2 * r.points
        views = (ssd.WarpView * 7)(*d["views"][:7])

        def call(h=det._h, ptr=r.src.ptr, stride=r.stride, nframes=6, v=views, dst=d["intr"], out=r.out.ptr, out_stride=r.out_stride):
            return L.ssd_enqueue_depth_warp(h, C.c_void_p(ptr), stride, nframes, None, v, None if dst is None else C.byref(dst), C.c_void_p(out), out_stride)

        def bad_view(field, i, x):
            arr = (ssd.WarpView * 7)(*d["views"][:7])
            if field == "src":
                setattr(arr[5].src, i, x)
            else:
                getattr(arr[5], field)[i] = x
            return arr
        zero_units = ssd.Intrinsics.from_buffer_copy(d["intr"])
        zero_units.depth_units = 0.0
        refused = [call(h=None), call(ptr=0), call(v=None), call(dst=None), call(out=0), call(nframes=0), call(nframes=-1), call(nframes=7),
                   call(ptr=r.src.ptr + 1), call(stride=r.stride + 1), call(stride=fb - 2),
                   # the word-wide swap: an output pointer or stride that is no multiple of 4, a stride that holds no frame
                   call(out=r.out.ptr + 2), call(out=r.out.ptr + 1), call(out_stride=r.out_stride + 2), call(out_stride=fb - 4),
                   call(dst=zero_units), call(v=bad_view("r", 4, float("nan"))), call(v=bad_view("t", 2, float("inf"))), call(v=bad_view("src", "fx", 0.0)),
                   # any overlap with the input: in place, the output's first bytes on the input's last, the output's last on its first
                   call(out=r.src.ptr, out_stride=r.stride), call(nframes=1, out=r.src.ptr), call(out=r.src.ptr + 4 * r.stride, out_stride=r.stride),
                   call(ptr=r.src.ptr + 2 * r.stride, nframes=1, out=r.src.ptr + 2 * r.stride - fb + 4),
                   call(ptr=r.src.ptr, nframes=1, out=r.src.ptr + fb - 4)]
        assert refused == [-1] * len(refused)
        # a frame with an odd number of pixels has a last pixel whose word is not the frame's own
        one = (ssd.WarpView * 1)(wm.identity_view(ssd, d["intr"]))
        assert L.ssd_enqueue_depth_warp(odd._h, C.c_void_p(r.src.ptr), 32, 1, None, one, C.byref(d["intr"]), C.c_void_p(r.out.ptr), 32) == -1
        assert b"even" in L.ssd_last_error()
        assert det.workspace_bytes == before, "a refused call allocates nothing"
        with pytest.raises(ssd.SsdError):
            det.fetch_depth_warp(1)                                   # ... and launched nothing: there is no pass to wait for
        assert L.ssd_get_depth_warp_time(det._h, C.byref(C.c_float())) == -1
        assert call() == 0
        after = det.workspace_bytes
        assert after - before == 2 * 6 * (C.sizeof(ssd.WarpStats) + C.sizeof(ssd.WarpView)), "exactly the records and the views, on the device and pinned"
        assert [bytes(s) for s in det.fetch_depth_warp(6)] == d["warp_stats"][:6]
        assert det.depth_warp_time_ms() == 0.0, "timing was off for it"
        assert [bytes(x) for x in det.fetch_list(6)] == before_results, "the detection's results are untouched by an interleaved warp"
        det.set_timing(True)
        assert call(nframes=2) == 0 and det.workspace_bytes == after, "made once"
        assert [bytes(s) for s in det.fetch_depth_warp(1)] == d["warp_stats"][:1]
        assert 0.0 < det.depth_warp_time_ms() < 1000.0
        with pytest.raises(ssd.SsdError):
            det.fetch_depth_warp(3)
        assert [bytes(x) for x in det.fetch_list(6)] == before_results
        assert plain.workspace_bytes == before
        got = r.frames_of(r.out.download(r.out.nbytes), 2)
        assert (got == d["warped"][:2]).all()
    finally:
        odd.close()
        plain.close()
        r.close()
