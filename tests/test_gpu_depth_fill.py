"""The depth fill on the GPU (ssd_enqueue_depth_fill / ssd_fetch_depth_fill / ssd_get_depth_fill_time / ssd_process_depth_host_fill /
ssd_process_depth_host_warp_fill_fused; include/ssd_hip.h).  Every comparison is bytes against ssd_depth_fill_host,
which tests/test_depth_fill.py holds to the numpy restatement of the rule, and every byte of the output and class buffers outside the
frames is checked untouched behind a fill pattern.

k_depth_fill walks k_depth_edges' layout (csrc/ssd_k_edges.h), so the shapes are those at which that stencil goes wrong:
  a lane's strip        8 pixels          widths 7, 8, 9
  a wave's row span     64 x 8 = 512      widths 511, 512, 513
  a block's row span    4 x 512 = 2048    2047 x 2, 2049 x 3
  the tile height       32 rows           heights 31, 32, 33, and 65 (two seams and a tile of one row)
  heights 1, 2, 3 (no row above and below, one of them, both), and 1 x 1, the smallest frame ssd_create accepts.
The wide body wants a width that is a multiple of 8 beside the 16-byte alignment: every other width takes the narrow body at either
alignment.  The content: seeded frames at 10 % and 60 % zeros with holes and one-pixel slits planted on the strip, wave, block and tile
seams (tests/fill_model.py: seeded_frame)."""
import ctypes as C

import numpy as np
import pytest

import fill_model as fm
import warp_model as wm
from test_gpu_depth_edges import FILL, SPAN, STRIP, TILE, Filter
from test_gpu_follow_passes import two_streams  # noqa: F401  (a fixture)

WIDTHS, HEIGHTS = (7, 8, 9, 511, 512, 513), (1, 2, 3, 31, 32, 33, 65)
SHAPES = [(w, h) for w in WIDTHS for h in HEIGHTS] + [(1, 1), (2047, 2), (2049, 3)]
OTHER = dict(min_pairs=2, cover=2, tol=25, slope=32)


class Filler(Filter):
    """test_gpu_depth_edges.py's resident batch - the frames, the output and the class buffer at strides wider than a frame, on 16-byte
    or on 2-byte boundaries only - through the fill"""

    def run(self, nframes, rule=None, classes=True, stream=None):
        """-> (filled frames [n, H, W], classes [n, H, W] or None, stats); everything outside the frames' pixels is untouched"""
        for buf in (self.out, self.cls):
            buf.upload(np.full(buf.nbytes, FILL, np.uint8))
        self.det.enqueue_depth_fill(self.src.ptr + self.lead, nframes, self.out.ptr + self.lead, rule, self.cls.ptr + self.lead if classes else None,
                                    self.stride, self.out_stride, self.cls_stride, stream)
        stats = self.det.fetch_depth_fill(nframes)
        raw, outs, cls = self.out.download(self.out.nbytes), [], []
        touched = np.zeros(self.out.nbytes, bool)
        for g in range(nframes):
            at = self.lead + g * self.out_stride
            outs.append(raw[at:at + 2 * self.points].view(np.uint16).copy().reshape(self.shape))
            touched[at:at + 2 * self.points] = True
        assert (raw[~touched] == FILL).all(), "a byte outside the filled frames was written"
        raws = self.cls.download(self.cls.nbytes)
        touched = np.zeros(self.cls.nbytes, bool)
        for g in range(nframes if classes else 0):
            at = self.lead + g * self.cls_stride
            cls.append(raws[at:at + self.points].copy().reshape(self.shape))
            touched[at:at + self.points] = True
        assert (raws[~touched] == FILL).all(), "a byte outside the class maps was written"
        return np.array(outs), np.array(cls) if classes else None, stats

    def frames_of(self, buf, stride, n):
        raw = buf.download(buf.nbytes)
        return np.array([raw[g * stride:g * stride + 2 * self.points].view(np.uint16).reshape(self.shape) for g in range(n)])


def _rule(ssd, r):
    return None if r is None else fm.make_rule(ssd, r)


def _want(ssd, frames, rule):
    got = [ssd.depth_fill_host(f, _rule(ssd, rule), classes=True) for f in frames]
    return np.array([o for o, _, _ in got]), np.array([c for _, _, c in got]), [bytes(st) for _, st, _ in got]


def _check(ssd, r, nframes, rule=None, classes=True, what=""):
    outs, cls, stats = r.run(nframes, _rule(ssd, rule), classes)
    want_o, want_c, want_st = _want(ssd, r.frames[:nframes], rule)
    bad = np.argwhere(outs != want_o)
    assert len(bad) == 0, "%s: the filled frames differ at (frame, row, column) %s ..." % (what, bad[:5].tolist())
    if classes:
        bad = np.argwhere(cls != want_c)
        assert len(bad) == 0, "%s: the class maps differ at %s ..." % (what, bad[:5].tolist())
    assert [bytes(s) for s in stats] == want_st, "%s: the frames' records" % what
    return stats


def _content(w, h):
    return [fm.seeded_frame(w, h, 0.1, seed=5), fm.seeded_frame(w, h, 0.6, seed=6), fm.seeded_frame(w, h, 0.1, seed=7, seams=False)]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_shapes_equal_the_host(ssd, gpu_device, shape, aligned):
    w, h = shape
    r = Filler(ssd, gpu_device, _content(w, h), aligned)
    try:
        stats = _check(ssd, r, 3, None, True, "defaults")
        assert all(s.n_kept + s.n_empty + s.n_filled + s.n_covered == w * h for s in stats)
        if w * h >= 200:
            assert all(s.n_filled > 0 for s in stats) and stats[0].n_covered > 0, "the frames exercise the classes"
        _check(ssd, r, 3, None, False, "defaults, no class map")
        _check(ssd, r, 2, OTHER, True, str(OTHER))
        _check(ssd, r, 1, dict(min_pairs=1, cover=1, tol=65535, slope=4096), False, "the widest rule")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
@pytest.mark.parametrize("rule", fm.RULES, ids=[str(sorted(r.items())) for r in fm.RULES])
def test_the_rule_variants_on_one_frame(ssd, gpu_device, rule, aligned):
    r = Filler(ssd, gpu_device, [fm.seeded_frame(513, 33, 0.1, seed=21), fm.seeded_frame(513, 33, 0.6, seed=22)], aligned)
    try:
        _check(ssd, r, 2, rule, True, str(rule))
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
def test_the_hand_made_frames_equal_the_host(ssd, gpu_device, aligned):
    """the hand-made frames of tests/fill_model.py: in their own shape, and - a pixel that does not exist is an invalid one to the rule -
    set into a frame of zeros with their centres on and beside the strip, wave and tile seams and in the frame's corners, where the
    centre named by hand must come out as stated too"""
    hand = fm.hand_frames()
    W, H = 528, 40
    # centres in the corners, on both sides of a strip seam (7 | 8, 15 | 16), of the wave seam (511 | 512) and of the tile seam (31 | 32)
    spots = [(1, 1), (1, STRIP - 1), (1, SPAN - 1), (1, W - 2), (5, STRIP), (5, SPAN), (5, 100), (TILE - 1, 2 * STRIP - 1), (TILE - 1, 300),
             (TILE - 1, SPAN), (TILE, STRIP), (TILE, 3 * STRIP), (36, SPAN - 1), (H - 2, 1), (H - 2, W - 2), (H - 2, 300)]
    own = Filler(ssd, gpu_device, [hand[0][2], hand[0][2]], aligned)
    big = Filler(ssd, gpu_device, [np.zeros((H, W), np.uint16)], aligned)
    try:
        for name, rule, f, want, want_cls in hand:
            own.load([f, f[::-1, ::-1].copy()])
            outs, cls, _ = own.run(2, _rule(ssd, rule), True)
            want_o, want_c, _ = _want(ssd, own.frames, rule)
            assert (outs == want_o).all() and (cls == want_c).all(), name
            assert [(int(o[1, 1]), int(c[1, 1])) for o, c in zip(outs, cls)] == [(want, want_cls)] * 2, name
        keys = []
        for case in hand:
            if case[1] not in keys:
                keys.append(case[1])
        for key in keys:                                              # one launch per rule: the frames of that rule tiled across the seams
            group = [c for c in hand if c[1] == key]
            for first in range(0, len(group), len(spots)):
                some = group[first:first + len(spots)]
                g, marks = fm.set_across((some * len(spots))[:len(spots)], W, H, spots)      # every spot taken, by the same frames again
                big.load([g])
                outs, cls, _ = big.run(1, _rule(ssd, key), True)
                want_o, want_c, _ = _want(ssd, [g], key)
                assert (outs == want_o).all() and (cls == want_c).all(), key
                for y, x, o, c, name in marks:
                    assert (int(outs[0][y, x]), int(cls[0][y, x])) == (o, c), "%s at %s" % (name, (y, x))
        for name, f, want in fm.border_frames():
            if f.shape == (3, 3):
                own.load([f, f])
                outs, _, _ = own.run(2, None, True)
                assert (outs[0] == want).all(), name
    finally:
        big.close()
        own.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (1, 2), (2, 2), (1, 1)], ids=lambda s: "%dx%d" % s)
def test_one_row_one_column_and_the_smallest_frames(ssd, gpu_device, shape):
    h, w = shape
    for name, f, want in fm.border_frames():
        if f.shape == (h, w):
            r = Filler(ssd, gpu_device, [f, f], False)
            try:
                outs, _, _ = r.run(2, None, True)
                assert (outs[0] == want).all() and (outs[1] == want).all(), name
                _check(ssd, r, 2, None, True, name)
            finally:
                r.close()


@pytest.mark.gpu
def test_a_batch_at_max_frames_per_batch_and_one_beyond(ssd, gpu_device):
    frames = [fm.seeded_frame(72, 40, 0.1 + 0.05 * s, seed=s) for s in range(9)]
    r = Filler(ssd, gpu_device, frames, batch=8)
    try:
        before = r.det.workspace_bytes
        with pytest.raises(ssd.SsdError):
            r.det.enqueue_depth_fill(r.src.ptr, 9, r.out.ptr, None, None, r.stride, r.out_stride)
        assert r.det.workspace_bytes == before
        with pytest.raises(ssd.SsdError):
            r.det.fetch_depth_fill(1)                                 # nothing was launched: there is no pass to wait for
        stats = _check(ssd, r, 8)
        assert len({bytes(s) for s in stats}) == 8, "every frame has a record of its own"
        _check(ssd, r, 8, classes=False)
        _check(ssd, r, 1)
    finally:
        r.close()


@pytest.fixture(scope="module")
def walk(ssd):
    """24 noisy frames of the 256 x 192 scene from the recipe's first three poses in turn, a view of its own per frame into the first
    pose, what detects them, and the host's chain: warp, fill, fusion of every three, edge filter"""
    w, h = wm.ACC_W, wm.ACC_H
    poses = wm.ACC_POSES[:3]
    target = wm.pose_scene(ssd, poses[0])
    frames = ssd.synth_depth_host([wm.pose_scene(ssd, poses[i % 3], seed=1000 + i, noisy=True) for i in range(24)])
    views = [wm.pose_view(ssd, poses[i % 3], poses[0]) for i in range(24)]
    for i, v in enumerate(views):                                     # every frame's view differs (0.1 mm a frame along the axis, a third of
        v.t[2] += 1e-4 * i                                            # a raw unit): a slice or a block that reads another frame's view is seen
    dst = ssd.intrinsics_for_scene(target)
    host = [ssd.depth_warp_host(f, v, dst) for f, v in zip(frames, views)]
    warped = np.array([o for o, _ in host])
    fills = [ssd.depth_fill_host(o) for o in warped]
    filled = np.array([o for o, _ in fills])
    fused = [ssd.depth_fuse_host(np.ascontiguousarray(filled[3 * g:3 * g + 3])) for g in range(8)]
    assert not (filled == warped).all()
    return dict(w=w, h=h, cal=ssd.transformation_for_scene(target).constants, intr=dst, frames=frames, views=views, warped=warped, filled=filled,
                warp_stats=[bytes(s) for _, s in host], fill_stats=[bytes(s) for _, s in fills], fused=np.array([o for o, _ in fused]),
                fuse_stats=[bytes(s) for _, s in fused], fused_filtered=np.array([ssd.depth_edges_host(o)[0] for o, _ in fused]),
                frames_filled=[ssd.depth_fill_host(f) for f in frames])


def _walker(ssd, device, d, frames, in_flight, batch):
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=batch, batches_in_flight=in_flight)
    r = Filler(ssd, device, list(frames), True, cfg=cfg, cal=d["cal"])
    r.det.set_intrinsics(d["intr"])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [0, 3])
def test_the_chain_warp_fill_fuse_edges_detect_with_no_host_wait(ssd, gpu_device, walk, in_flight):
    d = walk
    r = _walker(ssd, gpu_device, d, d["frames"][:9], in_flight, 9)
    warped = ssd.DeviceBuffer(9 * r.stride, gpu_device)
    mid = ssd.DeviceBuffer(3 * r.stride, gpu_device)
    last = ssd.DeviceBuffer(3 * r.stride, gpu_device)
    try:
        det = r.det
        want = [bytes(x) for x in det.process_depth_host(d["fused_filtered"][:3])]
        assert any(ssd.FrameResult.from_buffer_copy(x).n_steps >= 3 for x in want), "the warped, filled, fused and filtered frames show the staircase"
        for _ in range(2):                                            # the second round takes another workspace where there are several
            det.enqueue_depth_warp(r.src.ptr, 9, d["views"][:9], d["intr"], warped.ptr, r.stride, r.stride)
            det.enqueue_depth_fill(warped.ptr, 9, r.out.ptr, stride_bytes=r.stride, out_stride_bytes=r.out_stride)
            groups = det.enqueue_depth_fuse(r.out.ptr, 9, 3, mid.ptr, stride_bytes=r.out_stride, out_stride_bytes=r.stride)
            det.enqueue_depth_edges(mid.ptr, groups, last.ptr, stride_bytes=r.stride, out_stride_bytes=r.stride)
            det.enqueue_depth(last.ptr, groups, stride_bytes=r.stride)           # the same (null) stream, no host wait
            assert [bytes(x) for x in det.fetch_list(3)] == want
        assert (r.frames_of(last, r.stride, 3) == d["fused_filtered"][:3]).all()
        assert (r.frames_of(r.out, r.out_stride, 9) == d["filled"][:9]).all()
        assert [bytes(s) for s in det.fetch_depth_warp(9)] == d["warp_stats"][:9]
        assert [bytes(s) for s in det.fetch_depth_fill(9)] == d["fill_stats"][:9]
        assert [bytes(s) for s in det.fetch_depth_fuse(3)] == d["fuse_stats"][:3]
    finally:
        last.free()
        mid.free()
        warped.free()
        r.close()


@pytest.mark.gpu
def test_the_host_paths_over_four_slices_equal_the_host_chain(ssd, gpu_device, walk):
    d = walk
    r = _walker(ssd, gpu_device, d, d["frames"][:2], 0, 8)            # slices of 8 frames, cut down to 6 for groups of 3: 24 frames are four slices
    try:
        det = r.det
        # warp, fill, fuse, detect
        want = [bytes(x) for x in det.process_depth_host(d["fused"])]
        res, fused, ws, ls, fs = det.process_depth_host_warp_fill_fused(d["frames"], 3, d["views"], d["intr"], fused=True, warp_stats=True,
                                                                        fill_stats=True, fuse_stats=True)
        assert [bytes(x) for x in res] == want
        assert fused.shape == d["fused"].shape and (fused == d["fused"]).all()
        assert [bytes(s) for s in ws] == d["warp_stats"] and [bytes(s) for s in ls] == d["fill_stats"] and [bytes(s) for s in fs] == d["fuse_stats"]
        assert [bytes(x) for x in det.process_depth_host_warp_fill_fused(d["frames"], 3, d["views"], d["intr"])] == want, "without the frames and the records"
        unfilled = det.process_depth_host_warp_fused(d["frames"], 3, d["views"], d["intr"], fused=True)[1]
        assert not (unfilled == fused).all(), "ssd_process_depth_host_warp_fused is the chain without the fill"
        rule, fuse_rule = fm.make_rule(ssd, OTHER), ssd.FuseRule(1, 1, 20, 0)
        res, ls = det.process_depth_host_warp_fill_fused(d["frames"][:6], 2, d["views"][:6], d["intr"], fill_rule=rule, fuse_rule=fuse_rule, fill_stats=True)
        other = [ssd.depth_fill_host(f, rule) for f in d["warped"][:6]]
        two = np.array([ssd.depth_fuse_host(np.ascontiguousarray(np.array([o for o, _ in other[2 * g:2 * g + 2]])), fuse_rule)[0] for g in range(3)])
        assert [bytes(x) for x in res] == [bytes(x) for x in det.process_depth_host(two)] and [bytes(s) for s in ls] == [bytes(s) for _, s in other]
        bad_intr = ssd.Intrinsics.from_buffer_copy(d["intr"])
        bad_intr.fx += 1.0
        for kw in (dict(fill_rule=ssd.FillRule(0, 1, 40, 0)), dict(fill_rule=ssd.FillRule(1, 5, 40, 0)), dict(fuse_rule=ssd.FuseRule(4, 1, 20, 0)),
                   dict(dst=bad_intr), dict(n=4)):
            args = dict(dict(n=3, dst=d["intr"]), **kw)
            with pytest.raises(ssd.SsdError):
                det.process_depth_host_warp_fill_fused(d["frames"][:6], args.pop("n"), d["views"][:6], args.pop("dst"), **args)
        # fill, detect: groups of one
        host = d["frames_filled"]
        alone = np.array([o for o, _ in host])
        want = [bytes(x) for x in det.process_depth_host(alone)]
        res, filled, stats = det.process_depth_host_fill(d["frames"], filled=True, stats=True)
        assert [bytes(x) for x in res] == want and filled.shape == alone.shape and (filled == alone).all()
        assert [bytes(s) for s in stats] == [bytes(s) for _, s in host]
        assert [bytes(x) for x in det.process_depth_host_fill(d["frames"])] == want, "without the frames and the records"
        res = det.process_depth_host_fill(d["frames"][:11], rule=rule)
        want_o = np.array([ssd.depth_fill_host(f, rule)[0] for f in d["frames"][:11]])
        assert [bytes(x) for x in res] == [bytes(x) for x in det.process_depth_host(want_o)]
        with pytest.raises(ssd.SsdError):
            det.process_depth_host_fill(d["frames"][:3], rule=ssd.FillRule(5, 1, 40, 0))
    finally:
        r.close()


@pytest.mark.gpu
def test_two_calls_on_two_streams_with_no_host_wait(ssd, gpu_device, two_streams):  # noqa: F811
    """the order guard of test_gpu_follow_passes.py: it guards the order of the two calls, it cannot prove it"""
    a, b = two_streams
    frames = [fm.seeded_frame(64, 48, 0.3, seed=100 + s) for s in range(8)]
    r = Filler(ssd, gpu_device, frames)
    try:
        args = dict(stride_bytes=r.stride, out_stride_bytes=r.out_stride)
        second = dict(min_pairs=2, cover=0, tol=5, slope=0)
        r.det.enqueue_depth_fill(r.src.ptr, 8, r.out.ptr, stream=a, **args)
        r.det.enqueue_depth_fill(r.src.ptr, 8, r.out.ptr, rule=_rule(ssd, second), stream=b, **args)      # no host wait between them
        stats = r.det.fetch_depth_fill(8)
        want_o, _, want_st = _want(ssd, frames, second)
        first_o, _, _ = _want(ssd, frames, None)
        got = r.frames_of(r.out, r.out_stride, 8)
        assert (got == want_o).all() and not (got == first_o).all(), "the buffer holds the second call's frames"
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
    try:
        det = r.det
        assert det.workspace_bytes == plain.workspace_bytes, "a handle that never filled holds nothing for it"
        det.enqueue_depth(r.src.ptr, 6, stride_bytes=r.stride)
        before_results = [bytes(x) for x in det.fetch_list(6)]
        before = det.workspace_bytes
        fb = 2 * r.points

        def call(h=det._h, ptr=r.src.ptr, stride=r.stride, nframes=6, rule=None, out=r.out.ptr, out_stride=r.out_stride, cls=0, cls_stride=0):
            return L.ssd_enqueue_depth_fill(h, C.c_void_p(ptr), stride, nframes, None, None if rule is None else C.byref(rule), C.c_void_p(out),
                                            out_stride, C.c_void_p(cls), cls_stride)
        R = ssd.FillRule
        refused = [call(h=None), call(ptr=0), call(out=0), call(nframes=0), call(nframes=-1), call(nframes=7),
                   call(rule=R(0, 1, 40, 0)), call(rule=R(5, 1, 40, 0)), call(rule=R(1, -1, 40, 0)), call(rule=R(1, 5, 40, 0)), call(rule=R(1, 1, -1, 0)),
                   call(rule=R(1, 1, 65536, 0)), call(rule=R(1, 1, 40, -1)), call(rule=R(1, 1, 40, 4097)),
                   call(ptr=r.src.ptr + 1), call(stride=r.stride + 1), call(stride=fb - 2),
                   call(out=r.out.ptr + 1), call(out_stride=fb - 2), call(out_stride=fb + 1), call(cls=r.cls.ptr, cls_stride=r.points - 1),
                   # any overlap with the input: in place, the output's first byte on the input's last, the output's last on its first,
                   # and the class map likewise
                   call(out=r.src.ptr), call(nframes=1, out=r.src.ptr), call(out=r.src.ptr + 4 * r.stride),
                   call(ptr=r.src.ptr + 2 * r.stride, nframes=1, out=r.src.ptr + 2 * r.stride - fb + 2),
                   call(ptr=r.src.ptr, nframes=1, out=r.src.ptr + fb - 2),
                   call(ptr=r.src.ptr + 2 * r.stride, nframes=1, cls=r.src.ptr + 2 * r.stride - r.points + 1, cls_stride=r.cls_stride),
                   call(ptr=r.src.ptr, nframes=1, cls=r.src.ptr + fb - 1, cls_stride=r.cls_stride)]
        assert refused == [-1] * len(refused)
        assert det.workspace_bytes == before, "a refused call allocates nothing"
        with pytest.raises(ssd.SsdError):
            det.fetch_depth_fill(1)                                   # ... and launched nothing: there is no pass to wait for
        assert L.ssd_get_depth_fill_time(det._h, C.byref(C.c_float())) == -1
        assert call() == 0
        after = det.workspace_bytes
        assert after - before == 2 * 6 * C.sizeof(ssd.FillStats), "exactly the records, on the device and pinned"
        want = [bytes(s) for _, s in d["frames_filled"]]
        assert [bytes(s) for s in det.fetch_depth_fill(6)] == want[:6]
        assert det.depth_fill_time_ms() == 0.0, "timing was off for it"
        assert [bytes(x) for x in det.fetch_list(6)] == before_results, "the detection's results are untouched by an interleaved fill"
        det.set_timing(True)
        assert call(nframes=2, cls=r.cls.ptr, cls_stride=r.cls_stride) == 0 and det.workspace_bytes == after, "made once"
        assert [bytes(s) for s in det.fetch_depth_fill(1)] == want[:1]
        assert 0.0 < det.depth_fill_time_ms() < 1000.0
        with pytest.raises(ssd.SsdError):
            det.fetch_depth_fill(3)
        assert [bytes(x) for x in det.fetch_list(6)] == before_results
        assert plain.workspace_bytes == before
        assert (r.frames_of(r.out, r.out_stride, 2) == np.array([o for o, _ in d["frames_filled"][:2]])).all()
    finally:
        plain.close()
        r.close()
