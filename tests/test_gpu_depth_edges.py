"""The depth edge filter on the GPU (ssd_enqueue_depth_edges / ssd_fetch_depth_edges / ssd_get_depth_edges_time /
ssd_process_depth_host_edges; include/ssd_hip.h).  Every comparison is bytes against ssd_depth_edges_host, which
tests/test_depth_edges.py holds to the numpy restatement of the rule, and every byte of the output and class buffers outside the frames is
checked untouched behind a fill pattern.

The shapes are those at which a stencil goes wrong, derived from k_depth_edges' layout (csrc/ssd_k_edges.h):
  a lane's strip        8 pixels          widths 7, 8, 9
  a wave's row span     64 x 8 = 512      widths 511, 512, 513
  a block's row span    4 x 512 = 2048    widths 2047, 2048, 2049 (a block's four waves take neighbouring spans of one row tile)
  the tile height       32 rows           heights 31, 32, 33, and 65 (two seams and a tile of one row)
  heights 1, 2, 3 (no row above and below, one of them, both), and 1 x 1, the smallest frame ssd_create accepts.
The wide body wants a width that is a multiple of 8 beside the 16-byte alignment (rows are packed): every other width takes the narrow
body at either alignment, where every row ends in a partial strip."""
import ctypes as C

import numpy as np
import pytest

import edges_model as em
import fuse_model as fm
from test_gpu_follow_passes import two_streams  # noqa: F401  (a fixture)

FILL = 0xAB
STRIP, SPAN, BLOCK, TILE = 8, 512, 2048, 32
SHAPES = [(7, 3), (8, 3), (9, 3), (511, 3), (512, 3), (513, 3), (2047, 3), (2048, 3), (2049, 3), (24, 1), (24, 2), (520, 31), (520, 32), (520, 33),
          (16, 65), (1, 1), (64, 48), (256, 192)]
OTHER = (3, 1, 40, 64)


class Filter:
    """a batch of depth frames resident on the device behind one detector, the output and the class buffer, all of them at pointers and
    strides that are multiples of 16 bytes (the wide body, where the width allows it) or of 2 only (the narrow one); the strides are
    wider than a frame either way"""

    def __init__(self, ssd, device, frames, aligned=True, batch=None, cfg=None, cal=None):
        self.ssd, self.frames, self.total = ssd, frames, len(frames)
        h, w = frames[0].shape
        if cfg is None:
            cfg = ssd.default_config(w, h, max_frames_per_batch=batch or max(self.total, 2))
        self.cfg, self.points, self.shape = cfg, w * h, (h, w)
        self.det = ssd.Detector(cfg, cal if cal is not None else ssd.GeometricTransformation().constants, device)
        fb = self.points * 2
        pad = 32 if aligned else 6
        self.lead = 0 if aligned else 2
        self.stride = (fb + 15) // 16 * 16 + pad
        self.out_stride = (fb + 15) // 16 * 16 + pad
        self.cls_stride = (self.points + 15) // 16 * 16 + (8 if aligned else 3)
        assert (self.stride % 16 == 0) == aligned
        self.src = ssd.DeviceBuffer(self.lead + self.stride * self.total, device)
        self.out = ssd.DeviceBuffer(self.lead + self.out_stride * self.total, device)
        self.cls = ssd.DeviceBuffer(self.lead + self.cls_stride * self.total, device)
        self.load(frames)

    def load(self, frames):
        self.frames = frames
        for i, f in enumerate(frames):
            self.src.upload(np.ascontiguousarray(f), offset=self.lead + i * self.stride)

    def run(self, nframes, rule=None, classes=True, stream=None):
        """-> (filtered frames [n, H, W], classes [n, H, W] or None, stats); everything outside the frames' pixels is untouched"""
        for buf in (self.out, self.cls):
            buf.upload(np.full(buf.nbytes, FILL, np.uint8))
        self.det.enqueue_depth_edges(self.src.ptr + self.lead, nframes, self.out.ptr + self.lead, rule, self.cls.ptr + self.lead if classes else None,
                                     self.stride, self.out_stride, self.cls_stride, stream)
        stats = self.det.fetch_depth_edges(nframes)
        raw, outs, cls = self.out.download(self.out.nbytes), [], []
        touched = np.zeros(self.out.nbytes, bool)
        for g in range(nframes):
            at = self.lead + g * self.out_stride
            outs.append(raw[at:at + 2 * self.points].view(np.uint16).copy().reshape(self.shape))
            touched[at:at + 2 * self.points] = True
        assert (raw[~touched] == FILL).all(), "a byte outside the filtered frames was written"
        raws = self.cls.download(self.cls.nbytes)
        touched = np.zeros(self.cls.nbytes, bool)
        for g in range(nframes if classes else 0):
            at = self.lead + g * self.cls_stride
            cls.append(raws[at:at + self.points].copy().reshape(self.shape))
            touched[at:at + self.points] = True
        assert (raws[~touched] == FILL).all(), "a byte outside the class maps was written"
        return np.array(outs), np.array(cls) if classes else None, stats

    def close(self):
        for b in (self.src, self.out, self.cls):
            b.free()
        self.det.close()


def _want(ssd, frames, rule):
    got = [ssd.depth_edges_host(f, rule, classes=True) for f in frames]
    return np.array([o for o, _, _ in got]), np.array([c for _, _, c in got]), [bytes(st) for _, st, _ in got]


def _check(ssd, r, nframes, rule=None, classes=True, what=""):
    outs, cls, stats = r.run(nframes, rule, classes)
    want_o, want_c, want_st = _want(ssd, r.frames[:nframes], rule)
    bad = np.argwhere(outs != want_o)
    assert len(bad) == 0, "%s: the filtered frames differ at (frame, row, column) %s ..." % (what, bad[:5].tolist())
    if classes:
        bad = np.argwhere(cls != want_c)
        assert len(bad) == 0, "%s: the class maps differ at %s ..." % (what, bad[:5].tolist())
    assert [bytes(s) for s in stats] == want_st, "%s: the frames' records" % what
    return stats


def _seams(w, h):
    return [x for x in range(0, w + 1, STRIP) if x % SPAN == 0 or x % SPAN == STRIP or x % 64 == 0] + [w], [y for y in range(0, h + 1, TILE)] + [h]


def _content(ssd, w, h):
    """the scene where the shape holds one, else a seam frame; then seam frames, whose planted pixels sit on the strip, wave, block and
    tile seams and on the frame's last column and row"""
    sx, sy = _seams(w, h)
    first = em.stress_frame(ssd, w, h) if w >= 64 and h >= 48 else em.seam_frame(w, h, sx, sy, seed=5)
    dense = em.seam_frame(w, h, list(range(0, w + 1, STRIP)), sy, seed=6)
    return [first, em.seam_frame(w, h, sx, sy, seed=7), dense]


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_the_shapes_equal_the_host(ssd, gpu_device, shape, aligned):
    w, h = shape
    r = Filter(ssd, gpu_device, _content(ssd, w, h), aligned)
    try:
        stats = _check(ssd, r, 3, None, True, "defaults")
        assert all(s.n_kept + s.n_empty + s.n_lone + s.n_bridge == w * h for s in stats)
        _check(ssd, r, 3, None, False, "defaults, no class map")
        _check(ssd, r, 2, ssd.EdgeRule(*OTHER), True, str(OTHER))
        _check(ssd, r, 1, ssd.EdgeRule(8, 1, 65535, 4096), False, "the widest rule")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "2B"])
def test_the_hand_made_frames_equal_the_host(ssd, gpu_device, aligned):
    """the hand-made frames of tests/test_depth_edges.py: in their own shape, and - a pixel that does not exist is an invalid one to the
    rule - set into frames of zeros at the frame's corners and across the strip, wave and tile seams, where the pixels named by hand must
    come out as stated too"""
    hand = em.hand_frames()
    W, H = 528, 40
    places = ((0, 0), (H - 3, W - 3), (TILE - 1, SPAN - 1), (TILE - 2, STRIP - 1), (0, SPAN - 2))
    big = Filter(ssd, gpu_device, [np.zeros((H, W), np.uint16)] * len(places), aligned)
    own = {}
    try:
        for name, f, rule, want in hand:
            fh, fw = f.shape
            R = em.rule_of(ssd, rule)
            if (fh, fw) not in own:
                own[(fh, fw)] = Filter(ssd, gpu_device, [f, f], aligned)
            r = own[(fh, fw)]
            r.load([f, f[::-1, ::-1].copy()])
            _check(ssd, r, 2, R, True, name)
            frames, at = [], []
            for y, x in places:
                y, x = min(y, H - fh), min(x, W - fw)
                g = np.zeros((H, W), np.uint16)
                g[y:y + fh, x:x + fw] = f
                frames.append(g)
                at.append((y, x))
            big.load(frames)
            outs, cls, _ = big.run(len(places), R, True)
            want_o, want_c, _ = _want(ssd, frames, R)
            assert (outs == want_o).all() and (cls == want_c).all(), name
            for k, (y, x) in enumerate(at):
                for (py, px), (o, c) in want.items():
                    assert (int(outs[k][y + py, x + px]), int(cls[k][y + py, x + px])) == (o, c), "%s at %s" % (name, (y, x))
    finally:
        big.close()
        for r in own.values():
            r.close()


@pytest.mark.gpu
def test_a_batch_at_max_frames_per_batch_and_one_beyond(ssd, gpu_device):
    frames = [em.seam_frame(72, 40, [8, 64], [32], seed=s) for s in range(9)]
    r = Filter(ssd, gpu_device, frames, batch=8)
    try:
        before = r.det.workspace_bytes
        with pytest.raises(ssd.SsdError):
            r.det.enqueue_depth_edges(r.src.ptr, 9, r.out.ptr, None, None, r.stride, r.out_stride)
        assert r.det.workspace_bytes == before
        with pytest.raises(ssd.SsdError):
            r.det.fetch_depth_edges(1)                                # nothing was launched: there is no pass to wait for
        _check(ssd, r, 8)
        _check(ssd, r, 8, classes=False)
        _check(ssd, r, 1)
    finally:
        r.close()


@pytest.fixture(scope="module")
def stairs(ssd):
    """27 frames of the still 256 x 192 scene, what detects them, the host's fusion of every three and the host's filter over those"""
    w, h = 256, 192
    sc = ssd.make_scene(w, h, n_steps=3, seed=1000, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02)
    frames = fm.scene_frames(ssd, w, h, 27)
    fused = np.array([ssd.depth_fuse_host(np.ascontiguousarray(frames[3 * g:3 * g + 3]))[0] for g in range(9)])
    return dict(w=w, h=h, cal=ssd.transformation_for_scene(sc).constants, intr=ssd.intrinsics_for_scene(sc), frames=frames, fused=fused,
                fused_filtered=np.array([ssd.depth_edges_host(f)[0] for f in fused]), filtered=np.array([ssd.depth_edges_host(f)[0] for f in frames]))


def _stairs_filter(ssd, device, d, frames, in_flight, batch):
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=batch, batches_in_flight=in_flight)
    r = Filter(ssd, device, list(frames), True, cfg=cfg, cal=d["cal"])
    r.det.set_intrinsics(d["intr"])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [0, 3])
def test_the_chain_fuse_edges_detect_with_no_host_wait(ssd, gpu_device, stairs, in_flight):
    d = stairs
    r = _stairs_filter(ssd, gpu_device, d, d["frames"][:9], in_flight, 9)
    mid = ssd.DeviceBuffer(3 * r.stride, gpu_device)
    labels = ssd.DeviceBuffer(3 * d["w"] * d["h"], gpu_device)
    try:
        det = r.det
        want = [bytes(x) for x in det.process_depth_host(d["fused_filtered"][:3])]
        assert any(ssd.FrameResult.from_buffer_copy(x).n_steps >= 3 for x in want), "the filtered frames show the staircase"
        for _ in range(2):                                            # the second round takes another workspace where there are several
            groups = det.enqueue_depth_fuse(r.src.ptr, 9, 3, mid.ptr, stride_bytes=r.stride, out_stride_bytes=r.stride)
            det.enqueue_depth_edges(mid.ptr, groups, r.out.ptr, stride_bytes=r.stride, out_stride_bytes=r.out_stride)
            det.enqueue_depth(r.out.ptr, groups, stride_bytes=r.out_stride)       # the same (null) stream, no host wait
            assert [bytes(x) for x in det.fetch_list(3)] == want
        det.enqueue_depth_fuse(r.src.ptr, 9, 3, mid.ptr, stride_bytes=r.stride, out_stride_bytes=r.stride)
        det.enqueue_depth_edges(mid.ptr, 3, r.out.ptr, stride_bytes=r.stride, out_stride_bytes=r.out_stride)
        det.enqueue_depth_labels(r.out.ptr, 3, labels.ptr, stride_bytes=r.out_stride)
        assert [bytes(x) for x in det.fetch_list(3)] == want, "any depth-input entry takes the buffer"
        raw = r.out.download(r.out.nbytes)
        got = np.array([raw[g * r.out_stride:g * r.out_stride + 2 * r.points].view(np.uint16).reshape(d["h"], d["w"]) for g in range(3)])
        assert (got == d["fused_filtered"][:3]).all()
    finally:
        labels.free()
        mid.free()
        r.close()


@pytest.mark.gpu
def test_the_host_path_over_four_slices_equals_the_composition(ssd, gpu_device, stairs):
    d = stairs
    r = _stairs_filter(ssd, gpu_device, d, d["frames"][:2], 0, 8)     # slices of 8 frames: 27 frames are 8 + 8 + 8 + 3
    try:
        det = r.det
        frames = d["frames"]
        host = [ssd.depth_edges_host(f) for f in frames]
        want = [bytes(x) for x in det.process_depth_host(d["filtered"])]
        res, filtered, stats = det.process_depth_host_edges(frames, filtered=True, stats=True)
        assert [bytes(x) for x in res] == want
        assert filtered.shape == d["filtered"].shape and (filtered == d["filtered"]).all()
        assert [bytes(s) for s in stats] == [bytes(s) for _, s in host]
        assert [bytes(x) for x in det.process_depth_host_edges(frames)] == want, "without the frames and the records"
        other = ssd.EdgeRule(*OTHER)
        res = det.process_depth_host_edges(frames[:11], rule=other)
        want_o = np.array([ssd.depth_edges_host(f, other)[0] for f in frames[:11]])
        assert [bytes(x) for x in res] == [bytes(x) for x in det.process_depth_host(want_o)]
        with pytest.raises(ssd.SsdError):
            det.process_depth_host_edges(frames[:3], rule=ssd.EdgeRule(9, 1, 40, 0))
    finally:
        r.close()


@pytest.mark.gpu
def test_two_calls_on_two_streams_with_no_host_wait(ssd, gpu_device, two_streams):  # noqa: F811
    """the order guard of test_gpu_follow_passes.py: it guards the order of the two calls, it cannot prove it"""
    a, b = two_streams
    frames = [em.stress_frame(ssd, 64, 48, seed=1000 + s) for s in range(8)]
    r = Filter(ssd, gpu_device, frames)
    try:
        args = dict(stride_bytes=r.stride, out_stride_bytes=r.out_stride)
        second = ssd.EdgeRule(0, 1, 5, 0)
        r.det.enqueue_depth_edges(r.src.ptr, 8, r.out.ptr, stream=a, **args)
        r.det.enqueue_depth_edges(r.src.ptr, 8, r.out.ptr, rule=second, stream=b, **args)        # no host wait between them
        stats = r.det.fetch_depth_edges(8)
        want_o, _, want_st = _want(ssd, frames, second)
        first_o, _, _ = _want(ssd, frames, None)
        raw = r.out.download(r.out.nbytes)
        got = np.array([raw[g * r.out_stride:g * r.out_stride + 2 * r.points].view(np.uint16).reshape(48, 64) for g in range(8)])
        assert (got == want_o).all() and not (got == first_o).all(), "the buffer holds the second call's frames"
        assert [bytes(s) for s in stats] == want_st
    finally:
        r.close()


@pytest.mark.gpu
def test_refusals_workspace_detection_and_time(ssd, gpu_device, stairs):
    L = ssd.lib()
    d = stairs
    r = _stairs_filter(ssd, gpu_device, d, d["frames"][:7], 0, 6)     # (a frame more than a batch: every refused call's ranges lie inside the buffers)
    plain = ssd.Detector(r.cfg, d["cal"], gpu_device)
    plain.set_intrinsics(d["intr"])
    try:
        det = r.det
        assert det.workspace_bytes == plain.workspace_bytes, "a handle that never filtered holds nothing for it"
        det.enqueue_depth(r.src.ptr, 6, stride_bytes=r.stride)
        before_results = [bytes(x) for x in det.fetch_list(6)]
        before = det.workspace_bytes
        fb = 2 * r.points

        def call(h=det._h, ptr=r.src.ptr, stride=r.stride, nframes=6, rule=None, out=r.out.ptr, out_stride=r.out_stride, cls=0, cls_stride=0):
            return L.ssd_enqueue_depth_edges(h, C.c_void_p(ptr), stride, nframes, None, None if rule is None else C.byref(rule), C.c_void_p(out),
                                             out_stride, C.c_void_p(cls), cls_stride)
        R = ssd.EdgeRule
        refused = [call(h=None), call(ptr=0), call(out=0), call(nframes=0), call(nframes=-1), call(nframes=7),
                   call(rule=R(-1, 1, 40, 0)), call(rule=R(9, 1, 40, 0)), call(rule=R(2, 1, -1, 0)), call(rule=R(2, 1, 65536, 0)),
                   call(rule=R(2, 1, 40, -1)), call(rule=R(2, 1, 40, 4097)), call(ptr=r.src.ptr + 1), call(stride=r.stride + 1), call(stride=fb - 2),
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
            det.fetch_depth_edges(1)                                  # ... and launched nothing: there is no pass to wait for
        assert L.ssd_get_depth_edges_time(det._h, C.byref(C.c_float())) == -1
        assert call() == 0
        after = det.workspace_bytes
        assert after - before == 2 * 6 * C.sizeof(ssd.EdgeStats), "exactly the records, on the device and pinned"
        want = _want(ssd, r.frames, None)[2]
        assert [bytes(s) for s in det.fetch_depth_edges(6)] == want[:6]
        assert det.depth_edges_time() == 0.0, "timing was off for it"
        assert [bytes(x) for x in det.fetch_list(6)] == before_results, "the detection's results are untouched by an interleaved filter call"
        det.set_timing(True)
        assert call(nframes=2, cls=r.cls.ptr, cls_stride=r.cls_stride) == 0 and det.workspace_bytes == after, "made once"
        assert [bytes(s) for s in det.fetch_depth_edges(1)] == want[:1]
        assert 0.0 < det.depth_edges_time() < 1000.0
        with pytest.raises(ssd.SsdError):
            det.fetch_depth_edges(3)
        assert [bytes(x) for x in det.fetch_list(6)] == before_results
        assert plain.workspace_bytes == before
    finally:
        plain.close()
        r.close()
