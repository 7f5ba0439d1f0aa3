"""The depth fusion on the GPU (ssd_enqueue_depth_fuse / ssd_fetch_depth_fuse / ssd_get_depth_fuse_time / ssd_process_depth_host_fused;
include/ssd_hip.h).  Every comparison is bytes against ssd_depth_fuse_host, which tests/test_depth_fuse.py holds to
the numpy restatement of the rule.  Small shapes - the kernel's paths depend on n (the network's size), the alignment (the wide and the
narrow body) and the tails, not on the size: 64 x 48 frames, the smallest frame whose pixel count divides neither load unit, and
256 x 192 where a detection has to see the staircase."""
import ctypes as C

import numpy as np
import pytest

import fuse_model as fm
from test_gpu_follow_passes import two_streams  # noqa: F401  (a fixture)

NS = (1, 2, 3, 5, 8, 13, 16)
W, H = 64, 48
FILL = 0xAB


@pytest.fixture(scope="module")
def scene33(ssd):
    """33 noisy frames of one still scene: 2 n + 1 frames for every n"""
    return fm.scene_frames(ssd, W, H, 33)


class Fuser:
    """a batch of depth frames resident on the device behind one detector, the output and the support buffer, all of them at pointers and
    strides that are multiples of 16 bytes (the wide body) or of 2 only (the narrow one); the strides are wider than a frame either way"""

    def __init__(self, ssd, device, frames, aligned=True, batch=None, cfg=None, cal=None):
        self.ssd, self.frames, self.total = ssd, frames, len(frames)
        h, w = frames[0].shape
        if cfg is None:
            cfg = ssd.default_config(w, h, max_frames_per_batch=batch or max(self.total, 2))
        self.cfg, self.points = cfg, w * h
        self.det = ssd.Detector(cfg, cal if cal is not None else ssd.GeometricTransformation().constants, device)
        fb = self.points * 2
        pad = 32 if aligned else 6
        self.lead = 0 if aligned else 2
        self.stride = (fb + 15) // 16 * 16 + pad
        self.out_stride = (fb + 15) // 16 * 16 + pad
        self.sup_stride = (self.points + 15) // 16 * 16 + (8 if aligned else 3)
        assert (self.stride % 16 == 0) == aligned
        self.src = ssd.DeviceBuffer(self.lead + self.stride * self.total, device)
        self.out = ssd.DeviceBuffer(self.lead + self.out_stride * self.total, device)
        self.sup = ssd.DeviceBuffer(self.lead + self.sup_stride * self.total, device)
        for i, f in enumerate(frames):
            self.src.upload(np.ascontiguousarray(f), offset=self.lead + i * self.stride)

    def fuse(self, nframes, n, hop, rule=None, support=True, stream=None):
        """-> (fused frames [groups, points], support [groups, points] or None, stats); everything outside the groups' pixels is untouched"""
        for buf in (self.out, self.sup):
            buf.upload(np.full(buf.nbytes, FILL, np.uint8))
        groups = self.det.enqueue_depth_fuse(self.src.ptr + self.lead, nframes, n, self.out.ptr + self.lead, hop, rule,
                                             self.sup.ptr + self.lead if support else None, self.stride, self.out_stride, self.sup_stride, stream)
        stats = self.det.fetch_depth_fuse(groups)
        raw, fused, sup = self.out.download(self.out.nbytes), [], []
        touched = np.zeros(self.out.nbytes, bool)
        for g in range(groups):
            at = self.lead + g * self.out_stride
            fused.append(raw[at:at + 2 * self.points].view(np.uint16).copy())
            touched[at:at + 2 * self.points] = True
        assert (raw[~touched] == FILL).all(), "a byte outside the fused frames was written"
        raws = self.sup.download(self.sup.nbytes)
        touched = np.zeros(self.sup.nbytes, bool)
        for g in range(groups if support else 0):
            at = self.lead + g * self.sup_stride
            sup.append(raws[at:at + self.points].copy())
            touched[at:at + self.points] = True
        assert (raws[~touched] == FILL).all(), "a byte outside the support maps was written"
        return np.array(fused), np.array(sup) if support else None, stats

    def close(self):
        for b in (self.src, self.out, self.sup):
            b.free()
        self.det.close()


def _want(ssd, frames, nframes, n, hop, rule):
    groups = (nframes - n) // hop + 1
    got = [ssd.depth_fuse_host(np.ascontiguousarray(frames[g * hop:g * hop + n]), rule, support=True) for g in range(groups)]
    return (np.array([o.reshape(-1) for o, _, _ in got]), np.array([s.reshape(-1) for _, _, s in got]), [bytes(st) for _, st, _ in got])


def _check(ssd, r, nframes, n, hop, rule=None, support=True):
    fused, sup, stats = r.fuse(nframes, n, hop, rule, support)
    want_f, want_s, want_st = _want(ssd, r.frames, nframes, n, hop, rule)
    assert fused.shape == want_f.shape and (fused == want_f).all(), "n %d hop %d: the fused frames" % (n, hop)
    if support:
        assert (sup == want_s).all(), "n %d hop %d: the support maps" % (n, hop)
    assert [bytes(s) for s in stats] == want_st, "n %d hop %d: the groups' records" % (n, hop)
    return stats


def _hops(n):
    return sorted({n, 1, (n + 1) // 2})


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["wide-16B", "narrow-2B"])
@pytest.mark.parametrize("n", NS)
def test_the_scene_frames_equal_the_host(ssd, gpu_device, scene33, n, aligned):
    r = Fuser(ssd, gpu_device, list(scene33[:2 * n + 1]), aligned)
    try:
        for hop in _hops(n):
            stats = _check(ssd, r, 2 * n + 1, n, hop, support=hop != 1)
            assert all(s.n_fused + s.n_empty + s.n_few + s.n_split == W * H for s in stats)
        assert stats[0].n_fused > 0.9 * W * H
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["wide-16B", "narrow-2B"])
@pytest.mark.parametrize("n", NS)
def test_the_edge_frames_equal_the_host(ssd, gpu_device, n, aligned):
    rules = [None, (1, 1, 0), (n, n, 40), (1, n, 65535)]
    for k, rule in enumerate(rules):
        a, _ = fm.edge_frame(n, rule or fm.default_rule(n), W, H, seed=k)
        b, _ = fm.edge_frame(n, rule or fm.default_rule(n), W, H, seed=k + 50)
        r = Fuser(ssd, gpu_device, list(np.concatenate([a, b, a[:1]])), aligned)
        try:
            for hop in _hops(n) if k == 0 else (n,):
                _check(ssd, r, 2 * n + 1, n, hop, fm.rule_of(ssd, rule), support=True)
            _check(ssd, r, n, n, n, fm.rule_of(ssd, rule), support=False)
        finally:
            r.close()


@pytest.mark.gpu
def test_a_frame_whose_pixel_count_divides_neither_unit(ssd, gpu_device):
    """the smallest shape ssd_create accepts whose pixel count is a multiple of neither 4 nor 8: both bodies' tails"""
    shape = None
    for w, h in ((3, 3), (5, 3), (3, 5), (5, 5), (7, 5), (9, 7), (13, 11), (31, 23)):
        assert (w * h) % 4 != 0 and w * h > 8
        try:
            ssd.Detector(ssd.default_config(w, h, max_frames_per_batch=2), ssd.GeometricTransformation().constants, gpu_device).close()
        except ssd.SsdError:
            continue
        shape = (w, h)
        break
    assert shape is not None, "ssd_create accepts no shape whose pixel count is a multiple of neither 4 nor 8 among the candidates"
    w, h = shape
    for n in NS:
        rule = fm.default_rule(n)
        a, _ = fm.edge_frame(n, rule, w, h, seed=3)                  # (as many of the edge cases as the frame has pixels for: random ones)
        b, _ = fm.edge_frame(n, rule, w, h, seed=4)
        for aligned in (True, False):
            r = Fuser(ssd, gpu_device, list(np.concatenate([a, b])), aligned)
            try:
                _check(ssd, r, 2 * n, n, n)
                _check(ssd, r, 2 * n, n, 1, support=False)
            finally:
                r.close()


@pytest.mark.gpu
def test_a_batch_at_max_frames_per_batch_and_one_beyond(ssd, gpu_device, scene33):
    r = Fuser(ssd, gpu_device, list(scene33[:9]), batch=8)
    try:
        before = r.det.workspace_bytes
        with pytest.raises(ssd.SsdError):
            r.det.enqueue_depth_fuse(r.src.ptr, 9, 2, r.out.ptr, 2, None, None, r.stride, r.out_stride)
        assert r.det.workspace_bytes == before
        with pytest.raises(ssd.SsdError):
            r.det.fetch_depth_fuse(1)                                 # nothing was launched: there is no pass to wait for
        _check(ssd, r, 8, 2, 2)
        _check(ssd, r, 8, 2, 1)                                       # 7 groups
        _check(ssd, r, 8, 8, 8)
    finally:
        r.close()


@pytest.fixture(scope="module")
def stairs(ssd):
    """27 frames of the still 256 x 192 scene, what detects them, and the host's fusion of every three"""
    w, h = 256, 192
    sc = ssd.make_scene(w, h, n_steps=3, seed=1000, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02)
    frames = fm.scene_frames(ssd, w, h, 27)
    fused = np.array([ssd.depth_fuse_host(np.ascontiguousarray(frames[3 * g:3 * g + 3]))[0] for g in range(9)])
    return dict(w=w, h=h, cal=ssd.transformation_for_scene(sc).constants, intr=ssd.intrinsics_for_scene(sc), frames=frames, fused=fused)


def _stairs_fuser(ssd, device, d, frames, in_flight, batch):
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=batch, batches_in_flight=in_flight)
    r = Fuser(ssd, device, list(frames), True, cfg=cfg, cal=d["cal"])
    r.det.set_intrinsics(d["intr"])
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [0, 3])
def test_the_chain_fuse_then_detect_with_no_host_wait(ssd, gpu_device, stairs, in_flight):
    d = stairs
    r = _stairs_fuser(ssd, gpu_device, d, d["frames"][:9], in_flight, 9)
    labels = ssd.DeviceBuffer(3 * d["w"] * d["h"], gpu_device)
    try:
        det = r.det
        want = [bytes(x) for x in det.process_depth_host(d["fused"][:3])]
        assert any(ssd.FrameResult.from_buffer_copy(x).n_steps >= 3 for x in want), "the fused frames show the staircase"
        for _ in range(2):                                            # the second round takes another workspace where there are several
            groups = det.enqueue_depth_fuse(r.src.ptr, 9, 3, r.out.ptr, stride_bytes=r.stride, out_stride_bytes=r.out_stride)
            det.enqueue_depth(r.out.ptr, groups, stride_bytes=r.out_stride)       # the same (null) stream, no host wait
            assert [bytes(x) for x in det.fetch_list(3)] == want
        det.enqueue_depth_fuse(r.src.ptr, 9, 3, r.out.ptr, stride_bytes=r.stride, out_stride_bytes=r.out_stride)
        det.enqueue_depth_labels(r.out.ptr, 3, labels.ptr, stride_bytes=r.out_stride)
        assert [bytes(x) for x in det.fetch_list(3)] == want, "any depth-input entry takes the buffer"
    finally:
        labels.free()
        r.close()


@pytest.mark.gpu
def test_the_host_path_over_33_groups_equals_the_composition(ssd, gpu_device, stairs):
    d = stairs
    frames = np.concatenate([d["frames"]] * 4)[:99]                   # 33 groups of 3: more than one slice of 30 frames
    r = _stairs_fuser(ssd, gpu_device, d, d["frames"][:3], 0, 64)
    try:
        det = r.det
        host = [ssd.depth_fuse_host(np.ascontiguousarray(frames[3 * g:3 * g + 3])) for g in range(33)]
        want_f = np.array([o for o, _ in host])
        want = [bytes(x) for x in det.process_depth_host(want_f)]
        res, fused, stats = det.process_depth_host_fused(frames, 3, fused=True, stats=True)
        assert [bytes(x) for x in res] == want
        assert fused.shape == want_f.shape and (fused == want_f).all()
        assert [bytes(s) for s in stats] == [bytes(s) for _, s in host]
        assert [bytes(x) for x in det.process_depth_host_fused(frames, 3)] == want, "without the frames and the records"
        tight = ssd.FuseRule(3, 3, 20, 0)
        res = det.process_depth_host_fused(frames[:12], 3, rule=tight)
        want_t = np.array([ssd.depth_fuse_host(np.ascontiguousarray(frames[3 * g:3 * g + 3]), tight)[0] for g in range(4)])
        assert [bytes(x) for x in res] == [bytes(x) for x in det.process_depth_host(want_t)]
        with pytest.raises(ssd.SsdError):
            det.process_depth_host_fused(frames[:98], 3)
        with pytest.raises(ssd.SsdError):
            det.process_depth_host_fused(frames[:34], 17)
    finally:
        r.close()


@pytest.mark.gpu
def test_two_calls_on_two_streams_with_no_host_wait(ssd, gpu_device, scene33, two_streams):  # noqa: F811
    """the order guard of test_gpu_follow_passes.py: it guards the order of the two calls, it cannot prove it"""
    a, b = two_streams
    r = Fuser(ssd, gpu_device, list(scene33[:16]))
    try:
        args = dict(stride_bytes=r.stride, out_stride_bytes=r.out_stride)
        r.det.enqueue_depth_fuse(r.src.ptr, 16, 8, r.out.ptr, stream=a, **args)
        r.det.enqueue_depth_fuse(r.src.ptr, 16, 2, r.out.ptr, rule=ssd.FuseRule(1, 1, 5, 0), stream=b, **args)    # no host wait between them
        stats = r.det.fetch_depth_fuse(8)
        want_f, _, want_st = _want(ssd, r.frames, 16, 2, 2, ssd.FuseRule(1, 1, 5, 0))
        first_f, _, _ = _want(ssd, r.frames, 16, 8, 8, None)
        raw = r.out.download(r.out.nbytes)
        got = np.array([raw[g * r.out_stride:g * r.out_stride + 2 * r.points].view(np.uint16) for g in range(8)])
        assert (got == want_f).all() and not (got[:2] == first_f).all(), "the buffer holds the second call's frames"
        assert [bytes(s) for s in stats] == want_st
    finally:
        r.close()


@pytest.mark.gpu
def test_refusals_workspace_detection_and_time(ssd, gpu_device, stairs):
    L = ssd.lib()
    d = stairs
    r = _stairs_fuser(ssd, gpu_device, d, d["frames"][:7], 0, 6)      # (a frame more than a batch: every refused call's ranges lie inside the buffers)
    plain = ssd.Detector(r.cfg, d["cal"], gpu_device)
    plain.set_intrinsics(d["intr"])
    try:
        det = r.det
        assert det.workspace_bytes == plain.workspace_bytes, "a handle that never fused holds nothing for it"
        det.enqueue_depth(r.src.ptr, 6, stride_bytes=r.stride)
        before_results = [bytes(x) for x in det.fetch_list(6)]
        before = det.workspace_bytes
        fb = 2 * r.points

        def call(h=det._h, ptr=r.src.ptr, stride=r.stride, nframes=6, n=3, hop=3, rule=None, out=r.out.ptr, out_stride=r.out_stride, sup=0, sup_stride=0):
            return L.ssd_enqueue_depth_fuse(h, C.c_void_p(ptr), stride, nframes, None, n, hop, None if rule is None else C.byref(rule), C.c_void_p(out),
                                            out_stride, C.c_void_p(sup), sup_stride)
        R = ssd.FuseRule
        refused = [call(h=None), call(ptr=0), call(out=0), call(n=0), call(n=17), call(hop=0), call(hop=4), call(nframes=2), call(nframes=7),
                   call(rule=R(0, 1, 40, 0)), call(rule=R(4, 1, 40, 0)), call(rule=R(1, 0, 40, 0)), call(rule=R(1, 4, 40, 0)),
                   call(rule=R(1, 1, -1, 0)), call(rule=R(1, 1, 65536, 0)), call(ptr=r.src.ptr + 1), call(stride=r.stride + 1), call(stride=fb - 2),
                   call(out=r.out.ptr + 1), call(out_stride=fb - 2), call(out_stride=fb + 1), call(sup=r.sup.ptr, sup_stride=r.points - 1),
                   call(out=r.src.ptr + 4 * r.stride), call(ptr=r.src.ptr + 2 * r.stride, nframes=3, out=r.src.ptr + 2 * r.stride - fb + 2),
                   call(ptr=r.src.ptr + 2 * r.stride, nframes=3, sup=r.src.ptr + 2 * r.stride - r.points + 1, sup_stride=r.sup_stride)]
        assert refused == [-1] * len(refused)
        assert det.workspace_bytes == before, "a refused call allocates nothing"
        with pytest.raises(ssd.SsdError):
            det.fetch_depth_fuse(1)                                   # ... and launched nothing: there is no pass to wait for
        assert L.ssd_get_depth_fuse_time(det._h, C.byref(C.c_float())) == -1
        assert call() == 0
        after = det.workspace_bytes
        assert after - before == 2 * 6 * C.sizeof(ssd.FuseStats), "exactly the records, on the device and pinned"
        want = _want(ssd, r.frames, 6, 3, 3, None)[2]
        assert [bytes(s) for s in det.fetch_depth_fuse(2)] == want
        assert det.depth_fuse_time_ms() == 0.0, "timing was off for it"
        assert [bytes(x) for x in det.fetch_list(6)] == before_results, "the detection's results are untouched by an interleaved fuse"
        det.set_timing(True)
        assert call(sup=r.sup.ptr, sup_stride=r.sup_stride) == 0 and det.workspace_bytes == after, "made once"
        assert [bytes(s) for s in det.fetch_depth_fuse(1)] == want[:1]
        assert 0.0 < det.depth_fuse_time_ms() < 1000.0
        with pytest.raises(ssd.SsdError):
            det.fetch_depth_fuse(3)
        assert [bytes(x) for x in det.fetch_list(6)] == before_results
    finally:
        plain.close()
        r.close()
