"""The trimmed surface refit on the GPU (k_surface_refit; include/ssd_hip.h): the device's records against
ssd_surface_refit_moments_host over the labels the same handle returns for the same frames, bit for bit - on the gate's edge too -,
and the entry points' contract."""
import ctypes as C

import numpy as np
import pytest

import refit_model as rm
import scenes
import surface_model as sm
from test_gpu_surface_fit import _records, _scenes, _upload

CASES = [("256x192", False), ("256x192", True), ("250x190", False)]       # depth input wants W % 4 == 0
POISON = 0xA5


class Batch:
    """A shape's frames resident on the device behind one detector: labels, first-pass records and refit passes, all by the handle"""

    def __init__(self, ssd, device, shape, depth, lanes=1, frames=None, scs=None):
        self.ssd, self.depth = ssd, depth
        if scs is None:
            self.W, self.H, scs = _scenes(ssd, shape)
        else:
            self.W, self.H = scs[0].width, scs[0].height
        self.n, self.wh = len(scs), self.W * self.H
        self.trans = ssd.transformation_for_scene(scs[0])
        self.cfg = ssd.default_config(self.W, self.H, max_frames_per_batch=self.n, batches_in_flight=lanes)
        self.intr = ssd.intrinsics_for_scene(scs[0]) if depth else None
        self.frames = frames if frames is not None else (list(ssd.synth_depth_host(scs)) if depth else list(ssd.synth_host(scs)))
        self.rec = C.sizeof(ssd.FrameMoments)
        self.det = ssd.Detector(self.cfg, self.trans, device)
        self.bufs = []
        if depth:
            self.det.set_intrinsics(self.intr)
        buf, self.ptr, self.stride = _upload(ssd, self.frames, depth, 8 if depth else 4, device)
        self.bufs.append(buf)
        self.lab_buf = ssd.DeviceBuffer(self.wh * self.n, device)
        self.first_buf = ssd.DeviceBuffer(self.rec * self.n, device)
        self.out = ssd.DeviceBuffer(self.rec * self.n, device)
        self.bufs += [self.lab_buf, self.first_buf, self.out]

    def close(self):
        for b in self.bufs:
            b.free()
        self.det.close()

    def detect(self):
        """labels by one enqueue, then the first-pass records by the next (the one a refit is held to): (results, labels, records)"""
        d = self.det
        (d.enqueue_depth_labels if self.depth else d.enqueue_labels)(self.ptr, self.n, self.lab_buf.ptr, stride_bytes=self.stride)
        d.fetch_list(self.n)
        self.lab = self.lab_buf.download(self.wh * self.n).reshape(self.n, self.wh).copy()
        d.enqueue_surface_moments(self.ptr, self.n, self.first_buf.ptr, depth=self.depth, stride_bytes=self.stride)
        self.res = d.fetch_list(self.n)
        self.first = _records(self.ssd, self.first_buf.download(self.rec * self.n), self.n)
        return self.res, self.lab, self.first

    def refit(self, gates):
        self.out.upload(np.full(self.rec * self.n, POISON, dtype=np.uint8))          # the call zeroes the records itself
        self.det.enqueue_surface_refit(self.ptr, self.n, gates, self.out.ptr, depth=self.depth, stride_bytes=self.stride)
        self.det.fetch_surface_refit()
        return _records(self.ssd, self.out.download(self.rec * self.n), self.n)

    def host(self, gates, frames=None):
        return [self.ssd.surface_refit_moments_host(self.cfg, f, l, g, m.n_surfaces, m.ground, intr=self.intr)
                for f, l, g, m in zip(frames or self.frames, self.lab, gates, self.first)]

    def gates(self, moments, k_sigma=2.5):
        return [self.ssd.surface_gates_from_moments(m, sm.MIN_POINTS, k_sigma, 0.0) for m in moments]


def _same(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert sm.frame_tuple(g) == sm.frame_tuple(w), i
        assert bytes(g) == bytes(w), i


@pytest.mark.gpu
@pytest.mark.parametrize("shape,depth", CASES)
def test_device_refit_equals_the_host_walk_over_the_handles_labels(ssd, gpu_device, shape, depth):
    """two passes with one workspace, each against the host function and gated by the pass before; then the same with three workspaces"""
    b = Batch(ssd, gpu_device, shape, depth)
    try:
        res, lab, first = b.detect()
        assert max(r.n_steps for r in res) >= 3 and res[-1].n_steps == 0 and bytes(first[-1]) == bytes(b.rec), "staircases and a bare floor"
        cells = lab[:, :b.wh // 64 * 64].reshape(b.n, -1, 64)
        top, low = cells.max(axis=2), np.where(cells > 0, cells, 255).min(axis=2)
        assert ((top > 0) & (low < top)).sum() > 0, "a 64-point cell that carries two surfaces"
        passes, cur = [], first
        for p in range(2):
            gates = b.gates(cur)
            got = b.refit(gates)
            _same(got, b.host(gates))
            passes.append((gates, got))
            cur = got
        got = passes[0][1]
        kept = [int(got[i].s[k].m.n + got[i].s[k].n_far) for i in range(b.n) for k in range(first[i].n_surfaces)]
        full = [int(first[i].s[k].m.n + first[i].s[k].n_far) for i in range(b.n) for k in range(first[i].n_surfaces)]
        assert all(0 < a <= f for a, f in zip(kept, full)) and sum(kept) < sum(full), "the gates trim something"
        assert bytes(got[-1]) == bytes(b.rec), "the no-stairs frame's record is all zero"
        assert [bytes(r) for r in b.det.fetch_list(b.n)] == [bytes(r) for r in res], "the results are still the enqueue's"
    finally:
        b.close()
    b3 = Batch(ssd, gpu_device, shape, depth, lanes=ssd.BATCHES_IN_FLIGHT_THROUGHPUT, frames=b.frames)
    try:
        res3, lab3, first3 = b3.detect()
        assert np.array_equal(lab3, lab) and [bytes(m) for m in first3] == [bytes(m) for m in first]
        for gates, want in passes:
            _same(b3.refit(gates), want)
    finally:
        b3.close()


@pytest.mark.gpu
def test_points_on_the_gates_edge_agree_with_the_host(ssd, gpu_device):
    """the cloud of the host gate-edge test, placed on a detected tread: labelled points moved in camera z onto dist +- gate and one
    float ulp beyond (n = (0, 0, 1), dist and gate dyadic), the frame detected again, and the device held to the host there"""
    W, H, scs = _scenes(ssd, "256x192")
    frames = [f.copy() for f in ssd.synth_host(scs)]
    b0 = Batch(ssd, gpu_device, "256x192", False, frames=frames)
    try:
        res, lab, first = b0.detect()
    finally:
        b0.close()
    k = 1 if first[0].ground else 0                                # a tread of frame 0
    assert first[0].n_surfaces > k
    pts = frames[0].reshape(-1, 3)
    mine = np.flatnonzero(lab[0] == k + 1)
    z = pts[mine, 2].astype(np.float64)
    gate = 2.0 ** -6
    dist = round(float(np.median(z)) * 1024) / 1024
    assert z.min() < dist - gate and z.max() > dist + gate, "the tread reaches beyond the gate on both sides"
    targets = [(dist + gate, True), (float(rm.up(dist + gate)), False), (dist - gate, True), (float(rm.down(dist - gate)), False)]
    moved = {}
    for t, (zt, keep) in enumerate(targets):
        near = mine[np.argsort(np.abs(z - zt))]
        near = [i for i in near if i not in moved][:6]             # six points each: some keep their label after the move
        for i in near:
            pts[i, 2] = np.float32(zt)
            moved[i] = keep
    b = Batch(ssd, gpu_device, "256x192", False, frames=frames)
    try:
        res, lab, first = b.detect()
        still = [i for i in moved if lab[0][i] == k + 1]
        zs = pts[still, 2].astype(np.float64)
        assert (np.abs(zs - dist) == gate).sum() >= 2 and (np.abs(zs - dist) > gate).sum() >= 2, "points on the edge and beyond it are labelled"
        gates = b.gates(first)
        g = gates[0].g[k]
        g.n[:] = [0.0, 0.0, 1.0]
        g.dist, g.gate = dist, gate
        got = b.refit(gates)
        _same(got, b.host(gates))
        inside = (lab[0] == k + 1) & (np.abs(pts[:, 2].astype(np.float64) - dist) <= gate)
        assert int(got[0].s[k].m.n + got[0].s[k].n_far) == int(inside.sum())
        assert sm.frame_tuple(got[0])[2][k] == sm.moments_np(pts[inside], np.ones(int(inside.sum())), 1)[0]
    finally:
        b.close()


@pytest.mark.gpu
def test_the_device_sums_the_products_in_the_stated_order(ssd, gpu_device):
    """the order-sensitive points of the host test (tests/refit_model.order_sensitive_points) on a detected tread's own pixels: under
    (a + b) + c their residual EQUALS the gate, under a + (b + c) it lies beyond it - a kernel that summed in the other order, or
    contracted a product into an FMA, would trim them"""
    W, H, scs = _scenes(ssd, "256x192")
    frames = [f.copy() for f in ssd.synth_host(scs)]
    b0 = Batch(ssd, gpu_device, "256x192", False, frames=frames)
    try:
        res, lab, first = b0.detect()
    finally:
        b0.close()
    k = first[0].n_surfaces - 1                                    # the top tread of frame 0
    assert k >= 1
    pts = frames[0].reshape(-1, 3)
    plane, on, beyond = rm.order_sensitive_points(pts, lab[0], k)
    b = Batch(ssd, gpu_device, "256x192", False, frames=frames)
    try:
        res, lab, first = b.detect()
        on = [i for i in on if lab[0][i] == k + 1]
        beyond = [i for i in beyond if lab[0][i] == k + 1]
        assert len(on) >= 2 and len(beyond) >= 1, "moved points still carry the tread's label"
        gates = b.gates(first)
        g = gates[0].g[k]
        g.n[:] = plane[0]
        g.dist, g.gate = plane[1], plane[2]
        got = b.refit(gates)
        _same(got, b.host(gates))
        keep = rm.keeps(pts, lab[0], gates[0])
        assert all(keep[i] for i in on) and not any(keep[i] for i in beyond)
        p = pts.astype(np.float64)
        other = np.abs(plane[0][0] * p[:, 0] + (plane[0][1] * p[:, 1] + plane[0][2] * p[:, 2])) <= plane[2]
        mine = lab[0] == k + 1
        assert int((mine & keep).sum()) - int((mine & other).sum()) == len(on), "the other order loses exactly the points on the edge"
        assert int(got[0].s[k].m.n + got[0].s[k].n_far) == int((mine & keep).sum())
        assert sm.frame_tuple(got[0])[2][k] == rm.refit_np(pts, lab[0], gates[0], first[0].n_surfaces)[k]
    finally:
        b.close()


@pytest.mark.gpu
def test_refits_behind_batches_of_different_workspaces_do_not_share_their_gates(ssd, gpu_device):
    """three workspaces, no fetch between: enqueue A, refit A, enqueue B, refit B (B's frames in another order, other gates), and
    again - the device gates are one set, so each pass goes behind the one before; every record is its own batch's under its own gates"""
    W, H, scs = _scenes(ssd, "256x192")
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    xyz = ssd.synth_host(scs)
    order = [list(range(n)), list(range(n))[::-1], list(range(n))]
    fb, rec = W * H * 12, C.sizeof(ssd.FrameMoments)
    det = ssd.Detector(cfg, trans, gpu_device)
    bufs = [ssd.DeviceBuffer(fb * n, gpu_device) for _ in order]
    firsts = [ssd.DeviceBuffer(rec * n, gpu_device) for _ in order]
    outs = [ssd.DeviceBuffer(rec * n, gpu_device) for _ in order]
    try:
        for buf, o in zip(bufs, order):
            buf.upload(np.ascontiguousarray(xyz[o]))
        # the first-pass records and each batch's gates (2.5, 2.0 and 3.0 rms), one batch at a time
        want, gates = [], []
        for j, (buf, fbuf) in enumerate(zip(bufs, firsts)):
            det.enqueue_surface_moments(buf.ptr, n, fbuf.ptr)
            det.fetch_list(n)
            first = _records(ssd, fbuf.download(rec * n), n)
            gates.append([ssd.surface_gates_from_moments(m, sm.MIN_POINTS, (2.5, 2.0, 3.0)[j], 0.0) for m in first])
            det.enqueue_surface_refit(buf.ptr, n, gates[j], outs[j].ptr)
            det.fetch_surface_refit()
            want.append(outs[j].download(rec * n).tobytes())
        assert len(set(want)) == 3, "the batches' gates differ, and so do their records"
        for out in outs:
            out.upload(np.full(rec * n, POISON, dtype=np.uint8))
        for buf, fbuf, g, out in zip(bufs, firsts, gates, outs):
            det.enqueue_surface_moments(buf.ptr, n, fbuf.ptr)
            det.enqueue_surface_refit(buf.ptr, n, g, out.ptr)
        det.fetch_surface_refit()                                  # the last pass, and with it every one before
        assert [out.download(rec * n).tobytes() for out in outs] == want
    finally:
        for x in bufs + firsts + outs:
            x.free()
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True])
def test_a_huge_gate_gives_the_first_pass_and_a_zero_gate_nothing(ssd, gpu_device, depth):
    b = Batch(ssd, gpu_device, "256x192", depth)
    try:
        res, lab, first = b.detect()
        gates = b.gates(first)
        for g, m in zip(gates, first):
            for k in range(m.n_surfaces):
                g.g[k].gate = 1e9
        got = b.refit(gates)
        assert [bytes(g) for g in got] == [bytes(m) for m in first], "a gate of 1e9: the device's own first-pass records"
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            for g in gates:
                for k in range(ssd.MAX_STEPS):
                    g.g[k].gate = bad
            got = b.refit(gates)
            for g, m in zip(got, first):
                assert (g.n_surfaces, g.ground) == (m.n_surfaces, m.ground), "the header is kept"
                assert bytes(g)[8:] == bytes(b.rec - 8), bad
        # gates that name fewer surfaces than the frame has: those beyond gather nothing
        gates = b.gates(first)
        for g in gates:
            g.n_surfaces = min(g.n_surfaces, 1)
        got = b.refit(gates)
        _same(got, b.host(gates))
        assert got[0].s[0].m.n > 0 and bytes(got[0].s[1]) == bytes(C.sizeof(ssd.SurfaceMoments))
    finally:
        b.close()


@pytest.mark.gpu
def test_dead_frames_come_out_all_zero(ssd, gpu_device):
    """a frame the reference would have thrown on, a frame without stairs, and a staircase between them"""
    scs = [scenes.make(ssd, "vga_yaw50_throws"), scenes.make(ssd, "vga_3steps_noise2mm"), scenes.make(ssd, "vga_empty")]
    b = Batch(ssd, gpu_device, None, False, scs=scs)
    try:
        res, lab, first = b.detect()
        assert res[0].status & ssd.ST_THROW and res[2].n_steps == 0 and res[1].n_steps >= 3 and not (res[1].status & ssd.ST_THROW)
        gates = []
        for _ in range(b.n):
            g = ssd.FrameGates()
            g.n_surfaces = ssd.MAX_STEPS
            for k in range(ssd.MAX_STEPS):
                g.g[k].n[:] = [0.0, 0.0, 1.0]
                g.g[k].dist, g.g[k].gate = 1.0, 1e9
            gates.append(g)
        got = b.refit(gates)
        assert bytes(got[0]) == bytes(b.rec) and bytes(got[2]) == bytes(b.rec)
        assert bytes(got[1]) == bytes(first[1]) and got[1].s[0].m.n > 0
    finally:
        b.close()


@pytest.mark.gpu
def test_a_refit_leaves_the_detection_state_untouched(ssd, gpu_device):
    """results, risers and debug records after a refit are the plain enqueue's; the gate buffers are counted from the first refit on"""
    W, H, scs = _scenes(ssd, "256x192")
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n)
    xyz = ssd.synth_host(scs)
    fb, rec = W * H * 12, C.sizeof(ssd.FrameMoments)
    det, plain = ssd.Detector(cfg, trans, gpu_device), ssd.Detector(cfg, trans, gpu_device)
    buf, out = ssd.DeviceBuffer(fb * n, gpu_device), ssd.DeviceBuffer(rec * n, gpu_device)
    try:
        buf.upload(np.ascontiguousarray(xyz))
        for d in (det, plain):
            d.set_risers(True)
            d.set_debug(True, images=False)
        assert det.workspace_bytes == plain.workspace_bytes
        plain.enqueue(buf.ptr, n)
        want = ([bytes(r) for r in plain.fetch_list(n)], [bytes(r) for r in plain.fetch_risers(n)], [bytes(plain.debug(i)) for i in range(n)])
        det.enqueue_surface_moments(buf.ptr, n, out.ptr)
        res = det.fetch_list(n)
        first = _records(ssd, out.download(rec * n), n)
        gates = [ssd.surface_gates_from_moments(m, sm.MIN_POINTS, 2.5, 0.0) for m in first]
        for _ in range(2):
            det.enqueue_surface_refit(buf.ptr, n, gates, out.ptr)
            det.fetch_surface_refit()
        got = _records(ssd, out.download(rec * n), n)
        assert 0 < got[0].s[0].m.n < first[0].s[0].m.n
        assert ([bytes(r) for r in det.fetch_list(n)], [bytes(r) for r in det.fetch_risers(n)], [bytes(det.debug(i)) for i in range(n)]) == want
        assert [bytes(r) for r in res] == want[0]
        assert det.workspace_bytes == plain.workspace_bytes + 2 * n * C.sizeof(ssd.FrameGates)
        assert det.surface_refit_time_ms() == 0.0, "timing was off"
        # a plain enqueue behind the refit is the plain enqueue still; timing on: the pass's time
        det.set_timing(True)
        det.enqueue(buf.ptr, n)
        assert [bytes(r) for r in det.fetch_list(n)] == want[0]
        det.enqueue_surface_refit(buf.ptr, n, gates, out.ptr)
        det.fetch_surface_refit()
        assert det.surface_refit_time_ms() > 0.0
        assert [bytes(g) for g in _records(ssd, out.download(rec * n), n)] == [bytes(g) for g in got]
    finally:
        buf.free()
        out.free()
        det.close()
        plain.close()


@pytest.mark.gpu
def test_the_refusals_of_the_refit_entry_point(ssd, gpu_device):
    """SSD_E_ARG before anything is launched or copied: the destination keeps its poison and the handle allocates nothing"""
    W, H, scs = _scenes(ssd, "256x192")
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n)
    xyz = ssd.synth_host(scs)
    depth = ssd.synth_depth_host(scs)
    fb, rec = W * H * 12, C.sizeof(ssd.FrameMoments)
    det = ssd.Detector(cfg, trans, gpu_device)
    buf, dbuf, out = ssd.DeviceBuffer(fb * n, gpu_device), ssd.DeviceBuffer(W * H * 2 * n, gpu_device), ssd.DeviceBuffer(rec * n, gpu_device)
    try:
        buf.upload(np.ascontiguousarray(xyz))
        dbuf.upload(np.ascontiguousarray(depth))
        out.upload(np.full(rec * n, POISON, dtype=np.uint8))
        bytes0 = det.workspace_bytes
        gates = [ssd.FrameGates() for _ in range(n)]
        arr = (ssd.FrameGates * n)(*gates)
        L = ssd.lib()

        def refused(match, ptr=buf.ptr, stride=fb, frames=n, depth_in=False, g=arr, o=out.ptr):
            rc = L.ssd_enqueue_surface_refit(det._h, C.c_void_p(ptr), stride, frames, None, 1 if depth_in else 0, g, C.c_void_p(o))
            assert rc == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        refused(b"no whole enqueue")                                  # nothing enqueued yet
        with pytest.raises(ssd.SsdError, match="no ssd_enqueue_surface_refit"):
            det.fetch_surface_refit()
        det.enqueue(buf.ptr, n, stages=ssd.STAGE_ALL & ~64)           # a partial run (everything but k_final)
        refused(b"no whole enqueue")
        det.enqueue(buf.ptr, n)
        det.fetch_list(n)
        refused(b"nframes", frames=n - 1)
        refused(b"null", g=None)
        refused(b"null", o=None)
        refused(b"null", ptr=None)
        refused(b"intrinsics", ptr=dbuf.ptr, stride=W * H * 2, depth_in=True)      # depth input without intrinsics
        refused(b"not the last enqueue's", ptr=buf.ptr + fb, frames=n)             # other frames
        refused(b"not the last enqueue's", stride=fb + 4)
        assert det.workspace_bytes == bytes0, "a refused call allocates nothing"
        det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
        refused(b"no whole enqueue")                                  # new intrinsics withdraw the enqueue a refit could follow
        det.enqueue(buf.ptr, n)
        det.fetch_list(n)
        refused(b"not the last enqueue's", ptr=dbuf.ptr, stride=W * H * 2, depth_in=True)   # the last enqueue read vertices
        det.set_cameras([trans])
        det.enqueue_cameras(buf.ptr, n, [0] * n)
        det.fetch_list(n)
        refused(b"cameras batch")
        assert bytes(out.download(rec * n)) == bytes([POISON]) * (rec * n), "a refused call writes nothing"
        # and accepted behind a whole enqueue again
        det.enqueue(buf.ptr, n)
        det.fetch_list(n)
        before = det.workspace_bytes
        det.enqueue_surface_refit(buf.ptr, n, gates, out.ptr)
        det.fetch_surface_refit()
        assert det.workspace_bytes == before + 2 * n * C.sizeof(ssd.FrameGates)
        got = _records(ssd, out.download(rec * n), n)
        assert got[0].n_surfaces >= 3 and bytes(got[0])[8:] == bytes(rec - 8), "all-zero gates gather nothing"
    finally:
        buf.free()
        dbuf.free()
        out.free()
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2])
def test_the_host_path_over_more_than_one_slice(ssd, gpu_device, passes):
    """40 frames through 32-frame slices: results = ssd_process_host's, first = the surface fit's records, refit = the chain of host
    functions over the handle's labels pass by pass, out = ssd_surface_fit_solve of the last pass"""
    W, H, base = _scenes(ssd, "256x192")
    kw = dict(roll_deg=25.0)
    scs = [ssd.make_scene(W, H, n_steps=3 if i % 5 else 0, seed=100 + i, sigma=0.001 + 0.0002 * (i % 4), **kw) for i in range(40)]
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=32)
    xyz = ssd.synth_host(scs)
    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        want_res = det.process_host(xyz)
        _, lab = det.process_host_labels(xyz)
        lab = lab.reshape(n, W * H)
        _, _, want_first = det.process_host_surfaces(xyz, min_points=sm.MIN_POINTS, moments=True)
        res, fits, first, refit = det.process_host_surfaces_refit(xyz, min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0, passes=passes, moments=True)
        assert [bytes(r) for r in res] == [bytes(r) for r in want_res]
        assert [bytes(m) for m in first] == [bytes(m) for m in want_first]
        assert sum(1 for m in first if m.n_surfaces >= 3) >= 20 and sum(1 for m in first if m.n_surfaces == 0) >= 8
        for i in range(n):
            chain = rm.refit_chain(ssd, cfg, xyz[i], lab[i], first[i], 2.5, passes=passes)
            assert bytes(refit[i]) == bytes(chain[-1]), i
            assert bytes(fits[i]) == bytes(ssd.surface_fit_solve(chain[-1], trans, sm.MIN_POINTS)), i
        res2, fits2 = det.process_host_surfaces_refit(xyz, min_points=sm.MIN_POINTS, passes=passes)        # without the moments
        assert [bytes(f) for f in fits2] == [bytes(f) for f in fits] and [bytes(r) for r in res2] == [bytes(r) for r in want_res]
        L = ssd.lib()
        r1, o1 = (ssd.FrameResult * n)(), (ssd.FrameSurfaces * n)()
        for bad in (0, 5):
            assert L.ssd_process_host_surfaces_refit(det._h, xyz.ctypes.data_as(C.c_void_p), n, 0, r1, None, None, 200, 2.5, 0.0, bad, o1) == -1
            assert b"passes" in L.ssd_last_error()
        assert L.ssd_process_host_surfaces_refit(det._h, xyz.ctypes.data_as(C.c_void_p), n, 0, r1, None, None, 200, 0.0, 0.0, 1, o1) == -1
        assert b"k_sigma" in L.ssd_last_error()
    finally:
        det.close()
