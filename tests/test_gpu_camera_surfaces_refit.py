"""The trimmed surface refit of cameras batches on the GPU (k_surface_refit_cams; include/ssd_hip.h).  The contract
under test is section 7b's, extended to section 7g's pass: frame i's refit record is, byte for byte, what a handle created with that
frame's camera gives from ssd_enqueue_surface_refit for the frame alone under gates[i] - and ssd_surface_refit_moments_host over the
labels the same batch returns.  The handle's own calibration is the identity, so a fall-back to it would be wrong everywhere; the
gates go by frame, the cameras by the index the enqueue left."""
import ctypes as C

import numpy as np
import pytest

import refit_model as rm
import scenes
import surface_model as sm
import test_gpu_camera_surfaces as cs
from test_gpu_surface_refit import POISON, _same

ORDER = cs.ORDER
ORDER_B = [1, 3, 0, 2, 1, 3]
F = cs.F
ALONE = {}


def _cameras(ssd, shape, **scene_kw):
    """the four mountings of the cameras surface test at a shape: (W, H, depth, frames per camera, table, intrinsics per camera)"""
    W, H, depth = cs.SHAPES[shape]
    scs = [ssd.make_scene(W, H, n_steps=3, seed=11 + j, sigma=0.001 + 0.0005 * j, **cs.POSES[j], **(cs.OPTICS[j] if depth else {}), **scene_kw) for j in range(4)]
    trans = [ssd.transformation_for_scene(sc) for sc in scs]
    intr = [ssd.intrinsics_for_scene(sc, depth_units=u) for sc, u in zip(scs, cs.UNITS)] if depth else [None] * 4
    frames = [ssd.synth_depth_host([sc], depth_units=u)[0] for sc, u in zip(scs, cs.UNITS)] if depth else list(ssd.synth_host(scs))
    table = [(t, i) for t, i in zip(trans, intr)] if depth else trans
    return W, H, depth, frames, table, intr


def _alone(ssd, cfg, cam, frame, depth, chain, device):
    """the frame through a one-camera handle alone: a whole enqueue, then one ssd_enqueue_surface_refit per FrameGates of `chain`
    -> [bytes of each pass's record]; remembered per (camera, frame, gates), as several tests ask for the same"""
    trans, intr = cam if isinstance(cam, tuple) else (cam, None)
    key = (bytes(cfg), bytes(trans.constants), bytes(intr) if intr is not None else b"", np.ascontiguousarray(frame).tobytes(), tuple(bytes(g) for g in chain))
    if key in ALONE:
        return ALONE[key]
    rec = C.sizeof(ssd.FrameMoments)
    det = ssd.Detector(cfg, trans, device)
    buf, out = ssd.DeviceBuffer(frame.nbytes, device), ssd.DeviceBuffer(rec, device)
    try:
        if depth:
            det.set_intrinsics(intr)
        buf.upload(np.ascontiguousarray(frame))
        det.enqueue_surface_moments(buf.ptr, 1, out.ptr, depth=depth)
        det.fetch_list(1)
        got = []
        for g in chain:
            det.enqueue_surface_refit(buf.ptr, 1, [g], out.ptr, depth=depth)
            det.fetch_surface_refit()
            got.append(out.download(rec).tobytes())
    finally:
        buf.free()
        out.free()
        det.close()
    ALONE[key] = got
    return got


class CamBatch:
    """frames resident behind an identity-calibrated detector with a camera table: labels, first-pass records and refit passes"""

    def __init__(self, ssd, device, W, H, depth, frames, table, order, lanes=1, pad=None, max_frames=F, spare=True):
        self.ssd, self.depth, self.order, self.n, self.wh = ssd, depth, list(order), len(frames), W * H
        self.frames, self.table = frames, table
        self.cfg = ssd.default_config(W, H, max_frames_per_batch=max_frames, batches_in_flight=lanes)
        self.rec = C.sizeof(ssd.FrameMoments)
        self.det = cs._identity_detector(ssd, self.cfg, device)
        self.det.set_cameras(list(table) + ([ssd.GeometricTransformation()] if spare else []))      # the last: a camera nobody uses
        self.buf, self.stride = cs._upload(ssd, frames, (8 if depth else 4) if pad is None else pad, device)
        self.lab_buf = ssd.DeviceBuffer(self.wh * self.n, device)
        self.first_buf = ssd.DeviceBuffer(self.rec * self.n, device)
        self.out = ssd.DeviceBuffer(self.rec * (self.n + 1), device)

    def close(self):
        for b in (self.buf, self.lab_buf, self.first_buf, self.out):
            b.free()
        self.det.close()

    def detect(self):
        """labels by one cameras enqueue, the first-pass records by the next (the one a refit is held to): (results, labels, records)"""
        d = self.det
        d.enqueue_cameras(self.buf.ptr, self.n, self.order, depth=self.depth, d_labels=self.lab_buf.ptr, stride_bytes=self.stride)
        d.fetch_list(self.n)
        self.lab = self.lab_buf.download(self.wh * self.n).reshape(self.n, self.wh).copy()
        d.enqueue_cameras_surface_moments(self.buf.ptr, self.n, self.order, self.first_buf.ptr, depth=self.depth, stride_bytes=self.stride)
        self.res = d.fetch_list(self.n)
        self.first = cs._records(self.ssd, self.first_buf.download(self.rec * self.n), self.n)
        return self.res, self.lab, self.first

    def refit(self, gates):
        self.out.upload(np.full(self.rec * (self.n + 1), POISON, dtype=np.uint8))      # the call zeroes its records itself
        self.det.enqueue_cameras_surface_refit(self.buf.ptr, self.n, gates, self.out.ptr, depth=self.depth, stride_bytes=self.stride)
        self.det.fetch_surface_refit()
        raw = self.out.download(self.rec * (self.n + 1))
        assert np.all(raw[self.rec * self.n:] == POISON), "a record past nframes was written"
        return cs._records(self.ssd, raw[:self.rec * self.n], self.n)

    def intr_of(self, i):
        cam = self.table[self.order[i]]
        return cam[1] if isinstance(cam, tuple) else None

    def host(self, gates):
        return [self.ssd.surface_refit_moments_host(self.cfg, f, l, g, m.n_surfaces, m.ground, intr=self.intr_of(i))
                for i, (f, l, g, m) in enumerate(zip(self.frames, self.lab, gates, self.first))]

    def gates(self, moments, k_sigma=2.5):
        return [self.ssd.surface_gates_from_moments(m, sm.MIN_POINTS, k_sigma, 0.0) for m in moments]

    def alone(self, i, chain, device):
        cfg = self.ssd.default_config(self.cfg.width, self.cfg.height, max_frames_per_batch=self.cfg.max_frames_per_batch)     # one workspace
        return _alone(self.ssd, cfg, self.table[self.order[i]], self.frames[i], self.depth, chain, device)


def _kept(m):
    return [int(m.s[k].m.n + m.s[k].n_far) for k in range(m.n_surfaces)]


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("shape", list(cs.SHAPES))
def test_each_frames_record_is_the_host_walks_and_its_one_camera_handles(ssd, gpu_device, shape, lanes):
    """two chained passes over six frames of four cameras: against the host function over the batch's own labels and against the
    one-camera handles, the record past nframes untouched, the results the enqueue's - with one workspace and with three"""
    assert ssd.BATCHES_IN_FLIGHT_THROUGHPUT == 3
    W, H, depth, frames, table, intr = _cameras(ssd, shape)
    b = CamBatch(ssd, gpu_device, W, H, depth, [frames[j] for j in ORDER], table, ORDER, lanes=lanes)
    try:
        assert b.stride % 16 != 0
        res, lab, first = b.detect()
        assert min(m.n_surfaces for m in first) >= 2 and max(m.n_surfaces for m in first) >= 3 and all(m.ground == 1 for m in first)
        cells = lab[:, :b.wh // 64 * 64].reshape(b.n, -1, 64)
        top, low = cells.max(axis=2), np.where(cells > 0, cells, 255).min(axis=2)
        assert ((top > 0) & (low < top)).sum() > 0, "a 64-point cell that carries two surfaces"
        chain, passes, cur = [], [], first
        for p in range(2):
            gates = b.gates(cur)
            got = b.refit(gates)
            _same(got, b.host(gates))
            chain.append(gates)
            passes.append(got)
            cur = got
        for i, j in enumerate(ORDER):
            want = b.alone(i, [chain[0][i], chain[1][i]], gpu_device)
            assert [bytes(passes[0][i]), bytes(passes[1][i])] == want, "frame %d (camera %d): not the one-camera handle's records" % (i, j)
        kept = [v for m in passes[0] for v in _kept(m)]
        full = [v for m in first for v in _kept(m)]
        assert all(0 < a <= f for a, f in zip(kept, full)) and sum(kept) < sum(full), "the gates trim something"
        assert [bytes(r) for r in b.det.fetch_list(b.n)] == [bytes(r) for r in res], "the results are still the enqueue's"
    finally:
        b.close()


@pytest.mark.gpu
def test_gates_go_by_frame_and_cameras_by_index(ssd, gpu_device):
    """positions 0 and 4 hold the same frame of camera 2 under gates of 2.0 and 3.0 rms: two records, each the one-camera handle's under
    its own gates (a kernel that read the gates by camera would give one of them twice); and one frame content named under two cameras"""
    W, H, depth, frames, table, intr = _cameras(ssd, "256x192")
    b = CamBatch(ssd, gpu_device, W, H, depth, [frames[j] for j in ORDER], table, ORDER)
    try:
        assert ORDER[0] == ORDER[4] == 2
        res, lab, first = b.detect()
        assert bytes(first[0]) == bytes(first[4])
        gates = b.gates(first)
        gates[0] = ssd.surface_gates_from_moments(first[0], sm.MIN_POINTS, 2.0, 0.0)
        gates[4] = ssd.surface_gates_from_moments(first[4], sm.MIN_POINTS, 3.0, 0.0)
        got = b.refit(gates)
        _same(got, b.host(gates))
        assert bytes(got[0]) != bytes(got[4]) and sum(_kept(got[0])) < sum(_kept(got[4]))
        for i in (0, 4):
            assert [bytes(got[i])] == b.alone(i, [gates[i]], gpu_device), i
    finally:
        b.close()
    # frame content of camera 0, named under camera 0 and under camera 3 (the mounting nearest to it: surfaces are found under both)
    b = CamBatch(ssd, gpu_device, W, H, depth, [frames[0], frames[0]], table, [0, 3])
    try:
        res, lab, first = b.detect()
        assert first[0].n_surfaces >= 3 and first[1].n_surfaces >= 2 and bytes(first[0]) != bytes(first[1])
        gates = []
        for _ in range(2):
            g = ssd.FrameGates()
            g.n_surfaces = ssd.MAX_STEPS
            for k in range(ssd.MAX_STEPS):
                g.g[k].n[:] = [0.0, 0.0, 1.0]
                g.g[k].dist, g.g[k].gate = 1.25, 0.25                 # the same band of camera z for every surface of either frame
            gates.append(g)
        got = b.refit(gates)
        _same(got, b.host(gates))
        assert bytes(got[0]) != bytes(got[1]) and all(0 < sum(_kept(g)) < sum(_kept(m)) for g, m in zip(got, first))
        for i in range(2):
            assert [bytes(got[i])] == b.alone(i, [gates[i]], gpu_device), i
    finally:
        b.close()


@pytest.mark.gpu
def test_points_on_the_gates_edge_under_a_camera_that_is_not_index_0_of_the_batch(ssd, gpu_device):
    """the cloud of the one-calibration gate-edge test on a tread of the frame at position 1 (camera 0 of the table, behind a frame of
    camera 2): labelled points moved in camera z onto dist +- gate and one float ulp beyond, the device held to the host and to the count"""
    W, H, depth, frames, table, intr = _cameras(ssd, "256x192")
    batch = [frames[j].copy() for j in ORDER]
    assert ORDER[1] == 0
    b0 = CamBatch(ssd, gpu_device, W, H, depth, batch, table, ORDER)
    try:
        res, lab, first = b0.detect()
    finally:
        b0.close()
    k = 1 if first[1].ground else 0                                # a tread of the frame at position 1
    assert first[1].n_surfaces > k
    pts = batch[1].reshape(-1, 3)
    mine = np.flatnonzero(lab[1] == k + 1)
    z = pts[mine, 2].astype(np.float64)
    gate = 2.0 ** -6
    dist = round(float(np.median(z)) * 1024) / 1024
    assert z.min() < dist - gate and z.max() > dist + gate, "the tread reaches beyond the gate on both sides"
    targets = [(dist + gate, True), (float(rm.up(dist + gate)), False), (dist - gate, True), (float(rm.down(dist - gate)), False)]
    moved = {}
    for zt, keep in targets:
        near = mine[np.argsort(np.abs(z - zt))]
        near = [i for i in near if i not in moved][:6]             # six points each: some keep their label after the move
        for i in near:
            pts[i, 2] = np.float32(zt)
            moved[i] = keep
    b = CamBatch(ssd, gpu_device, W, H, depth, batch, table, ORDER)
    try:
        res, lab, first = b.detect()
        still = [i for i in moved if lab[1][i] == k + 1]
        zs = pts[still, 2].astype(np.float64)
        assert (np.abs(zs - dist) == gate).sum() >= 2 and (np.abs(zs - dist) > gate).sum() >= 2, "points on the edge and beyond it are labelled"
        gates = b.gates(first)
        g = gates[1].g[k]
        g.n[:] = [0.0, 0.0, 1.0]
        g.dist, g.gate = dist, gate
        got = b.refit(gates)
        _same(got, b.host(gates))
        inside = (lab[1] == k + 1) & (np.abs(pts[:, 2].astype(np.float64) - dist) <= gate)
        assert int(got[1].s[k].m.n + got[1].s[k].n_far) == int(inside.sum())
        assert sm.frame_tuple(got[1])[2][k] == sm.moments_np(pts[inside], np.ones(int(inside.sum())), 1)[0]
        assert [bytes(got[1])] == b.alone(1, [gates[1]], gpu_device)
    finally:
        b.close()


@pytest.mark.gpu
def test_both_checks_instantiations(ssd, oracle, gpu_device):
    """a table of the common regime alone runs CHECKS = false; with a camera that needs the rare configurations' tests the whole batch
    runs CHECKS = true: every frame's refit record is its one-camera handle's either way"""
    w, h, table, frames = cs._regime_table(ssd, oracle)
    some = 0
    for tab, order in ((table[:1], [0, 0]), (table, [0, 1, 0, 2])):
        b = CamBatch(ssd, gpu_device, w, h, False, [frames[j] for j in order], tab, order, pad=0, spare=False)
        try:
            res, lab, first = b.detect()
            gates = b.gates(first)
            got = b.refit(gates)
            for i in range(b.n):
                assert [bytes(got[i])] == b.alone(i, [gates[i]], gpu_device), (order, i)
            some += sum(sum(_kept(m)) for m in got)
            assert 0 < sum(_kept(got[0])) < sum(_kept(first[0]))
        finally:
            b.close()
    assert some > 0


@pytest.mark.gpu
def test_depth_input_takes_each_cameras_own_intrinsics(ssd, gpu_device):
    """16-bit depth from cameras that differ in field of view and depth units, in another order than the table's: every record is the
    one-camera handle's with ssd_set_intrinsics of that camera"""
    W, H, depth, frames, table, intr = _cameras(ssd, "256x192-depth16")
    assert depth and len(set(bytes(i) for i in intr)) == 4 and len(set(cs.UNITS)) >= 3
    order = [3, 1, 0, 2, 1]
    b = CamBatch(ssd, gpu_device, W, H, True, [frames[j] for j in order], table, order)
    try:
        res, lab, first = b.detect()
        gates = b.gates(first, k_sigma=2.0)
        got = b.refit(gates)
        _same(got, b.host(gates))
        assert len(set(bytes(g) for g in got)) == 4, "four cameras, four records; camera 1 twice"
        for i in range(b.n):
            assert [bytes(got[i])] == b.alone(i, [gates[i]], gpu_device), i
            assert 0 < sum(_kept(got[i])) < sum(_kept(first[i]))
    finally:
        b.close()


@pytest.mark.gpu
def test_refits_behind_batches_of_different_workspaces_keep_their_own_index_and_gates(ssd, gpu_device):
    """three workspaces, no fetch between: enqueue A, refit A, enqueue B (another camera_of_frame, other gates), refit B, and A again
    under a third set of gates - each workspace keeps its own index, the device gates are one set, so each pass goes behind the one
    before; every record is its own batch's under its own index and gates"""
    W, H, depth, frames, table, intr = _cameras(ssd, "256x192")
    n, rec, fb = len(ORDER), C.sizeof(ssd.FrameMoments), W * H * 12
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    cfg1 = ssd.default_config(W, H, max_frames_per_batch=F)
    orders, sigmas = [ORDER, ORDER_B, ORDER], (2.5, 2.0, 3.0)
    det = cs._identity_detector(ssd, cfg, gpu_device)
    bufs = [ssd.DeviceBuffer(fb * n, gpu_device) for _ in orders]
    firsts = [ssd.DeviceBuffer(rec * n, gpu_device) for _ in orders]
    outs = [ssd.DeviceBuffer(rec * n, gpu_device) for _ in orders]
    try:
        det.set_cameras(table)
        for buf, o in zip(bufs, orders):
            buf.upload(np.ascontiguousarray(np.stack([frames[j] for j in o])))
        want, gates = [], []
        for j, (buf, fbuf, o) in enumerate(zip(bufs, firsts, orders)):          # one batch at a time: what each must give
            det.enqueue_cameras_surface_moments(buf.ptr, n, o, fbuf.ptr)
            det.fetch_list(n)
            first = cs._records(ssd, fbuf.download(rec * n), n)
            gates.append([ssd.surface_gates_from_moments(m, sm.MIN_POINTS, sigmas[j], 0.0) for m in first])
            det.enqueue_cameras_surface_refit(buf.ptr, n, gates[j], outs[j].ptr)
            det.fetch_surface_refit()
            want.append(outs[j].download(rec * n).tobytes())
            for i, c in enumerate(o):
                assert [want[j][i * rec:(i + 1) * rec]] == _alone(ssd, cfg1, table[c], frames[c], False, [gates[j][i]], gpu_device), (j, i)
        assert len(set(want)) == 3, "the batches' indices and gates differ, and so do their records"
        for out in outs:
            out.upload(np.full(rec * n, POISON, dtype=np.uint8))
        for buf, fbuf, o, g, out in zip(bufs, firsts, orders, gates, outs):
            det.enqueue_cameras_surface_moments(buf.ptr, n, o, fbuf.ptr)
            det.enqueue_cameras_surface_refit(buf.ptr, n, g, out.ptr)
        det.fetch_surface_refit()                                  # the last pass, and with it every one before
        assert [out.download(rec * n).tobytes() for out in outs] == want
    finally:
        for x in bufs + firsts + outs:
            x.free()
        det.close()


@pytest.mark.gpu
def test_the_refusals_of_the_cameras_refit_entry_point(ssd, gpu_device):
    """SSD_E_ARG before anything is launched or copied: the destination keeps its poison and the handle allocates nothing"""
    W, H, depth, frames, table, intr = _cameras(ssd, "256x192")
    n, rec, fb = len(ORDER), C.sizeof(ssd.FrameMoments), W * H * 12
    cfg = ssd.default_config(W, H, max_frames_per_batch=F)
    det = cs._identity_detector(ssd, cfg, gpu_device)
    buf, dbuf, out = ssd.DeviceBuffer(fb * n, gpu_device), ssd.DeviceBuffer(W * H * 2 * n, gpu_device), ssd.DeviceBuffer(rec * n, gpu_device)
    try:
        buf.upload(np.ascontiguousarray(np.stack([frames[j] for j in ORDER])))
        dbuf.upload(np.zeros(W * H * n, dtype=np.uint16))
        out.upload(np.full(rec * n, POISON, dtype=np.uint8))
        det.set_cameras(table)
        bytes0 = det.workspace_bytes
        arr = (ssd.FrameGates * n)()
        L = ssd.lib()

        def refused(match, ptr=buf.ptr, stride=fb, nf=n, inp=ssd.INPUT_VERTICES, g=arr, o=out.ptr):
            rc = L.ssd_enqueue_cameras_surface_refit(det._h, C.c_void_p(ptr), stride, nf, None, inp, g, C.c_void_p(o))
            assert rc == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        refused(b"no whole cameras enqueue")                         # nothing enqueued yet
        det.enqueue(buf.ptr, n)
        det.fetch_list(n)
        refused(b"one-calibration")                                  # a whole enqueue, but not a cameras batch: told apart from "none yet"
        assert b"no whole" not in L.ssd_last_error()
        det.enqueue(buf.ptr, n, stages=ssd.STAGE_ALL & ~64)          # a partial run (everything but k_final)
        refused(b"no whole cameras enqueue")
        det.enqueue_cameras(buf.ptr, n, ORDER)
        det.fetch_list(n)
        refused(b"nframes", nf=n - 1)
        refused(b"not the last enqueue's", stride=fb + 4)
        refused(b"not the last enqueue's", ptr=buf.ptr + fb)         # other frames
        refused(b"not the last enqueue's", ptr=dbuf.ptr, stride=W * H * 2, inp=ssd.INPUT_DEPTH16)       # the enqueue read vertices
        refused(b"input must be", inp=2)
        refused(b"null", g=None)
        refused(b"null", o=None)
        refused(b"null", ptr=None)
        rc = L.ssd_enqueue_cameras_surface_refit(None, C.c_void_p(buf.ptr), fb, n, None, 0, arr, C.c_void_p(out.ptr))
        assert rc == -1 and b"null" in L.ssd_last_error()
        det.set_cameras(table)                                       # the table's buffers are other ones: the enqueue is withdrawn
        refused(b"no whole cameras enqueue")
        assert det.workspace_bytes == bytes0, "a refused call allocates nothing"
        assert bytes(out.download(rec * n)) == bytes([POISON]) * (rec * n), "a refused call writes nothing"
        # accepted again behind a fresh cameras enqueue; the gate buffers are counted from the first accepted call
        det.enqueue_cameras(buf.ptr, n, ORDER)
        det.fetch_list(n)
        det.enqueue_cameras_surface_refit(buf.ptr, n, arr, out.ptr)
        det.fetch_surface_refit()
        assert det.workspace_bytes == bytes0 + 2 * F * C.sizeof(ssd.FrameGates)
        got = cs._records(ssd, out.download(rec * n), n)
        assert got[0].n_surfaces >= 2 and bytes(got[0])[8:] == bytes(rec - 8), "all-zero gates gather nothing"
        # the one-calibration entry point still refuses a cameras batch
        rc = L.ssd_enqueue_surface_refit(det._h, C.c_void_p(buf.ptr), fb, n, None, 0, arr, C.c_void_p(out.ptr))
        assert rc == -1 and b"cameras batch" in L.ssd_last_error()
        # ... and a labels enqueue or a surface-moments enqueue of a cameras batch is refit as well
        det.enqueue_cameras_surface_moments(buf.ptr, n, ORDER, out.ptr)
        det.fetch_list(n)
        first = cs._records(ssd, out.download(rec * n), n)
        gates = [ssd.surface_gates_from_moments(m, sm.MIN_POINTS, 2.5, 0.0) for m in first]
        det.enqueue_cameras_surface_refit(buf.ptr, n, gates, out.ptr)
        det.fetch_surface_refit()
        got = cs._records(ssd, out.download(rec * n), n)
        assert all(0 < sum(_kept(g)) < sum(_kept(m)) for g, m in zip(got, first))
        assert det.workspace_bytes == bytes0 + 2 * F * C.sizeof(ssd.FrameGates)
    finally:
        buf.free()
        dbuf.free()
        out.free()
        det.close()


@pytest.mark.gpu
def test_dead_frames_come_out_all_zero(ssd, gpu_device):
    """a frame the reference would have thrown on, a staircase and a frame without stairs (the scenes of the one-calibration test), named
    under cameras 1 and 2 of a table whose camera 0 is the identity: all zero, the first pass's under a huge gate, all zero; and gates
    that are not finite numbers above 0 gather nothing and keep the header"""
    scs = [scenes.make(ssd, "vga_yaw50_throws"), scenes.make(ssd, "vga_3steps_noise2mm"), scenes.make(ssd, "vga_empty")]
    trans = ssd.transformation_for_scene(scs[0])
    frames = list(ssd.synth_host(scs))
    table = [ssd.GeometricTransformation(), trans, ssd.transformation_for_scene(scs[0])]
    b = CamBatch(ssd, gpu_device, scs[0].width, scs[0].height, False, frames, table, [1, 2, 1], pad=0)
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
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            for g in gates:
                for k in range(ssd.MAX_STEPS):
                    g.g[k].gate = bad
            got = b.refit(gates)
            assert bytes(got[0]) == bytes(b.rec) and bytes(got[2]) == bytes(b.rec)
            assert (got[1].n_surfaces, got[1].ground) == (first[1].n_surfaces, first[1].ground), "the header is kept"
            assert bytes(got[1])[8:] == bytes(b.rec - 8), bad
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2])
def test_the_host_path_over_more_than_one_slice(ssd, gpu_device, passes):
    """40 frames of four cameras cycling through 32-frame slices: results = ssd_process_host_cameras', first = the cameras surface
    fit's records, refit = the chain of host functions over the batch's labels pass by pass, out = ssd_surface_fit_solve of the last
    pass under the frame's camera; and Detector.camera_drift folds what it says it folds"""
    W, H = 256, 192
    n = 40
    which = [i % 4 for i in range(n)]
    scs = [ssd.make_scene(W, H, n_steps=3 if i % 5 else 0, seed=100 + i, sigma=0.001 + 0.0002 * (i % 4), **cs.POSES[which[i]]) for i in range(n)]
    trans = [ssd.transformation_for_scene(scs[j]) for j in range(4)]
    assert all(bytes(ssd.transformation_for_scene(scs[i]).constants) == bytes(trans[which[i]].constants) for i in range(n))
    cfg = ssd.default_config(W, H, max_frames_per_batch=32)
    xyz = ssd.synth_host(scs)
    det = cs._identity_detector(ssd, cfg, gpu_device)
    try:
        det.set_cameras(trans)
        want_res = det.process_host_cameras(xyz, which)
        _, lab = det.process_host_cameras(xyz, which, labels=True)
        lab = lab.reshape(n, W * H)
        _, _, want_first = det.process_host_cameras_surfaces(xyz, which, min_points=sm.MIN_POINTS, moments=True)
        res, fits, first, refit = det.process_host_cameras_surfaces_refit(xyz, which, min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0, passes=passes, moments=True)
        assert [bytes(r) for r in res] == [bytes(r) for r in want_res]
        assert [bytes(m) for m in first] == [bytes(m) for m in want_first]
        assert sum(1 for m in first if m.n_surfaces >= 3) >= 20 and sum(1 for m in first if m.n_surfaces == 0) >= 8
        for i in range(n):
            chain = rm.refit_chain(ssd, cfg, xyz[i], lab[i], first[i], 2.5, passes=passes)
            assert bytes(refit[i]) == bytes(chain[-1]), i
            assert bytes(fits[i]) == bytes(ssd.surface_fit_solve(chain[-1], trans[which[i]], sm.MIN_POINTS)), i
        res2, fits2 = det.process_host_cameras_surfaces_refit(xyz, which, min_points=sm.MIN_POINTS, passes=passes)      # without the moments
        assert [bytes(f) for f in fits2] == [bytes(f) for f in fits] and [bytes(r) for r in res2] == [bytes(r) for r in want_res]
        L = ssd.lib()
        idx = np.asarray(which, dtype=np.uint16)
        pidx = idx.ctypes.data_as(C.POINTER(C.c_uint16))
        r1, o1 = (ssd.FrameResult * n)(), (ssd.FrameSurfaces * n)()
        for bad in (0, 5):
            assert L.ssd_process_host_cameras_surfaces_refit(det._h, xyz.ctypes.data_as(C.c_void_p), n, pidx, 0, r1, None, None, 200, 2.5, 0.0, bad, o1) == -1
            assert b"passes" in L.ssd_last_error()
        assert L.ssd_process_host_cameras_surfaces_refit(det._h, xyz.ctypes.data_as(C.c_void_p), n, pidx, 0, r1, None, None, 200, 0.0, 0.0, 1, o1) == -1
        assert b"k_sigma" in L.ssd_last_error()
        idx[7] = 4
        assert L.ssd_process_host_cameras_surfaces_refit(det._h, xyz.ctypes.data_as(C.c_void_p), n, pidx, 0, r1, None, None, 200, 2.5, 0.0, 1, o1) == -1
        assert b"names camera 4 of 4" in L.ssd_last_error()
        # the drift watch: passes = 0 is the fold of the first-pass records as before, passes >= 1 the fold of the last refit pass's
        res_d, drift0 = det.camera_drift(xyz, which)
        assert [bytes(r) for r in res_d] == [bytes(r) for r in want_res]
        assert [bytes(d) for d in drift0] == [bytes(d) for d in ssd.camera_drift_fold(want_first, which, trans)]
        assert [bytes(d) for d in det.camera_drift(xyz, which, passes=0)[1]] == [bytes(d) for d in drift0]
        res_d, drift = det.camera_drift(xyz, which, passes=passes)
        assert [bytes(r) for r in res_d] == [bytes(r) for r in want_res]
        assert [bytes(d) for d in drift] == [bytes(d) for d in ssd.camera_drift_fold(refit, which, trans)]
        assert all(d.fit.status == ssd.GF_OK and 0 < d.m.n < d0.m.n for d, d0 in zip(drift, drift0))
    finally:
        det.close()
