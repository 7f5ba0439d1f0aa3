"""Camera fold on the device (k_camera_fold, k_camera_ground_gates; include/ssd_hip.h): (a) the fold kernel
against the heads of ssd_camera_drift_fold's records, (b) the overlay against ssd_camera_ground_gates over that fold, (c) the refit
with the camera's gate against the host composition on the same handle, (d) the host-fed drift watch with the fold on the device
against the one without, (e) the resident drift watch, (f) the refusals - all byte for byte.  256 x 192 wherever frames are needed."""
import ctypes as C
import random

import numpy as np
import pytest

import surface_model as sm
import test_camera_fold as tcf
import test_gpu_camera_surfaces as cs
from test_gpu_camera_surfaces_refit import CamBatch
from test_gpu_surface_refit import POISON, _same

GARBAGE = 0x5A
MAX_FRAMES = 192
FOLD_MIN = 1000                                    # the cameras' folds at 256 x 192: a frame's floor holds a few thousand points
ORDER = cs.ORDER
ORDER_B = [1, 3, 0, 2, 1, 3]


class Rig:
    """a small handle (the fold and the overlay take only its device and its frame limit) and the buffers of one call"""

    def __init__(self, ssd, device):
        self.ssd, self.device = ssd, device
        sc = ssd.make_scene(256, 192, n_steps=3, seed=11)
        self.det = ssd.Detector(ssd.default_config(256, 192, max_frames_per_batch=MAX_FRAMES), ssd.transformation_for_scene(sc), device)
        self.rec, self.fsz, self.gsz = C.sizeof(ssd.FrameMoments), C.sizeof(ssd.CameraFold), C.sizeof(ssd.FrameGates)
        self.bufs = []

    def buffer(self, raw):
        b = self.ssd.DeviceBuffer(len(raw), self.device)
        b.upload(np.frombuffer(bytes(raw), dtype=np.uint8))
        self.bufs.append(b)
        return b

    def release(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def fold(self, recs, idx, ncams, start=None, tail=2):
        """records (bytes each) under the int32 index -> (bytes of each of the ncams CameraFold, the bytes behind them); start: the bytes
        of ncams records to accumulate onto, None: a buffer of poison and accumulate = 0"""
        n = len(recs)
        src = self.buffer(b"".join(recs))
        ind = self.buffer(np.asarray(idx, dtype=np.int32).tobytes())
        dst = self.buffer((start if start is not None else bytes([POISON]) * (self.fsz * ncams)) + bytes([POISON]) * (self.fsz * tail))
        self.det.enqueue_camera_fold(src.ptr, ind.ptr, n, ncams, dst.ptr, accumulate=start is not None)
        self.ssd.lib().ssd_device_sync(self.device)
        raw = dst.download(self.fsz * (ncams + tail)).tobytes()
        self.release()
        return [raw[c * self.fsz:(c + 1) * self.fsz] for c in range(ncams)], raw[ncams * self.fsz:]

    def host_fold(self, recs, idx, ncams, min_points=1):
        """ssd_camera_drift_fold over the frames whose index names a camera of the table (the others count nowhere) -> [CameraDrift]"""
        keep = [i for i, c in enumerate(idx) if 0 <= c < ncams]
        return self.ssd.camera_drift_fold([self.ssd.FrameMoments.from_buffer_copy(recs[i]) for i in keep], [idx[i] for i in keep], tcf.cams(self.ssd, ncams),
                                          min_points=min_points)

    def close(self):
        self.release()
        self.det.close()


@pytest.fixture(scope="module")
def rig(ssd, gpu_device):
    r = Rig(ssd, gpu_device)
    yield r
    r.close()


def _garbled(ssd, fm):
    """the record's bytes with garbage where the fold may not read: s[1..], and s[0] too unless the frame has a ground"""
    raw = bytearray(bytes(fm))
    at = 8 if fm.ground != 1 or fm.n_surfaces < 1 else 8 + C.sizeof(ssd.SurfaceMoments)
    raw[at:] = bytes([GARBAGE]) * (len(raw) - at)
    return bytes(raw)


def _crafted(ssd, nframes, ncams, seed):
    """nframes records and their index: sums of either sign that never overflow, every seventh frame without a ground and every seventh
    with n_surfaces = 0 (garbage in their s[0]), one camera of the table that no frame names (ncams > 1), an index of -1 and one of ncams"""
    rng = random.Random(seed)
    named = list(range(ncams - 1)) if ncams > 1 else [0]
    recs, idx = [], []
    for i in range(nframes):
        sums = [rng.randrange(1000, 50000)] + [rng.randrange(-(1 << 40), 1 << 40) for _ in range(3)]
        sums += [rng.randrange(0, 1 << 55), rng.randrange(-(1 << 54), 1 << 54), rng.randrange(-(1 << 54), 1 << 54), rng.randrange(0, 1 << 55),
                 rng.randrange(-(1 << 54), 1 << 54), rng.randrange(0, 1 << 55)]
        fm = tcf.record(ssd, sums, n_far=rng.randrange(0, 100), ground=0 if i % 7 == 4 else 1, n_surfaces=0 if i % 7 == 5 else 1 + i % 3)
        recs.append(_garbled(ssd, fm))
        idx.append(named[rng.randrange(len(named))])
    if nframes >= 63:
        idx[5], idx[nframes - 2] = -1, ncams
    return recs, idx


def _frames(ssd, shape, order):
    """the four mountings of the cameras tests, frame i from camera order[i] under a seed and a noise of its own - two frames of one camera
    differ, so a camera's fold is no frame's own plane -> (W, H, depth, frames, table)"""
    W, H, depth = cs.SHAPES[shape]
    kw = [dict(cs.POSES[j], **(cs.OPTICS[j] if depth else {})) for j in range(4)]
    scs = [ssd.make_scene(W, H, n_steps=3, seed=11 + j + 10 * i, sigma=0.001 + 0.0005 * j + 0.0003 * i, **kw[j]) for i, j in enumerate(order)]
    base = [ssd.make_scene(W, H, n_steps=3, seed=11 + j, **kw[j]) for j in range(4)]
    trans = [ssd.transformation_for_scene(sc) for sc in base]
    assert all(bytes(ssd.transformation_for_scene(sc).constants) == bytes(trans[j].constants) for sc, j in zip(scs, order))
    if depth:
        table = [(t, ssd.intrinsics_for_scene(sc, depth_units=u)) for t, sc, u in zip(trans, base, cs.UNITS)]
        frames = [ssd.synth_depth_host([sc], depth_units=cs.UNITS[j])[0] for sc, j in zip(scs, order)]
    else:
        table, frames = trans, list(ssd.synth_host(scs))
    return W, H, depth, frames, table


def _heads(drift):
    return [bytes(d)[:104] for d in drift]


@pytest.mark.gpu
@pytest.mark.parametrize("ncams", [1, 3, 5])
@pytest.mark.parametrize("nframes", [1, 63, 64, 65, 130])
def test_the_fold_is_the_host_functions_head(ssd, rig, nframes, ncams):
    """(a) crafted records at a chunk's edges: frames without a ground and without a surface, garbage wherever nothing may be read, a
    camera nobody names, indices outside the table; all 104 bytes of every record into poison, the bytes behind them untouched"""
    recs, idx = _crafted(ssd, nframes, ncams, 1000 * nframes + ncams)
    want = rig.host_fold(recs, idx, ncams)
    got, behind = rig.fold(recs, idx, ncams)
    assert got == _heads(want)
    assert behind == bytes([POISON]) * len(behind), "bytes behind ncams records were written"
    if nframes >= 63:
        assert sum(d.frames for d in want) == nframes - 2 and 0 < sum(d.frames_ground for d in want) < sum(d.frames for d in want)
        assert all(d.frames_left == 0 for d in want) and (ncams == 1 or want[ncams - 1].frames == 0)


def _placed(ssd, case, at):
    """an overflow case of the CPU file with `at` frames in front of it and some behind: fillers of a camera of their own (the table's
    last) and small records of camera 0 in turn -> (records, index, ncams)"""
    name, recs, idx, ncams, counts = case
    small = _garbled(ssd, tcf.record(ssd, tcf.SMALL, n_far=1))
    fill = lambda k: [(small, ncams if i % 2 == 0 else 0) for i in range(k)]
    rows = fill(at) + [(_garbled(ssd, r), c) for r, c in zip(recs, idx)] + fill(5)
    return [r for r, _ in rows], [c for _, c in rows], ncams + 1


@pytest.mark.gpu
@pytest.mark.parametrize("at", [0, 62, 63])
def test_the_overflow_rule_on_the_device(ssd, rig, at):
    """(a) every overflow record of the CPU file - a frame left and a later smaller one taken, n_far at INT64_MAX, -2^63, and the
    mixed-sign triple whose total fits while its prefix does not - inside one chunk (at = 0) and across two (at = 62: the triple's third
    frame, at = 63: its second and third lie in the next chunk)"""
    for case in tcf.overflow_cases(ssd):
        recs, idx, ncams = _placed(ssd, case, at)
        want = rig.host_fold(recs, idx, ncams)
        left = sum(d.frames_left for d in want)                      # the fillers of camera 0 in front may let one more frame fit
        assert left == sum(c[2] for c in case[4]) if at == 0 else left >= 1, case[0]
        got, behind = rig.fold(recs, idx, ncams)
        assert got == _heads(want), case[0]
        assert behind == bytes([POISON]) * len(behind)


@pytest.mark.gpu
def test_two_accumulating_calls_equal_one(ssd, rig):
    """(a) accumulate: a call over the first k frames into poison, one over the rest on top - the bytes of one call over all of them, with
    the overflow across the boundary (k = 1 of the mixed-sign triple: 2^62 is held, +2^62 is left, -2^62 taken) and with a boundary that
    is no chunk's"""
    triple = tcf.overflow_cases(ssd)[2]
    recs = [_garbled(ssd, r) for r in triple[1]]
    want = rig.host_fold(recs, triple[2], 1)
    assert (want[0].frames_ground, want[0].frames_left, want[0].m.ss[5]) == (2, 1, 0)
    part, _ = rig.fold(recs[:1], triple[2][:1], 1)
    got, behind = rig.fold(recs[1:], triple[2][1:], 1, start=b"".join(part))
    assert got == _heads(want) and behind == bytes([POISON]) * len(behind)
    for case in tcf.overflow_cases(ssd):
        recs, idx, ncams = _placed(ssd, case, 62)
        want = _heads(rig.host_fold(recs, idx, ncams))
        assert rig.fold(recs, idx, ncams)[0] == want
        for k in (1, 63, 64, len(recs) - 1):
            part, _ = rig.fold(recs[:k], idx[:k], ncams)
            assert part == _heads(rig.host_fold(recs[:k], idx[:k], ncams))
            assert rig.fold(recs[k:], idx[k:], ncams, start=b"".join(part))[0] == want, (case[0], k)
    recs, idx = _crafted(ssd, 130, 3, 7)
    part, _ = rig.fold(recs[:37], idx[:37], 3)
    assert rig.fold(recs[37:], idx[37:], 3, start=b"".join(part))[0] == _heads(rig.host_fold(recs, idx, 3))


def _sums_of_points(pts):
    """ten exact sums of integer points (q = the record's fixed point): n, s[3], ss[6] = xx, xy, xz, yy, yz, zz"""
    s = [sum(p[k] for p in pts) for k in range(3)]
    ss = [sum(p[a] * p[b] for p in pts) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return [len(pts)] + s + ss


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [(2.5, 0.0), (2.0, 2.0 ** -10)])
def test_the_overlay_is_the_host_functions(ssd, gpu_device, rig, rule):
    """(b) real first-pass records of six frames under two cameras, and crafted ones behind them: a camera FEW under fold_min_points, one
    DEGENERATE (collinear points), one whose plane is fine but gives no pose (its normal has no y: camera_to_world_from_plane fails), a
    groundless frame, a frame whose incoming gates have n_surfaces == 0, an index outside the table; all 688 bytes of every frame"""
    k_sigma, gate_min = rule
    order = [0, 1, 0, 1, 1, 0]
    W, H, depth, frames, table = _frames(ssd, "256x192", order)
    b = CamBatch(ssd, gpu_device, W, H, depth, frames, table[:2], order)
    try:
        first = b.detect()[2]
    finally:
        b.close()
    assert all(m.ground == 1 and m.n_surfaces >= 2 and m.s[0].m.n > FOLD_MIN for m in first)
    few = tcf.record(ssd, _sums_of_points([(x * 700, y * 900, 65536 + x * 13) for x in range(8) for y in range(8)]))
    line = tcf.record(ssd, _sums_of_points([(t * 20, t * 40 + 1000, 65536 + t * 60) for t in range(3000)]))
    flat = tcf.record(ssd, _sums_of_points([(x * 500, y * 500, 65536) for x in range(-30, 31) for y in range(-30, 31)]))
    groundless = ssd.FrameMoments.from_buffer_copy(first[0])
    groundless.ground = 0
    moments = list(first) + [few, line, flat, groundless, first[2], first[3]]
    idx = order + [2, 3, 4, 0, 0, 7]
    ncams = 7                                      # cameras 5 and 6: nobody names them
    cams = tcf.cams(ssd, ncams)
    gates = [ssd.surface_gates_from_moments(m, sm.MIN_POINTS, k_sigma, gate_min) for m in moments]
    gates[len(first) + 4] = ssd.FrameGates()       # first[2] again, its gates empty: n_surfaces is raised to 1
    keep = [i for i, c in enumerate(idx) if c < ncams]
    drift = ssd.camera_drift_fold([moments[i] for i in keep], [idx[i] for i in keep], cams, min_points=FOLD_MIN)
    assert [d.fit.status for d in drift] == [ssd.GF_OK, ssd.GF_OK, ssd.GF_FEW, ssd.GF_DEGENERATE, ssd.GF_DEGENERATE, ssd.GF_FEW, ssd.GF_FEW]
    assert gates[len(first) + 2].g[0].gate > 0 or gate_min == 0.0, "the flat record's own plane is fine"
    assert ssd.surface_gates_from_moments(flat, 1, 2.5, 1.0).g[0].n[2] in (1.0, -1.0) and drift[4].frames_ground == 1
    over = ssd.camera_ground_gates([moments[i] for i in keep], [idx[i] for i in keep], drift, [gates[i] for i in keep], k_sigma, gate_min)
    want = list(gates)
    for i, g in zip(keep, over):
        want[i] = g
    changed = [i for i in range(len(moments)) if bytes(want[i]) != bytes(gates[i])]
    assert changed == [0, 1, 2, 3, 4, 5, len(first) + 4], "the frames of cameras 0 and 1 with a ground, and no other"
    assert want[len(first) + 4].n_surfaces == 1
    try:
        src = rig.buffer(b"".join(bytes(m) for m in moments))
        ind = rig.buffer(np.asarray(idx, dtype=np.int32).tobytes())
        fold = rig.buffer(bytes([POISON]) * (rig.fsz * ncams))
        dst = rig.buffer(b"".join(bytes(g) for g in gates) + bytes([POISON]) * rig.gsz)
        n = len(moments)
        rig.det.enqueue_camera_fold(src.ptr, ind.ptr, n, ncams, fold.ptr)
        rig.det.enqueue_camera_ground_gates(src.ptr, ind.ptr, n, fold.ptr, ncams, dst.ptr, fold_min_points=FOLD_MIN, k_sigma=k_sigma, gate_min=gate_min)
        ssd.lib().ssd_device_sync(gpu_device)
        raw = dst.download(rig.gsz * (n + 1)).tobytes()
        assert fold.download(rig.fsz * ncams).tobytes() == b"".join(_heads(drift))
    finally:
        rig.release()
    for i in range(n):
        assert raw[i * rig.gsz:(i + 1) * rig.gsz] == bytes(want[i]), "frame %d" % i
    assert raw[n * rig.gsz:] == bytes([POISON]) * rig.gsz


def _composition(b, prev, k_sigma=2.5, gate_min=0.0):
    """the host composition in front of a pass: per-frame gates of `prev`, its fold against the handle's table, the camera's gate over
    the ground gates -> (per-frame gates, the gates with the cameras' on top)"""
    ssd = b.ssd
    gates = [ssd.surface_gates_from_moments(m, sm.MIN_POINTS, k_sigma, gate_min) for m in prev]
    drift = ssd.camera_drift_fold(prev, b.order, b.det._cameras, min_points=FOLD_MIN)
    return gates, ssd.camera_ground_gates(prev, b.order, drift, gates, k_sigma, gate_min), drift


def _folded(b, d_prev, **kw):
    b.det.enqueue_cameras_surface_refit_folded(b.buf.ptr, b.n, d_prev, b.out.ptr, min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0,
                                               fold_min_points=FOLD_MIN, depth=b.depth, stride_bytes=b.stride, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("shape", ["256x192", "256x192-depth16"])
def test_the_folded_refit_is_the_host_composition(ssd, gpu_device, shape, lanes):
    """(c) behind a cameras enqueue with its first moments: one folded pass (first -> out), and the chain of two with no fetch between,
    the second in place (d_prev == d_out) - against ssd_enqueue_cameras_surface_refit of the same handle under the gates the host makes
    from the downloaded records; the fold buffer is counted once"""
    W, H, depth, frames, table = _frames(ssd, shape, ORDER)
    b = CamBatch(ssd, gpu_device, W, H, depth, frames, table, ORDER, lanes=lanes)
    try:
        res, lab, first = b.detect()
        own, cam, drift = _composition(b, first)
        assert [d.fit.status for d in drift] == [ssd.GF_OK] * 4 + [ssd.GF_FEW] and [bytes(g) for g in own] != [bytes(g) for g in cam]
        want1 = b.refit(cam)
        assert [bytes(m) for m in want1] != [bytes(m) for m in b.refit(own)], "the camera's gate gathers other points than the frame's own"
        want2 = b.refit(_composition(b, want1)[1])
        bytes0 = b.det.workspace_bytes
        d = b.det
        for passes, want in ((1, want1), (2, want2)):
            b.out.upload(np.full(b.rec * (b.n + 1), POISON, dtype=np.uint8))
            d.enqueue_cameras_surface_moments(b.buf.ptr, b.n, b.order, b.first_buf.ptr, depth=b.depth, stride_bytes=b.stride)
            _folded(b, b.first_buf.ptr)
            if passes == 2:
                _folded(b, b.out.ptr)
            got_res = d.fetch_list(b.n)
            d.fetch_surface_refit()
            raw = b.out.download(b.rec * (b.n + 1))
            _same(cs._records(ssd, raw[:b.rec * b.n], b.n), want)
            assert np.all(raw[b.rec * b.n:] == POISON) and [bytes(r) for r in got_res] == [bytes(r) for r in res]
        assert d.workspace_bytes == bytes0 + ssd.MAX_CAMERAS * C.sizeof(ssd.CameraFold), "the fold buffer: once, one record per camera a table can hold"
    finally:
        b.close()


@pytest.mark.gpu
def test_two_folded_batches_back_to_back(ssd, gpu_device):
    """(c) three workspaces, no fetch between: batch A through moments and a folded pass, batch B (another index) through the same -
    each workspace keeps its own index, the fold buffer and the device gates are one set, so B's pass goes behind A's"""
    n, rec = len(ORDER), C.sizeof(ssd.FrameMoments)
    bs = []
    for k, o in enumerate((ORDER, ORDER_B)):
        W, H, depth, frames, table = _frames(ssd, "256x192", o)
        bs.append(CamBatch(ssd, gpu_device, W, H, depth, frames, table, o, lanes=3 if k == 0 else 1))
    a, bb = bs
    try:
        wants = []
        for b in bs:                                                 # what each must give, on a handle of its own
            first = b.detect()[2]
            wants.append(b.refit(_composition(b, first)[1]))
        assert [bytes(m) for m in wants[0]] != [bytes(m) for m in wants[1]]
        d = a.det                                                    # both batches through the handle with three workspaces
        outs = [a.out, a.first_buf]
        firsts = [ssd.DeviceBuffer(rec * n, gpu_device), ssd.DeviceBuffer(rec * n, gpu_device)]
        try:
            for o in outs:
                o.upload(np.full(rec * n, POISON, dtype=np.uint8))
            for b, fbuf, out in zip(bs, firsts, outs):
                d.enqueue_cameras_surface_moments(b.buf.ptr, n, b.order, fbuf.ptr, stride_bytes=b.stride)
                d.enqueue_cameras_surface_refit_folded(b.buf.ptr, n, fbuf.ptr, out.ptr, min_points=sm.MIN_POINTS, fold_min_points=FOLD_MIN, stride_bytes=b.stride)
            d.fetch_surface_refit()
            for out, want in zip(outs, wants):
                _same(cs._records(ssd, out.download(rec * n), n), want)
        finally:
            for x in firsts:
                x.free()
    finally:
        for b in bs:
            b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True])
@pytest.mark.parametrize("passes", [0, 2])
def test_the_host_path_with_the_fold_on_the_device(ssd, gpu_device, passes, depth):
    """(d) 40 frames of four cameras cycling through two 32-frame slices, every camera's frames on both: camera_drift(device_fold=True)
    against device_fold=False by the bytes of the results and of every CameraDrift"""
    W, H, n = 256, 192, 40
    which = [i % 4 for i in range(n)]
    optics = [cs.OPTICS[j] if depth else {} for j in range(4)]
    scs = [ssd.make_scene(W, H, n_steps=3 if i % 5 else 0, seed=100 + i, sigma=0.001 + 0.0002 * (i % 4), **cs.POSES[which[i]], **optics[which[i]]) for i in range(n)]
    trans = [ssd.transformation_for_scene(scs[j]) for j in range(4)]
    if depth:
        table = [(t, ssd.intrinsics_for_scene(scs[j], depth_units=cs.UNITS[j])) for j, t in enumerate(trans)]
        frames = np.stack([ssd.synth_depth_host([sc], depth_units=cs.UNITS[which[i]])[0] for i, sc in enumerate(scs)])
    else:
        table, frames = trans, ssd.synth_host(scs)
    det = cs._identity_detector(ssd, ssd.default_config(W, H, max_frames_per_batch=32), gpu_device)
    try:
        det.set_cameras(table)
        kw = dict(depth=depth, min_points=FOLD_MIN, passes=passes, k_sigma=2.0, gate_min=2.0 ** -10)
        res0, drift0 = det.camera_drift(frames, which, device_gates=True, **kw)
        res1, drift1 = det.camera_drift(frames, which, device_fold=True, **kw)
        assert [bytes(r) for r in res1] == [bytes(r) for r in res0]
        assert [bytes(d) for d in drift1] == [bytes(d) for d in drift0]
        assert all(d.fit.status == ssd.GF_OK and d.frames == 10 and d.frames_ground >= 6 for d in drift1)
        if passes:
            first = det.camera_drift(frames, which, depth=depth, min_points=FOLD_MIN, device_fold=True)[1]
            assert all(0 < d.m.n < f.m.n for d, f in zip(drift1, first)), "the refit records are folded, not the first pass's"
    finally:
        det.close()


@pytest.mark.gpu
def test_the_resident_drift_watch(ssd, gpu_device):
    """(e) camera_drift_resident over six resident frames of four cameras: with the camera's gate in front of the last of two passes, the
    CameraDrift bytes of the host composition over the device's own labels and records; without it, those of camera_drift(passes = 2,
    device_gates) over the same frames from the host"""
    W, H, depth, frames, table = _frames(ssd, "256x192", ORDER)
    b = CamBatch(ssd, gpu_device, W, H, depth, frames, table, ORDER, pad=0)
    try:
        res, lab, first = b.detect()
        pass1 = b.host(b.gates(first))
        pass2 = b.host(_composition(b, pass1)[1])
        want = ssd.camera_drift_fold(pass2, ORDER, b.det._cameras, min_points=FOLD_MIN)
        got_res, got = b.det.camera_drift_resident(b.buf.ptr, b.n, ORDER, min_points=sm.MIN_POINTS, fold_min_points=FOLD_MIN, passes=2, camera_gate=True)
        assert [bytes(d) for d in got] == [bytes(d) for d in want] and [bytes(r) for r in got_res] == [bytes(r) for r in res]
        assert [d.fit.status for d in got] == [ssd.GF_OK] * 4 + [ssd.GF_FEW]
        plain_res, plain = b.det.camera_drift(np.stack(b.frames), ORDER, min_points=FOLD_MIN, passes=2, device_gates=True)
        got_res, got2 = b.det.camera_drift_resident(b.buf.ptr, b.n, ORDER, min_points=sm.MIN_POINTS, fold_min_points=FOLD_MIN, passes=2, camera_gate=False)
        assert [bytes(d) for d in got2] == [bytes(d) for d in plain] and [bytes(r) for r in got_res] == [bytes(r) for r in plain_res]
        assert [bytes(d) for d in got2] != [bytes(d) for d in got]
        none_res, none = b.det.camera_drift_resident(b.buf.ptr, b.n, ORDER, fold_min_points=FOLD_MIN, passes=0)
        assert [bytes(d) for d in none] == [bytes(d) for d in ssd.camera_drift_fold(first, ORDER, b.det._cameras, min_points=FOLD_MIN)]
    finally:
        b.close()


@pytest.mark.gpu
def test_the_refusals_of_the_new_entry_points(ssd, gpu_device):
    """(f) SSD_E_ARG before anything is launched: the destinations keep their poison, the handle allocates nothing - and works afterwards"""
    W, H, depth, frames, table = _frames(ssd, "256x192", ORDER)
    b = CamBatch(ssd, gpu_device, W, H, depth, frames, table, ORDER)
    L = ssd.lib()
    n, rec, fsz, gsz = b.n, b.rec, C.sizeof(ssd.CameraFold), C.sizeof(ssd.FrameGates)
    ind, fold, gates = ssd.DeviceBuffer(4 * n, gpu_device), ssd.DeviceBuffer(fsz * 5, gpu_device), ssd.DeviceBuffer(gsz * n, gpu_device)
    try:
        res, lab, first = b.detect()
        ind.upload(np.asarray(ORDER, dtype=np.int32))
        fold.upload(np.full(fsz * 5, POISON, dtype=np.uint8))
        gates.upload(np.full(gsz * n, POISON, dtype=np.uint8))
        b.out.upload(np.full(rec * (n + 1), POISON, dtype=np.uint8))
        bytes0 = b.det.workspace_bytes
        h, vp = b.det._h, C.c_void_p

        def refused(rc, match):
            assert rc == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        good = dict(m=b.first_buf.ptr, i=ind.ptr, n=n, c=5, f=fold.ptr, g=gates.ptr, ks=2.5, gm=0.0)
        for bad, match in ((dict(m=None), b"null"), (dict(i=None), b"null"), (dict(f=None), b"null"), (dict(n=0), b"nframes"), (dict(n=b.cfg.max_frames_per_batch + 1), b"nframes"),
                           (dict(c=0), b"ncams"), (dict(c=ssd.MAX_CAMERAS + 1), b"ncams")):
            a = dict(good, **bad)
            refused(L.ssd_enqueue_camera_fold(h, vp(a["m"]), vp(a["i"]), a["n"], a["c"], 0, None, vp(a["f"])), match)
            refused(L.ssd_enqueue_camera_ground_gates(h, vp(a["m"]), vp(a["i"]), a["n"], vp(a["f"]), a["c"], FOLD_MIN, a["ks"], a["gm"], None, vp(a["g"])), match)
        for bad, match in ((dict(g=None), b"null"), (dict(ks=0.0), b"k_sigma"), (dict(ks=17.0), b"k_sigma"), (dict(gm=-1.0), b"gate_min"), (dict(gm=2.0), b"gate_min")):
            a = dict(good, **bad)
            refused(L.ssd_enqueue_camera_ground_gates(h, vp(a["m"]), vp(a["i"]), a["n"], vp(a["f"]), a["c"], FOLD_MIN, a["ks"], a["gm"], None, vp(a["g"])), match)

        def folded(ptr=b.buf.ptr, stride=b.stride, nf=n, inp=ssd.INPUT_VERTICES, prev=b.first_buf.ptr, ks=2.5, gm=0.0, o=b.out.ptr):
            return L.ssd_enqueue_cameras_surface_refit_folded(h, vp(ptr), stride, nf, None, inp, vp(prev), sm.MIN_POINTS, ks, gm, FOLD_MIN, vp(o))

        refused(folded(prev=None), b"null")
        refused(folded(o=None), b"null")
        refused(folded(ptr=None), b"null")
        refused(folded(ks=0.0), b"k_sigma")
        refused(folded(gm=1.5), b"gate_min")
        refused(folded(nf=n - 1), b"nframes")
        refused(folded(stride=b.stride + 4), b"not the last enqueue's")
        refused(folded(inp=2), b"input must be")
        b.det.enqueue(b.buf.ptr, n, stride_bytes=b.stride)
        b.det.fetch_list(n)
        refused(folded(), b"one-calibration")
        # the host path
        xyz = np.ascontiguousarray(np.stack(b.frames))
        idx = np.asarray(ORDER, dtype=np.uint16)
        pidx = idx.ctypes.data_as(C.POINTER(C.c_uint16))
        r1, out = (ssd.FrameResult * n)(), (ssd.CameraDrift * 5)()
        C.memset(out, POISON, C.sizeof(out))
        before = bytes(out)

        def drift(frames=xyz.ctypes.data_as(vp), nf=n, ix=pidx, r=r1, ks=2.5, gm=0.0, passes=2, o=out):
            return L.ssd_process_host_cameras_drift(h, frames, nf, ix, 0, r, sm.MIN_POINTS, ks, gm, passes, FOLD_MIN, o)

        for rc in (drift(frames=None), drift(r=None), drift(o=None), drift(nf=0), drift(ix=None)):
            assert rc == -1 and L.ssd_last_error()
        refused(drift(passes=-1), b"passes")
        refused(drift(passes=5), b"passes")
        refused(drift(ks=0.0), b"k_sigma")
        refused(drift(gm=2.0), b"gate_min")
        idx[3] = 5
        refused(drift(), b"names camera 5 of 5")
        idx[3] = ORDER[3]
        assert bytes(out) == before and b.det.workspace_bytes == bytes0, "a refused call writes and allocates nothing"
        assert fold.download(fsz * 5).tobytes() == bytes([POISON]) * (fsz * 5) and gates.download(gsz * n).tobytes() == bytes([POISON]) * (gsz * n)
        assert b.out.download(rec * (n + 1)).tobytes() == bytes([POISON]) * (rec * (n + 1))
        # the handle still works: the folded pass behind a fresh cameras enqueue is the host composition's
        b.det.enqueue_cameras_surface_moments(b.buf.ptr, n, ORDER, b.first_buf.ptr, stride_bytes=b.stride)
        b.det.fetch_list(n)
        want = b.refit(_composition(b, first)[1])
        b.det.enqueue_cameras_surface_moments(b.buf.ptr, n, ORDER, b.first_buf.ptr, stride_bytes=b.stride)
        _folded(b, b.first_buf.ptr)
        b.det.fetch_list(n)
        b.det.fetch_surface_refit()
        _same(cs._records(ssd, b.out.download(rec * n), n), want)
        assert drift() == 0 and [d.frames for d in out] == [ORDER.count(c) for c in range(5)]
    finally:
        for x in (ind, fold, gates):
            x.free()
        b.close()
