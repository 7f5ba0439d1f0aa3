"""Surface gates on the device (k_surface_gates; include/ssd_hip.h): the kernel against the host function over
the golden records (tests/golden/solve_goldens.json), byte for byte; refit passes chained on the device with no fetch between against
the host-gated passes of the same handle; the cameras form; the host paths with device_gates against the ones without; the refusals."""
import ctypes as C

import numpy as np
import pytest

import camera_drift_model as cdm
import ground_model as gm
import solve_goldens as sg
import surface_model as sm
import test_gpu_camera_surfaces as cs
from test_gpu_camera_surfaces_refit import CamBatch, _cameras
from test_gpu_surface_fit import _records, _scenes
from test_gpu_surface_refit import CASES, POISON, Batch, _same

GARBAGE = 0x5A


def _golden_frames(ssd):
    """the golden records as FrameMoments with garbage where nothing may be read (the surfaces at k >= n_surfaces), and last a record
    with n_surfaces = 40 and garbage all through: (records to upload, records the host function is asked about)"""
    recs = sg.doc()["records"]
    size, per = C.sizeof(ssd.FrameMoments), C.sizeof(ssd.SurfaceMoments)
    up, ask = [], []
    for r in recs:
        fm = sg.frame_moments(ssd, r)
        raw = bytearray(bytes(fm))
        at = 8 + per * r["n_surfaces"]
        raw[at:] = bytes([GARBAGE]) * (size - at)
        up.append(bytes(raw))
        ask.append(ssd.FrameMoments.from_buffer_copy(bytes(raw)))
    bad = bytearray([GARBAGE]) * size
    bad[0:4] = (40).to_bytes(4, "little")
    up.append(bytes(bad))
    ask.append(None)
    return up, ask


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [0, 1, 2])
def test_the_kernels_gates_are_the_host_functions_byte_for_byte(ssd, gpu_device, rule):
    """(a) every golden record, frames with n_surfaces 0 and 17 among them, and one with n_surfaces = 40: all 688 bytes of each, into a
    poisoned buffer; the bytes past nframes records stay poison - for the whole batch and for its first three records alone"""
    mp, ks, gmin = sg.rules()[rule]
    assert (mp, ks, gmin) == [(200, 2.5, 0.0), (1, 16.0, 0.0), (200, 2.0, 2.0 ** -10)][rule]
    up, ask = _golden_frames(ssd)
    n, rec, gsz = len(up), C.sizeof(ssd.FrameMoments), C.sizeof(ssd.FrameGates)
    assert gsz == 688 and {0, 17} <= {m.n_surfaces for m in ask if m is not None} and n % 8 != 0
    want = [bytes(ssd.surface_gates_from_moments(m, mp, ks, gmin)) if m is not None else bytes(gsz) for m in ask]
    for r, w in zip(sg.doc()["records"], want):
        assert w == bytes(sg.gates_of(ssd, r, rule)), "the host function on this machine gives the goldens"
    sc = ssd.make_scene(256, 192, n_steps=3, seed=11)
    det = ssd.Detector(ssd.default_config(256, 192, max_frames_per_batch=n), ssd.transformation_for_scene(sc), gpu_device)
    src, dst = ssd.DeviceBuffer(rec * n, gpu_device), ssd.DeviceBuffer(gsz * (n + 2), gpu_device)
    try:
        bytes0 = det.workspace_bytes
        src.upload(np.frombuffer(b"".join(up), dtype=np.uint8))
        for count in (n, 3):
            dst.upload(np.full(gsz * (n + 2), POISON, dtype=np.uint8))
            det.enqueue_surface_gates(src.ptr, count, dst.ptr, min_points=mp, k_sigma=ks, gate_min=gmin)
            ssd.lib().ssd_device_sync(gpu_device)
            got = dst.download(gsz * (n + 2)).tobytes()
            for i in range(count):
                assert got[i * gsz:(i + 1) * gsz] == want[i], "frame %d (%s)" % (i, sg.doc()["records"][i]["name"] if i < n - 1 else "n_surfaces = 40")
            assert got[count * gsz:] == bytes([POISON]) * (gsz * (n + 2 - count)), "bytes past nframes records were written"
        assert det.workspace_bytes == bytes0, "the gates alone take nothing of the handle"
    finally:
        src.free()
        dst.free()
        det.close()


def _poison(b, buf=None):
    (buf or b.out).upload(np.full(b.rec * b.n, POISON, dtype=np.uint8))


def _host_gated(b, first, passes=2):
    """the existing path on the same handle: gates on the host from the records of the pass before -> [records per pass]"""
    out, cur = [], first
    for _ in range(passes):
        gates = b.gates(cur)
        cur = b.refit(gates)
        _same(cur, b.host(gates))
        out.append(cur)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,depth", CASES)
def test_the_chain_on_the_device_equals_the_host_gated_passes(ssd, gpu_device, shape, depth):
    """(b) detect, then enqueue_surface_moments, refit_device(first -> out), refit_device(out -> out) with no fetch between: pass 1 (a
    chain of its own) and pass 2 are the host-gated passes' records on the same handle, and so the host walk's; with three workspaces
    two batches go through the chain back to back and are fetched afterwards"""
    b = Batch(ssd, gpu_device, shape, depth)
    kw = dict(min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0, depth=depth)
    try:
        res, lab, first = b.detect()
        assert max(r.n_steps for r in res) >= 3 and res[-1].n_steps == 0
        want = _host_gated(b, first)
        assert [bytes(m) for m in want[0]] != [bytes(m) for m in want[1]], "the second pass moves something"
        d = b.det
        _poison(b)
        d.enqueue_surface_moments(b.ptr, b.n, b.first_buf.ptr, depth=depth, stride_bytes=b.stride)
        d.enqueue_surface_refit_device(b.ptr, b.n, b.first_buf.ptr, b.out.ptr, stride_bytes=b.stride, **kw)
        d.fetch_list(b.n)
        d.fetch_surface_refit()
        _same(_records(ssd, b.out.download(b.rec * b.n), b.n), want[0])
        _poison(b)
        _poison(b, b.first_buf)
        d.enqueue_surface_moments(b.ptr, b.n, b.first_buf.ptr, depth=depth, stride_bytes=b.stride)
        d.enqueue_surface_refit_device(b.ptr, b.n, b.first_buf.ptr, b.out.ptr, stride_bytes=b.stride, **kw)
        d.enqueue_surface_refit_device(b.ptr, b.n, b.out.ptr, b.out.ptr, stride_bytes=b.stride, **kw)
        got_res = d.fetch_list(b.n)
        d.fetch_surface_refit()
        got = _records(ssd, b.out.download(b.rec * b.n), b.n)
        _same(got, want[1])
        _same(_records(ssd, b.first_buf.download(b.rec * b.n), b.n), first)
        assert [bytes(r) for r in got_res] == [bytes(r) for r in res], "the batch's results are still the enqueue's"
        assert bytes(got[-1]) == bytes(b.rec), "the no-stairs frame's record is all zero"
    finally:
        b.close()
    # several workspaces: batch A, and batch B = A's frames in reverse, each through the chain; both fetched at the end
    b3 = Batch(ssd, gpu_device, shape, depth, lanes=ssd.BATCHES_IN_FLIGHT_THROUGHPUT, frames=b.frames)
    rev = ssd.DeviceBuffer(b3.stride * b3.n, gpu_device)
    first_b, out_b = ssd.DeviceBuffer(b3.rec * b3.n, gpu_device), ssd.DeviceBuffer(b3.rec * b3.n, gpu_device)
    try:
        for i, f in enumerate(b3.frames[::-1]):
            rev.upload(np.ascontiguousarray(f), offset=i * b3.stride)
        d = b3.det
        for buf in (b3.out, out_b):
            _poison(b3, buf)
        for ptr, fbuf, obuf in ((b3.ptr, b3.first_buf, b3.out), (rev.ptr, first_b, out_b)):
            d.enqueue_surface_moments(ptr, b3.n, fbuf.ptr, depth=depth, stride_bytes=b3.stride)
            d.enqueue_surface_refit_device(ptr, b3.n, fbuf.ptr, obuf.ptr, stride_bytes=b3.stride, **kw)
            d.enqueue_surface_refit_device(ptr, b3.n, obuf.ptr, obuf.ptr, stride_bytes=b3.stride, **kw)
        res_a = [bytes(r) for r in d.fetch(b3.n, back=1)]
        res_b = [bytes(r) for r in d.fetch(b3.n, back=0)]
        d.fetch_surface_refit()
        assert res_a == [bytes(r) for r in res] and res_b == res_a[::-1]
        _same(_records(ssd, b3.out.download(b3.rec * b3.n), b3.n), want[1])
        _same(_records(ssd, out_b.download(b3.rec * b3.n), b3.n), want[1][::-1])
    finally:
        for x in (rev, first_b, out_b):
            x.free()
        b3.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["256x192", "256x192-depth16"])
def test_the_cameras_chain_equals_the_host_gated_cameras_passes(ssd, gpu_device, shape):
    """(c) enqueue_cameras_surface_moments plus two enqueue_cameras_surface_refit_device, two cameras, no fetch between: the records of
    enqueue_cameras_surface_refit under host-made gates on the same handle"""
    W, H, depth, frames, table, intr = _cameras(ssd, shape)
    order = [1, 0, 1, 1, 0]
    b = CamBatch(ssd, gpu_device, W, H, depth, [frames[j] for j in order], table[:2], order, spare=False)
    kw = dict(min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0, depth=depth, stride_bytes=b.stride)
    try:
        res, lab, first = b.detect()
        assert min(m.n_surfaces for m in first) >= 2
        want, cur = [], first
        for _ in range(2):
            cur = b.refit(b.gates(cur))
            want.append(cur)
        assert bytes(want[0][0]) != bytes(want[0][1]) and [bytes(m) for m in want[0]] != [bytes(m) for m in want[1]]
        d = b.det
        for passes in (1, 2):
            b.out.upload(np.full(b.rec * (b.n + 1), POISON, dtype=np.uint8))
            d.enqueue_cameras_surface_moments(b.buf.ptr, b.n, order, b.first_buf.ptr, depth=depth, stride_bytes=b.stride)
            d.enqueue_cameras_surface_refit_device(b.buf.ptr, b.n, b.first_buf.ptr, b.out.ptr, **kw)
            if passes == 2:
                d.enqueue_cameras_surface_refit_device(b.buf.ptr, b.n, b.out.ptr, b.out.ptr, **kw)
            got_res = d.fetch_list(b.n)
            d.fetch_surface_refit()
            raw = b.out.download(b.rec * (b.n + 1))
            assert np.all(raw[b.rec * b.n:] == POISON), "a record past nframes was written"
            _same(cs._records(ssd, raw[:b.rec * b.n], b.n), want[passes - 1])
            assert [bytes(r) for r in got_res] == [bytes(r) for r in res]
    finally:
        b.close()


HOST_SCENES = {}


def _host_frames(ssd, depth, cameras):
    """40 frames (two slices of 32), every fifth without stairs; cameras: four mountings cycling"""
    key = (depth, cameras)
    if key not in HOST_SCENES:
        W, H = 256, 192
        which = [i % 4 for i in range(40)]
        pose = (lambda i: cs.POSES[which[i]]) if cameras else (lambda i: dict(roll_deg=25.0))
        scs = [ssd.make_scene(W, H, n_steps=3 if i % 5 else 0, seed=100 + i, sigma=0.001 + 0.0002 * (i % 4), **pose(i)) for i in range(40)]
        frames = ssd.synth_depth_host(scs) if depth else ssd.synth_host(scs)
        HOST_SCENES[key] = (W, H, scs, which, frames)
    return HOST_SCENES[key]


def _bytes_of(parts):
    return [[bytes(x) for x in p] for p in parts]


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("depth", [False, True])
def test_the_host_path_with_device_gates_equals_the_one_without(ssd, gpu_device, depth, passes):
    """(d) 40 frames through 32-frame slices: results, first, refit and the solved surfaces of device_gates=True are device_gates=False's"""
    W, H, scs, _, frames = _host_frames(ssd, depth, False)
    det = ssd.Detector(ssd.default_config(W, H, max_frames_per_batch=32), ssd.transformation_for_scene(scs[0]), gpu_device)
    try:
        if depth:
            det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
        kw = dict(depth=depth, min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0, passes=passes, moments=True)
        want = _bytes_of(det.process_host_surfaces_refit(frames, **kw))
        got = _bytes_of(det.process_host_surfaces_refit(frames, device_gates=True, **kw))
        for name, g, w in zip(("results", "surfaces", "first", "refit"), got, want):
            assert g == w, name
        assert want[2] != want[3] and sum(1 for m in want[2] if m != bytes(len(m))) >= 20, "staircases, and the refit trims them"
        res2, fits2 = det.process_host_surfaces_refit(frames, depth=depth, min_points=sm.MIN_POINTS, passes=passes, device_gates=True)   # without the moments
        assert _bytes_of((res2, fits2)) == want[:2]
        again = _bytes_of(det.process_host_surfaces_refit(frames, **kw))                 # and the host-gated path behind the device-gated one
        assert again == want
    finally:
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("depth", [False, True])
def test_the_cameras_host_path_with_device_gates_equals_the_one_without(ssd, gpu_device, depth, passes):
    W, H, scs, which, frames = _host_frames(ssd, depth, True)
    trans = [ssd.transformation_for_scene(scs[j]) for j in range(4)]
    table = [(t, ssd.intrinsics_for_scene(scs[j])) for j, t in enumerate(trans)] if depth else trans
    det = cs._identity_detector(ssd, ssd.default_config(W, H, max_frames_per_batch=32), gpu_device)
    try:
        det.set_cameras(table)
        kw = dict(depth=depth, min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0, passes=passes, moments=True)
        want = _bytes_of(det.process_host_cameras_surfaces_refit(frames, which, **kw))
        got = _bytes_of(det.process_host_cameras_surfaces_refit(frames, which, device_gates=True, **kw))
        for name, g, w in zip(("results", "surfaces", "first", "refit"), got, want):
            assert g == w, name
        assert want[2] != want[3] and sum(1 for m in want[2] if m != bytes(len(m))) >= 20
    finally:
        det.close()


@pytest.mark.gpu
def test_camera_drift_with_device_gates_equals_the_one_without(ssd, gpu_device):
    """(d) the drift watch over tests/camera_drift_model.py's table (a true entry, and one pitched by a degree and 2 cm low), two passes"""
    scs = [gm.scene(ssd, "steps", seed=seed, sigma=sigma) for seed, sigma in cdm.FRAMES]
    table = [ssd.transformation_for_scene(gm.scene(ssd, "steps", seed=cdm.FRAMES[0][0], sigma=cdm.FRAMES[0][1],
                                                   **{k: gm.POSE[k] + v for k, v in cdm.ENTRIES[e][1].items()})) for e in (0, 1)]
    frames = np.concatenate([ssd.synth_host(scs)] * 2)
    which = [0] * len(scs) + [1] * len(scs)
    det = cs._identity_detector(ssd, ssd.default_config(cdm.W, cdm.H, max_frames_per_batch=len(which)), gpu_device)
    try:
        det.set_cameras(table)
        res0, drift0 = det.camera_drift(frames, which, min_points=cdm.MIN_POINTS, passes=2)
        res1, drift1 = det.camera_drift(frames, which, min_points=cdm.MIN_POINTS, passes=2, device_gates=True)
        assert _bytes_of((res1, drift1)) == _bytes_of((res0, drift0))
        assert all(d.fit.status == ssd.GF_OK for d in drift1)
        plain = det.camera_drift(frames, which, min_points=cdm.MIN_POINTS)[1]
        assert all(0 < d.m.n < p.m.n for d, p in zip(drift1, plain)), "the fold of refit records, not of the first pass's"
    finally:
        det.close()


@pytest.mark.gpu
def test_the_refusals_of_the_device_gated_entry_points(ssd, gpu_device):
    """(e) SSD_E_ARG before anything is launched or copied: the destinations keep their poison and the handle allocates nothing"""
    W, H, scs = _scenes(ssd, "256x192")
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    det = ssd.Detector(ssd.default_config(W, H, max_frames_per_batch=n), trans, gpu_device)
    fb, rec, gsz = W * H * 12, C.sizeof(ssd.FrameMoments), C.sizeof(ssd.FrameGates)
    buf, first, out, gates = (ssd.DeviceBuffer(fb * n, gpu_device), ssd.DeviceBuffer(rec * n, gpu_device), ssd.DeviceBuffer(rec * n, gpu_device),
                              ssd.DeviceBuffer(gsz * n, gpu_device))
    L = ssd.lib()
    try:
        buf.upload(np.ascontiguousarray(ssd.synth_host(scs)))
        out.upload(np.full(rec * n, POISON, dtype=np.uint8))
        gates.upload(np.full(gsz * n, POISON, dtype=np.uint8))
        bytes0 = det.workspace_bytes

        def refused(match, cameras=False, frames=n, prev=first.ptr, ks=2.5, gmin=0.0, o=out.ptr):
            fn = L.ssd_enqueue_cameras_surface_refit_device if cameras else L.ssd_enqueue_surface_refit_device
            rc = fn(det._h, C.c_void_p(buf.ptr), fb, frames, None, 0, C.c_void_p(prev), 200, ks, gmin, C.c_void_p(o))
            assert rc == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        def no_gates(match, src=first.ptr, frames=n, ks=2.5, gmin=0.0, dst=gates.ptr):
            rc = L.ssd_enqueue_surface_gates(det._h, C.c_void_p(src), frames, None, 200, ks, gmin, C.c_void_p(dst))
            assert rc == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        refused(b"no whole enqueue")                                  # a refit with no whole enqueue
        refused(b"no whole cameras enqueue", cameras=True)
        det.enqueue_surface_moments(buf.ptr, n, first.ptr)
        det.fetch_list(n)
        refused(b"null", prev=None)
        refused(b"null", o=None)
        refused(b"k_sigma", ks=0.0)
        refused(b"k_sigma", ks=17.0)
        refused(b"gate_min", gmin=-1.0)
        refused(b"gate_min", gmin=float("nan"))
        refused(b"nframes", frames=0)
        refused(b"nframes", frames=n - 1)
        refused(b"one-calibration", cameras=True)                    # the cameras form after a one-calibration enqueue
        assert det.workspace_bytes == bytes0, "a refused call allocates nothing"
        det.set_cameras([trans])
        det.enqueue_cameras_surface_moments(buf.ptr, n, [0] * n, first.ptr)
        det.fetch_list(n)
        bytes0 = det.workspace_bytes                                 # with the table
        refused(b"cameras batch")                                    # ... and the reverse
        refused(b"k_sigma", cameras=True, ks=17.0)
        no_gates(b"null", src=None)
        no_gates(b"null", dst=None)
        no_gates(b"nframes", frames=0)
        no_gates(b"nframes", frames=n + 1)
        no_gates(b"k_sigma", ks=0.0)
        no_gates(b"k_sigma", ks=17.0)
        no_gates(b"gate_min", gmin=-1.0)
        assert det.workspace_bytes == bytes0, "a refused call allocates nothing"
        assert bytes(out.download(rec * n)) == bytes([POISON]) * (rec * n), "a refused call writes nothing"
        assert bytes(gates.download(gsz * n)) == bytes([POISON]) * (gsz * n)
        # accepted behind the cameras enqueue; the gate buffers are counted from the first accepted call, whatever its kind
        det.enqueue_cameras_surface_refit_device(buf.ptr, n, first.ptr, out.ptr)
        det.fetch_surface_refit()
        assert det.workspace_bytes == bytes0 + 2 * n * gsz
        got, was = _records(ssd, out.download(rec * n), n), _records(ssd, first.download(rec * n), n)
        assert 0 < got[0].s[0].m.n < was[0].s[0].m.n
    finally:
        for x in (buf, first, out, gates):
            x.free()
        det.close()
