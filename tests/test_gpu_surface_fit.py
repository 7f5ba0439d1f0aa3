"""Per-surface moments on the GPU (k_surface_moments; include/ssd_hip.h): the device's records against the host
sums over the labels the same handle returns for the same frames, bit for bit, and the entry points' contract."""
import ctypes as C

import numpy as np
import pytest

import ground_model as gm
import surface_model as sm

# poses whose camera rows cross from one surface to the next (rolled, XGA with low risers besides): cells that carry two surfaces
SHAPES = {
    "256x192": (256, 192, dict(roll_deg=25.0), 2),
    "250x190": (250, 190, dict(roll_deg=25.0), 2),
    "xga": (1024, 768, dict(roll_deg=30.0, rise=0.07), 3),
}
CASES = [("256x192", False), ("256x192", True), ("250x190", False), ("xga", False), ("xga", True)]     # depth input wants W % 4 == 0


def _scenes(ssd, shape):
    """the shape's staircases and, last, a frame of the same pose that shows the bare floor"""
    W, H, kw, n = SHAPES[shape]
    scs = [ssd.make_scene(W, H, n_steps=3, seed=11 + i, sigma=0.001 + 0.0005 * i, **kw) for i in range(n)]
    floor = dict(kw)
    floor.pop("rise", None)
    return W, H, scs + [ssd.make_scene(W, H, n_steps=0, seed=5, sigma=0.001, **floor)]


def _records(ssd, raw, n):
    return list((ssd.FrameMoments * n).from_buffer_copy(np.ascontiguousarray(raw).tobytes()))


def _upload(ssd, frames, depth, pad, device):
    """frames at a stride that is no multiple of 16 -> (buffer, pointer to the first frame, stride)"""
    fb = frames[0].nbytes
    stride = fb + pad
    buf = ssd.DeviceBuffer(stride * len(frames), device)
    for i, f in enumerate(frames):
        buf.upload(np.ascontiguousarray(f), offset=i * stride)
    return buf, buf.ptr, stride


def _host_sums(ssd, cfg, frames, labels, res, ground, intr=None):
    out = []
    for f, lab, r, g in zip(frames, labels, res, ground):
        live = not (r.status & ssd.ST_THROW) and r.n_steps > 0
        out.append(ssd.surface_moments_host(cfg, f, lab, r.n_steps if live else 0, g if live else 0, intr=intr))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,depth", CASES)
def test_device_moments_equal_the_sums_over_the_handles_labels(ssd, gpu_device, shape, depth):
    """one workspace (debug records on: m.n + n_far = n_in_quad, results = a plain enqueue's) and three with fetch_back"""
    W, H, scs = _scenes(ssd, shape)
    n, wh = len(scs), W * H
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n)
    intr = ssd.intrinsics_for_scene(scs[0]) if depth else None
    frames = list(ssd.synth_depth_host(scs)) if depth else list(ssd.synth_host(scs))
    rec_bytes = C.sizeof(ssd.FrameMoments)
    det = ssd.Detector(cfg, trans, gpu_device)
    bufs = []
    try:
        if depth:
            det.set_intrinsics(intr)
            res_l, lab = det.process_depth_host_labels(np.stack(frames))
        else:
            res_l, lab = det.process_host_labels(np.stack(frames))
        lab = lab.reshape(n, wh)
        # what the batch must hold, from the labels, before anything is uploaded
        assert max(r.n_steps for r in res_l) >= 3 and max(int(l.max()) for l in lab) >= 3, "a frame with at least three surfaces"
        assert res_l[-1].n_steps == 0 and not lab[-1].any(), "a no-stairs frame"
        cells = lab[:, :wh // 64 * 64].reshape(n, -1, 64)
        top, low = cells.max(axis=2), np.where(cells > 0, cells, 255).min(axis=2)
        assert ((top > 0) & (low < top)).sum() > 0, "a 64-point cell that carries two surfaces"

        buf, ptr, stride = _upload(ssd, frames, depth, 8 if depth else 4, gpu_device)
        bufs.append(buf)
        assert stride % 16 != 0
        out = ssd.DeviceBuffer(rec_bytes * n, gpu_device)
        bufs.append(out)
        out.upload(np.full(rec_bytes * n, 0xA5, dtype=np.uint8))             # the call zeroes the records itself
        det.set_debug(True, images=False)
        det.enqueue_surface_moments(ptr, n, out.ptr, depth=depth, stride_bytes=stride)
        res = det.fetch_list(n)
        got = _records(ssd, out.download(rec_bytes * n), n)
        dbg = [det.debug(i) for i in range(n)]
        assert [bytes(r) for r in res] == [bytes(r) for r in res_l]
        # results byte-equal to a plain enqueue of the same frames
        (det.enqueue_depth if depth else det.enqueue)(ptr, n, stride_bytes=stride)
        assert [bytes(r) for r in det.fetch_list(n)] == [bytes(r) for r in res]
        det.set_debug(False)

        ground = [1 if d.ground_ind >= 0 else 0 for d in dbg]
        want = _host_sums(ssd, cfg, frames, lab, res, ground, intr)
        for i in range(n):
            assert got[i].n_surfaces == want[i].n_surfaces and got[i].ground == want[i].ground, i
            assert sm.frame_tuple(got[i]) == sm.frame_tuple(want[i]), i
            assert bytes(got[i]) == bytes(want[i]), i
        assert bytes(got[-1]) == bytes(rec_bytes), "the no-stairs frame's record is all zero"
        # m.n + n_far = the debug record's n_in_quad
        for i in range(n - 1):
            d, r = dbg[i], res[i]
            valid = [k for k in range(d.first_valid_ind, d.n_plateaus) if d.plateaus[k].valid]
            for s in range(r.n_steps):
                cnt = int(got[i].s[s].m.n + got[i].s[s].n_far)
                if s == 0 and ground[i]:
                    assert cnt == d.ground_n_in_quad, (i, s)
                else:
                    assert cnt == d.plateaus[valid[s - ground[i]]].n_in_quad, (i, s)
                assert cnt > 0

        # three workspaces: the frames as three batches in flight, each into records of its own, fetched back in order
        cfg3 = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
        det3 = ssd.Detector(cfg3, trans, gpu_device)
        try:
            if depth:
                det3.set_intrinsics(intr)
            parts = [(0, 1), (1, n - 2), (n - 1, 1)]
            out3 = ssd.DeviceBuffer(rec_bytes * n, gpu_device)
            bufs.append(out3)
            out3.upload(np.full(rec_bytes * n, 0x5A, dtype=np.uint8))
            for at, m in parts:
                det3.enqueue_surface_moments(ptr + at * stride, m, out3.ptr + at * rec_bytes, depth=depth, stride_bytes=stride)
            for back, (at, m) in zip((2, 1, 0), parts):
                r3 = det3.fetch(m, back=back)
                assert [bytes(r3[j]) for j in range(m)] == [bytes(r) for r in res[at:at + m]]
                part = _records(ssd, out3.download(rec_bytes * m, offset=at * rec_bytes), m)
                assert [bytes(p) for p in part] == [bytes(g) for g in got[at:at + m]], at
        finally:
            det3.close()
    finally:
        for b in bufs:
            b.free()
        det.close()


@pytest.mark.gpu
def test_points_at_and_beyond_16_m_are_counted_in_n_far(ssd, gpu_device):
    """a detecting cloud shifted by 15.95 m in camera x, with b compensating (world = a (p - shift) + b): part of it has x >= 16 m"""
    W, H = 256, 192
    sc = gm.scene(ssd, "steps")
    trans = ssd.transformation_for_scene(sc)
    a = np.array(list(trans.constants.a), dtype=np.float64).reshape(3, 3)
    shift = np.array([15.95, 0.0, 0.0])
    use = ssd.GeometricTransformation()
    C.memmove(C.byref(use.constants), C.byref(trans.constants), C.sizeof(use.constants))
    b = np.array(list(trans.constants.b)) - a @ shift
    for i in range(3):
        use.constants.b[i] = b[i]
    xyz = ssd.synth_host([sc])[0].reshape(-1, 3).copy()
    valid = xyz[:, 2] > 0
    xyz[valid] = (xyz[valid].astype(np.float64) + shift).astype(np.float32)
    xyz = xyz.reshape(1, H, W, 3)
    assert (xyz[..., 0] >= 16.0).sum() > 100 and (xyz[..., 0][xyz[..., 2] > 0] < 16.0).sum() > 100
    cfg = ssd.default_config(W, H, max_frames_per_batch=1)
    det = ssd.Detector(cfg, use, gpu_device)
    rec_bytes = C.sizeof(ssd.FrameMoments)
    buf = ssd.DeviceBuffer(xyz.nbytes, gpu_device)
    out = ssd.DeviceBuffer(rec_bytes, gpu_device)
    try:
        res_l, lab = det.process_host_labels(xyz)
        assert res_l[0].n_steps >= 2 and not (res_l[0].status & ssd.ST_THROW), "the shifted cloud still detects"
        buf.upload(xyz)
        det.set_debug(True, images=False)
        det.enqueue_surface_moments(buf.ptr, 1, out.ptr)
        res = det.fetch_list(1)
        ground = 1 if det.debug(0).ground_ind >= 0 else 0
        got = _records(ssd, out.download(rec_bytes), 1)[0]
        want = ssd.surface_moments_host(cfg, xyz[0], lab[0], res[0].n_steps, ground)
        assert bytes(got) == bytes(want)
        far = [int(got.s[k].n_far) for k in range(got.n_surfaces)]
        assert sum(far) > 0 and sum(int(got.s[k].m.n) for k in range(got.n_surfaces)) > 0, far
        assert [int(got.s[k].m.n + got.s[k].n_far) for k in range(ssd.MAX_STEPS)] == [int(c) for c in np.bincount(lab[0].reshape(-1), minlength=ssd.MAX_STEPS + 1)[1:]]
    finally:
        buf.free()
        out.free()
        det.close()


@pytest.mark.gpu
def test_the_surface_moments_contract(ssd, gpu_device):
    """workspace bytes unchanged until the first call; the host entry point over three slices = the enqueue path followed by
    ssd_surface_fit_solve; detection batches in flight are left alone; the pass's time; a null destination"""
    W, H, scs = _scenes(ssd, "256x192")
    scs = scs + scs[:2]                                       # five frames, two per slice: three slices
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=2, batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    xyz = ssd.synth_host(scs)
    fb = W * H * 12
    rec_bytes = C.sizeof(ssd.FrameMoments)
    det = ssd.Detector(cfg, trans, gpu_device)
    plain = ssd.Detector(cfg, trans, gpu_device)
    buf = ssd.DeviceBuffer(fb * n, gpu_device)
    out = ssd.DeviceBuffer(rec_bytes * n, gpu_device)
    try:
        assert det.workspace_bytes == plain.workspace_bytes
        buf.upload(np.ascontiguousarray(xyz))
        assert ssd.lib().ssd_enqueue_surface_moments(det._h, C.c_void_p(buf.ptr), fb, 1, None, None) == -1
        assert b"null" in ssd.lib().ssd_last_error()
        assert det.workspace_bytes == plain.workspace_bytes
        # the enqueue path, batch by batch, beside plain detection of the same frames
        want_res = []
        for at in range(0, n, 2):
            m = min(2, n - at)
            plain.enqueue(buf.ptr + at * fb, m)
            want_res += plain.fetch_list(m)
        # detection batches in flight around a batch with surface moments: plain, with moments, plain - each result its own
        det.enqueue(buf.ptr, 2)
        det.enqueue_surface_moments(buf.ptr + 2 * fb, 2, out.ptr + 2 * rec_bytes)
        det.enqueue(buf.ptr + 4 * fb, 1)
        got_res = []
        for back, m in ((2, 2), (1, 2), (0, 1)):
            r = det.fetch(m, back=back)
            got_res += [bytes(r[j]) for j in range(m)]
        assert got_res == [bytes(r) for r in want_res]
        det.enqueue_surface_moments(buf.ptr, 2, out.ptr)
        det.enqueue_surface_moments(buf.ptr + 4 * fb, 1, out.ptr + 4 * rec_bytes)
        det.fetch(2, back=1)
        det.fetch(1, back=0)
        mom = _records(ssd, out.download(rec_bytes * n), n)
        assert max(m.n_surfaces for m in mom) >= 3 and bytes(mom[2]) == bytes(rec_bytes)
        # the host entry point: three slices
        res_h, fits_h, mom_h = det.process_host_surfaces(xyz, min_points=sm.MIN_POINTS, moments=True)
        assert [bytes(r) for r in res_h] == [bytes(r) for r in want_res]
        assert [bytes(m) for m in mom_h] == [bytes(m) for m in mom]
        want_fits = [ssd.surface_fit_solve(m, trans, sm.MIN_POINTS) for m in mom]
        assert [bytes(f) for f in fits_h] == [bytes(f) for f in want_fits]
        assert any(f.s[k].status == ssd.GF_OK for f in fits_h for k in range(f.n_surfaces))
        res_n, fits_n = det.process_host_surfaces(xyz, min_points=sm.MIN_POINTS)          # without the moments
        assert [bytes(f) for f in fits_n] == [bytes(f) for f in want_fits]
        # timing: the pass's time of an enqueue with surface moments, 0 for a plain one
        det.set_timing(True)
        det.enqueue_surface_moments(buf.ptr, 2, out.ptr)
        det.fetch(2)
        assert det.surface_moments_time_ms(0) > 0.0
        det.enqueue(buf.ptr, 2)
        det.fetch(2)
        assert det.surface_moments_time_ms(0) == 0.0
    finally:
        buf.free()
        out.free()
        det.close()
        plain.close()
