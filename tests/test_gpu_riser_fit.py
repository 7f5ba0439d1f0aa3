"""Riser moments on the GPU (k_riser_moments; include/ssd_hip.h): the device's records against the host sums over
the riser labels of tests/riser_model.py on the handle's own debug record, bit for bit; nothing else changes when the moments are
switched on; the host path over three slices; camera batches against one-camera handles; the entry points' contract."""
import ctypes as C

import numpy as np
import pytest

import riser_model as rm

TOL, SUPPORT = 0.03, 200
# poses whose camera rows cross from one riser to the next (rolled; XGA with low risers besides: several chunks per frame)
SHAPES = {
    "256x192": (256, 192, dict(roll_deg=25.0), 2),
    "250x190": (250, 190, dict(roll_deg=25.0), 2),
    "xga": (1024, 768, dict(roll_deg=30.0, rise=0.07), 1),
}
CASES = [("256x192", False), ("256x192", True), ("250x190", False), ("xga", False), ("xga", True)]     # depth input wants W % 4 == 0
ZERO = bytes(C.sizeof(C.c_int64) * 11 * 17 + 8)


def _scenes(ssd, shape):
    """the shape's staircases and, last, a frame of the same pose that shows the bare floor"""
    W, H, kw, n = SHAPES[shape]
    scs = [ssd.make_scene(W, H, n_steps=3, seed=11 + i, sigma=0.001 + 0.0005 * i, **kw) for i in range(n)]
    floor = dict(kw)
    floor.pop("rise", None)
    return W, H, scs + [ssd.make_scene(W, H, n_steps=0, seed=5, sigma=0.001, **floor)]


def _upload(ssd, frames, pad, device):
    """frames at a stride of their size + pad -> (buffer, stride)"""
    stride = frames[0].nbytes + pad
    buf = ssd.DeviceBuffer(stride * len(frames), device)
    for i, f in enumerate(frames):
        buf.upload(np.ascontiguousarray(f), offset=i * stride)
    return buf, stride


def _detector(ssd, cfg, trans, device, moments, intr=None):
    det = ssd.Detector(cfg, trans, device)
    if intr is not None:
        det.set_intrinsics(intr)
    det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
    if moments:
        det.set_riser_moments(True)
    return det


def _enqueue(det, ptr, n, depth, stride):
    (det.enqueue_depth if depth else det.enqueue)(ptr, n, stride_bytes=stride)
    return det.fetch_list(n), det.fetch_risers(n)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,depth", CASES)
def test_device_moments_equal_the_host_sums_over_the_models_labels(ssd, gpu_device, shape, depth):
    """debug records on (records only): each frame's ssd_fetch_riser_moments record = ssd_surface_moments_host over riser_labels of the
    handle's own debug record (its own fixed-point heights), byte for byte, and m.n + n_far = the riser's n_points"""
    W, H, scs = _scenes(ssd, shape)
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n)
    intr = ssd.intrinsics_for_scene(scs[0]) if depth else None
    frames = list(ssd.synth_depth_host(scs)) if depth else list(ssd.synth_host(scs))
    xyz = [ssd.deproject_host(intr, f) for f in frames] if depth else frames
    det = _detector(ssd, cfg, trans, gpu_device, True, intr)
    buf, stride = _upload(ssd, frames, 8 if depth else 4, gpu_device)
    try:
        assert stride % 16 != 0
        det.set_debug(True, images=False)
        res, ris = _enqueue(det, buf.ptr, n, depth, stride)
        got = det.fetch_riser_moments(n)
        dbg = [det.debug(i) for i in range(n)]
        det.set_debug(False)
        two = 0
        for i in range(n):
            labels = rm.riser_labels(cfg, trans.constants, dbg[i], xyz[i], TOL)
            want = ssd.surface_moments_host(cfg, frames[i], labels, ris[i].n_risers, 0, intr=intr)
            assert got[i].n_surfaces == ris[i].n_risers == max(res[i].n_steps - 1, 0) and got[i].ground == 0, i
            assert bytes(got[i]) == bytes(want), "frame %d: the device's record is not the host's sums" % i
            counts = np.bincount(labels, minlength=ssd.MAX_STEPS + 1)[1:]
            for k in range(ssd.MAX_STEPS):
                cnt = int(got[i].s[k].m.n + got[i].s[k].n_far)
                assert cnt == int(counts[k]) and cnt == (ris[i].risers[k].n_points if k < ris[i].n_risers else 0), (i, k)
            rows = labels.reshape(H, W)
            top, low = rows.max(axis=1), np.where(rows > 0, rows, 255).min(axis=1)
            two += int(((top > 0) & (low < top)).sum())
        assert max(r.n_risers for r in ris) >= 2 and all(ris[0].risers[k].n_points >= SUPPORT for k in range(2)), "risers with evidence"
        assert two > 0, "a camera row that crosses from one riser to the next"
        assert ris[-1].n_risers == 0 and bytes(got[-1]) == ZERO, "the bare floor: no riser, an all-zero record"
        # a second pass over the same frames: the records are zeroed in front of the kernel, not added to
        _enqueue(det, buf.ptr, n, depth, stride)
        assert [bytes(g) for g in det.fetch_riser_moments(n)] == [bytes(g) for g in got]
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("workspaces", [1, 3])
def test_switching_the_moments_on_changes_nothing_else(ssd, gpu_device, workspaces):
    """a handle with the moments on beside a handle with only risers on: ssd_frame_result and ssd_frame_risers byte for byte the same"""
    W, H, scs = _scenes(ssd, "256x192")
    n = len(scs)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=workspaces)
    intr = ssd.intrinsics_for_scene(scs[0])
    on, off = _detector(ssd, cfg, trans, gpu_device, True, intr), _detector(ssd, cfg, trans, gpu_device, False, intr)
    bufs = []
    try:
        for depth in (False, True):
            frames = list(ssd.synth_depth_host(scs)) if depth else list(ssd.synth_host(scs))
            buf, stride = _upload(ssd, frames, 0, gpu_device)
            bufs.append(buf)
            for rep in range(2):
                res_a, ris_a = _enqueue(on, buf.ptr, n, depth, stride)
                res_b, ris_b = _enqueue(off, buf.ptr, n, depth, stride)
                assert [bytes(r) for r in res_a] == [bytes(r) for r in res_b], (depth, rep)
                assert [bytes(r) for r in ris_a] == [bytes(r) for r in ris_b], (depth, rep)
                mom = on.fetch_riser_moments(n)
                assert sum(int(m.s[k].m.n) for m in mom for k in range(m.n_surfaces)) > 2 * SUPPORT
                with pytest.raises(ssd.SsdError, match="gathered none"):
                    off.fetch_riser_moments(n)
        # off again: the next pass gathers none, results and risers stay what they were
        on.set_riser_moments(False)
        res_a, ris_a = _enqueue(on, bufs[-1].ptr, n, True, stride)
        assert [bytes(r) for r in res_a] == [bytes(r) for r in res_b] and [bytes(r) for r in ris_a] == [bytes(r) for r in ris_b]
        with pytest.raises(ssd.SsdError, match="gathered none"):
            on.fetch_riser_moments(n)
    finally:
        for b in bufs:
            b.free()
        on.close()
        off.close()


@pytest.mark.gpu
def test_the_host_path_covers_every_slice(ssd, gpu_device):
    """70 frames of 256 x 192 through ssd_process_host_riser_fits: three slices.  Every frame's moments equal those of a one-frame
    enqueue, every fit is ssd_riser_fit_solve of them, the previous setting is restored, and n + 1 frames are refused."""
    W, H, scs3 = _scenes(ssd, "256x192")
    n = 70
    scs = [scs3[i % len(scs3)] for i in range(n)]
    trans = ssd.transformation_for_scene(scs3[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=32)
    unique = ssd.synth_host(scs3)
    xyz = np.stack([unique[i % len(scs3)] for i in range(n)])
    det = _detector(ssd, cfg, trans, gpu_device, False)
    buf = ssd.DeviceBuffer(unique[0].nbytes, gpu_device)
    try:
        res, ris, fits, mom = det.process_host_riser_fits(xyz, min_points=rm.MIN_POINTS, moments=True)
        assert len(res) == len(ris) == len(fits) == len(mom) == n
        assert [bytes(r) for r in det.fetch_risers(n)] == [bytes(r) for r in ris]
        assert [bytes(m) for m in det.fetch_riser_moments(n)] == [bytes(m) for m in mom], "the whole batch of the last host call"
        with pytest.raises(ssd.SsdError, match="exceeds"):
            det.fetch_riser_moments(n + 1)
        res2, ris2, fits2 = det.process_host_riser_fits(xyz, min_points=rm.MIN_POINTS)              # without the moments
        assert [bytes(f) for f in fits2] == [bytes(f) for f in fits] and [bytes(r) for r in ris2] == [bytes(r) for r in ris]
        # the setting before the call (off) is back: a plain host call gathers none
        det.process_host(xyz[:2])
        with pytest.raises(ssd.SsdError, match="gathered none"):
            det.fetch_riser_moments(2)
        # each frame alone, through a one-frame enqueue
        det.set_riser_moments(True)
        alone = []
        for j in range(len(scs3)):
            buf.upload(np.ascontiguousarray(unique[j]))
            r1, s1 = _enqueue(det, buf.ptr, 1, False, None)
            alone.append((bytes(r1[0]), bytes(s1[0]), det.fetch_riser_moments(1)[0]))
        for i in range(n):
            r1, s1, m1 = alone[i % len(scs3)]
            assert bytes(res[i]) == r1 and bytes(ris[i]) == s1 and bytes(mom[i]) == bytes(m1), "frame %d" % i
            assert bytes(fits[i]) == bytes(ssd.riser_fit_solve(mom[i], ris[i], trans, rm.MIN_POINTS)), "frame %d: the fit" % i
        assert any(f.r[k].status == ssd.GF_OK and f.r[k].going > 0.1 for f in fits for k in range(f.n_risers)), "a going is measured"
        assert bytes(mom[len(scs3) - 1]) == ZERO and fits[len(scs3) - 1].n_risers == 0
    finally:
        buf.free()
        det.close()


# three mountings that differ in pitch, roll and height; for depth input the first two also differ in optics and depth units
POSES = [dict(pitch_deg=50.0, roll_deg=25.0, cam_height=1.0), dict(pitch_deg=46.0, roll_deg=-20.0, cam_height=0.92),
         dict(pitch_deg=52.0, roll_deg=18.0, cam_height=1.06)]
OPTICS = [dict(hfov_deg=70.0), dict(hfov_deg=62.0)]
UNITS = [0.00025, 0.0001]


def _alone(ssd, cfg, trans, intr, frame, device):
    """the frame through a one-camera handle alone -> bytes of (result, risers, riser moments)"""
    det = _detector(ssd, cfg, trans, device, True, intr)
    buf = ssd.DeviceBuffer(frame.nbytes, device)
    try:
        buf.upload(np.ascontiguousarray(frame))
        res, ris = _enqueue(det, buf.ptr, 1, intr is not None, None)
        return bytes(res[0]), bytes(ris[0]), bytes(det.fetch_riser_moments(1)[0])
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
def test_camera_batches_equal_the_one_camera_handles(ssd, gpu_device):
    """three cameras whose calibrations differ, six frames: each frame's riser moments (and result and risers) are byte for byte those
    of a handle created with that frame's camera, for vertices from all three and for 16-bit depth from the two with intrinsics; the
    host entry point solves each frame under its own camera.  The handle's own calibration is the identity: a fall-back to it would be
    wrong everywhere."""
    W, H = 256, 192
    cfg = ssd.default_config(W, H, max_frames_per_batch=8)
    det = ssd.Detector(cfg, ssd.GeometricTransformation(), gpu_device)
    det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
    det.set_riser_moments(True)
    bufs = []
    try:
        for depth, order in ((False, [2, 0, 1, 2, 0, 1]), (True, [1, 0, 0, 1, 1, 0])):
            ncam = 2 if depth else 3
            scs = [ssd.make_scene(W, H, n_steps=3, seed=11 + j, sigma=0.001 + 0.0005 * j, **POSES[j], **(OPTICS[j] if depth else {})) for j in range(ncam)]
            trans = [ssd.transformation_for_scene(sc) for sc in scs]
            intr = [ssd.intrinsics_for_scene(sc, depth_units=u) for sc, u in zip(scs, UNITS)] if depth else [None] * ncam
            frames = [ssd.synth_depth_host([sc], depth_units=u)[0] for sc, u in zip(scs, UNITS)] if depth else list(ssd.synth_host(scs))
            alone = [_alone(ssd, cfg, trans[j], intr[j], frames[j], gpu_device) for j in range(ncam)]
            assert len(set(a[2] for a in alone)) == ncam, "as many different records as cameras"
            assert all(ssd.FrameMoments.from_buffer_copy(a[2]).n_surfaces >= 2 for a in alone)
            # the table: the cameras in use, then (depth: a camera without intrinsics) one nobody names
            table = ([(t, i) for t, i in zip(trans, intr)] if depth else trans) + [ssd.GeometricTransformation()]
            det.set_cameras(table)
            n = len(order)
            buf, stride = _upload(ssd, [frames[j] for j in order], 8 if depth else 4, gpu_device)
            bufs.append(buf)
            det.enqueue_cameras(buf.ptr, n, order, depth=depth, stride_bytes=stride)
            res, ris, mom = det.fetch_list(n), det.fetch_risers(n), det.fetch_riser_moments(n)
            for i, j in enumerate(order):
                assert (bytes(res[i]), bytes(ris[i])) == alone[j][:2], "frame %d (camera %d): result / risers" % (i, j)
                assert bytes(mom[i]) == alone[j][2], "frame %d (camera %d): not the one-camera handle's riser moments" % (i, j)
            host = np.stack([frames[j] for j in order])
            res_h, ris_h, fits_h, mom_h = det.process_host_cameras_riser_fits(host, order, depth=depth, min_points=rm.MIN_POINTS, moments=True)
            assert [bytes(m) for m in mom_h] == [bytes(m) for m in mom] and [bytes(r) for r in ris_h] == [bytes(r) for r in ris]
            for i, j in enumerate(order):
                assert bytes(fits_h[i]) == bytes(ssd.riser_fit_solve(mom[i], ris[i], trans[j], rm.MIN_POINTS)), "frame %d under camera %d" % (i, j)
            assert any(f.r[k].status == ssd.GF_OK for f in fits_h for k in range(f.n_risers))
    finally:
        for b in bufs:
            b.free()
        det.close()


@pytest.mark.gpu
def test_contract_errors_and_idleness(ssd, gpu_device):
    """fetching before any pass, the host entry point with risers off, and a handle that never enables the moments holding nothing for
    them: of two fresh handles the one that enables and disables the moments reports more workspace bytes, by the two buffers' size"""
    W, H, scs = _scenes(ssd, "256x192")
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=4)
    xyz = ssd.synth_host(scs[:1])
    plain, det = ssd.Detector(cfg, trans, gpu_device), ssd.Detector(cfg, trans, gpu_device)
    try:
        assert det.workspace_bytes == plain.workspace_bytes
        with pytest.raises(ssd.SsdError, match="gathered none"):
            det.fetch_riser_moments(1)
        with pytest.raises(ssd.SsdError, match="ssd_set_risers"):
            det.process_host_riser_fits(xyz)
        assert det.workspace_bytes == plain.workspace_bytes, "a refused call allocates nothing"
        # legal while risers are off; takes effect when they come on
        det.set_riser_moments(True)
        grown = det.workspace_bytes
        assert grown == plain.workspace_bytes + 4 * C.sizeof(ssd.FrameMoments)
        det.process_host(xyz)
        with pytest.raises(ssd.SsdError, match="gathered none"):
            det.fetch_riser_moments(1)
        det.set_riser_moments(False)
        assert det.workspace_bytes == grown > plain.workspace_bytes
        plain.set_risers(True, tolerance=TOL, min_support=SUPPORT)
        det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
        assert det.workspace_bytes - plain.workspace_bytes == 4 * C.sizeof(ssd.FrameMoments)
        det.set_riser_moments(True)
        res = det.process_host(xyz)
        mom = det.fetch_riser_moments(1)[0]
        assert mom.n_surfaces == res[0].n_steps - 1 >= 2 and mom.s[0].m.n >= SUPPORT
    finally:
        plain.close()
        det.close()
