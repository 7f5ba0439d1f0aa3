"""Surface moments of cameras batches on the GPU (k_surface_moments_cams; include/ssd_hip.h).  The contract under
test is section 7b's, extended: frame i's ssd_frame_moments is, byte for byte, what a handle created with that frame's camera returns
for the frame alone - and the host sums over the labels the same batch returns.  The handle's own calibration is the identity, so a
fall-back to it would be wrong everywhere."""
import ctypes as C

import numpy as np
import pytest

import surface_model as sm
import test_gpu_prefilter_regimes as regimes
from test_cameras import scene_set

ORDER = [2, 0, 3, 1, 2, 0]                 # frame -> camera: not monotonic, cameras repeated
F = 8
# four mountings that differ in pitch, roll and height; rolled, so that camera rows cross from one surface to the next
POSES = [dict(pitch_deg=50.0, roll_deg=25.0, cam_height=1.0), dict(pitch_deg=46.0, roll_deg=-20.0, cam_height=0.92),
         dict(pitch_deg=52.0, roll_deg=18.0, cam_height=1.06), dict(pitch_deg=48.0, roll_deg=28.0, cam_height=0.97)]
# depth input: the cameras differ in field of view and depth units as well
OPTICS = [dict(hfov_deg=70.0), dict(hfov_deg=62.0), dict(hfov_deg=66.0, vfov_deg=52.0), dict(hfov_deg=74.0)]
UNITS = [0.00025, 0.0001, 0.0002, 0.00025]
SHAPES = {"256x192": (256, 192, False), "250x190": (250, 190, False), "256x192-depth16": (256, 192, True)}
REC = None


def _records(ssd, raw, n):
    return list((ssd.FrameMoments * n).from_buffer_copy(np.ascontiguousarray(raw).tobytes()))


def _upload(ssd, frames, pad, device):
    """frames at a stride of their size + pad -> (buffer, stride)"""
    stride = frames[0].nbytes + pad
    buf = ssd.DeviceBuffer(stride * len(frames), device)
    for i, f in enumerate(frames):
        buf.upload(np.ascontiguousarray(f), offset=i * stride)
    return buf, stride


def _alone(ssd, cfg, cam, frame, depth, device):
    """the frame through a one-camera handle alone -> bytes of (result, FrameMoments)"""
    trans, intr = cam if isinstance(cam, tuple) else (cam, None)
    det = ssd.Detector(cfg, trans, device)
    buf = ssd.DeviceBuffer(frame.nbytes, device)
    out = ssd.DeviceBuffer(C.sizeof(ssd.FrameMoments), device)
    try:
        if depth:
            det.set_intrinsics(intr)
        buf.upload(np.ascontiguousarray(frame))
        det.enqueue_surface_moments(buf.ptr, 1, out.ptr, depth=depth)
        res = bytes(det.fetch_list(1)[0])
        return res, out.download(C.sizeof(ssd.FrameMoments)).tobytes()
    finally:
        buf.free()
        out.free()
        det.close()


def _identity_detector(ssd, cfg, device):
    return ssd.Detector(cfg, ssd.GeometricTransformation(), device)


def _host_sums(ssd, cfg, frame, lab, res, dbg, intr=None):
    live = not (res.status & ssd.ST_THROW) and res.n_steps > 0
    return ssd.surface_moments_host(cfg, frame, lab, res.n_steps if live else 0, 1 if live and dbg.ground_ind >= 0 else 0, intr=intr)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_mixed_poses_equal_the_one_camera_handles_and_the_host_sums(ssd, gpu_device, shape):
    W, H, depth = SHAPES[shape]
    wh, n, rec = W * H, len(ORDER), C.sizeof(ssd.FrameMoments)
    scs = [ssd.make_scene(W, H, n_steps=3, seed=11 + j, sigma=0.001 + 0.0005 * j, **POSES[j], **(OPTICS[j] if depth else {})) for j in range(4)]
    trans = [ssd.transformation_for_scene(sc) for sc in scs]
    intr = [ssd.intrinsics_for_scene(sc, depth_units=u) for sc, u in zip(scs, UNITS)] if depth else [None] * 4
    frames = [ssd.synth_depth_host([sc], depth_units=u)[0] for sc, u in zip(scs, UNITS)] if depth else list(ssd.synth_host(scs))
    table = [(t, i) for t, i in zip(trans, intr)] if depth else trans
    cfg = ssd.default_config(W, H, max_frames_per_batch=F)
    alone = [_alone(ssd, cfg, table[j], frames[j], depth, gpu_device) for j in range(4)]
    assert len(set(a[1] for a in alone)) == 4, "four cameras, four different records"
    det = _identity_detector(ssd, cfg, gpu_device)
    buf, stride = _upload(ssd, [frames[j] for j in ORDER], 8 if depth else 4, gpu_device)
    out = ssd.DeviceBuffer(rec * (n + 1), gpu_device)
    lbuf = ssd.DeviceBuffer(wh * n, gpu_device)
    try:
        assert stride % 16 != 0
        det.set_cameras(table + [ssd.GeometricTransformation()])               # the last: a camera nobody uses
        out.upload(np.full(rec * (n + 1), 0xA5, dtype=np.uint8))                # the call zeroes its records itself
        det.set_debug(True, images=False)
        det.enqueue_cameras_surface_moments(buf.ptr, n, ORDER, out.ptr, depth=depth, stride_bytes=stride)
        res = det.fetch_list(n)
        raw = out.download(rec * (n + 1))
        got = _records(ssd, raw[:rec * n], n)
        dbg = [det.debug(i) for i in range(n)]
        assert np.all(raw[rec * n:] == 0xA5), "a record past nframes was written"
        # a plain cameras batch of the same frames: the same results, and the labels the sums are taken over
        det.enqueue_cameras(buf.ptr, n, ORDER, depth=depth, d_labels=lbuf.ptr, stride_bytes=stride)
        plain = det.fetch_list(n)
        lab = lbuf.download(wh * n).reshape(n, wh)
        det.set_debug(False)
        two = 0
        for i, j in enumerate(ORDER):
            assert bytes(res[i]) == alone[j][0] == bytes(plain[i]), "frame %d (camera %d): result" % (i, j)
            assert bytes(got[i]) == alone[j][1], "frame %d (camera %d): not the one-camera handle's record" % (i, j)
            want = _host_sums(ssd, cfg, frames[j], lab[i], res[i], dbg[i], intr[j])
            assert sm.frame_tuple(got[i]) == sm.frame_tuple(want) and bytes(got[i]) == bytes(want), "frame %d: the host sums" % i
            assert got[i].n_surfaces == res[i].n_steps >= 2 and got[i].ground == 1, (i, got[i].n_surfaces)
            d = dbg[i]
            valid = [k for k in range(d.first_valid_ind, d.n_plateaus) if d.plateaus[k].valid]
            for s in range(res[i].n_steps):
                cnt = int(got[i].s[s].m.n + got[i].s[s].n_far)
                assert cnt == (d.ground_n_in_quad if s == 0 else d.plateaus[valid[s - 1]].n_in_quad) > 0, (i, s)
            cells = lab[i, :wh // 64 * 64].reshape(-1, 64)
            top, low = cells.max(axis=1), np.where(cells > 0, cells, 255).min(axis=1)
            two += int(((top > 0) & (low < top)).sum())
        assert two > 0, "no 64-point cell carries two surfaces"
        assert max(g.n_surfaces for g in got) >= 3, "a frame with at least three surfaces"
    finally:
        buf.free()
        out.free()
        lbuf.free()
        det.close()


def _regime_table(ssd, oracle):
    """test_gpu_cameras.test_mixed_prefilter_regimes_in_one_batch's table: the common regime, one that needs CHECKS, one all doubles"""
    w, h, scs = scene_set(ssd, "vga")
    cases = [regimes.build_case(ssd, oracle, "B-km-aligned-640"), regimes.build_case(ssd, oracle, "C-xy-aligned-640")]
    table = [ssd.transformation_for_scene(scs[0]), cases[0]["trans"], cases[1]["trans"]]
    frames = [ssd.synth_host([scs[0]])[0]] + [np.asarray(c["frame"], dtype=np.float32).reshape(h, w, 3) for c in cases]
    return w, h, table, frames


@pytest.mark.gpu
def test_both_checks_instantiations(ssd, oracle, gpu_device):
    """a table of the common regime alone runs CHECKS = false; with a camera that needs the rare configurations' tests the whole batch
    runs CHECKS = true: every frame's record is its one-camera handle's either way"""
    w, h, table, frames = _regime_table(ssd, oracle)
    cfg = ssd.default_config(w, h, max_frames_per_batch=F)
    rec = C.sizeof(ssd.FrameMoments)
    alone = [_alone(ssd, cfg, t, f, False, gpu_device) for t, f in zip(table, frames)]
    det = _identity_detector(ssd, cfg, gpu_device)
    out = ssd.DeviceBuffer(rec * 4, gpu_device)
    bufs = []
    try:
        for tab, order in ((table[:1], [0, 0]), (table, [0, 1, 0, 2]), (table, [2, 0, 1, 0])):
            det.set_cameras(tab)
            buf, stride = _upload(ssd, [frames[j] for j in order], 0, gpu_device)
            bufs.append(buf)
            det.enqueue_cameras_surface_moments(buf.ptr, len(order), order, out.ptr)
            res = det.fetch_list(len(order))
            got = _records(ssd, out.download(rec * len(order)), len(order))
            for i, j in enumerate(order):
                assert bytes(res[i]) == alone[j][0] and bytes(got[i]) == alone[j][1], (order, i, j)
        assert all(ssd.FrameMoments.from_buffer_copy(a[1]).n_surfaces >= 2 for a in alone[:1])
    finally:
        for b in bufs:
            b.free()
        out.free()
        det.close()


def _vga(ssd, device):
    """the smallest scene set of tests/scenes.py (640 x 480, four cameras) and each frame's one-camera bytes, once per session"""
    global REC
    if REC is None:
        w, h, scs = scene_set(ssd, "vga")
        trans = [ssd.transformation_for_scene(sc) for sc in scs]
        frames = ssd.synth_host(scs)
        cfg = ssd.default_config(w, h, max_frames_per_batch=F)
        REC = dict(w=w, h=h, trans=trans, frames=frames, cfg=cfg, alone=[_alone(ssd, cfg, t, f, False, device) for t, f in zip(trans, frames)])
    return REC


@pytest.mark.gpu
def test_three_workspaces_and_the_index_is_copied_during_the_call(ssd, gpu_device):
    d = _vga(ssd, gpu_device)
    rec = C.sizeof(ssd.FrameMoments)
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=F, batches_in_flight=3)
    det = _identity_detector(ssd, cfg, gpu_device)
    buf, stride = _upload(ssd, list(d["frames"]), 0, gpu_device)              # frames 0 .. 3 in scene order
    out = ssd.DeviceBuffer(rec * 12, gpu_device)
    try:
        det.set_cameras(d["trans"])
        assert det.batches_in_flight == 3
        # three batches in flight, each into records of its own: all four frames, then the last two, then the first three
        parts = [(0, 4), (2, 2), (0, 3)]
        host = np.zeros(4, dtype=np.uint16)
        L = ssd.lib()
        for b, (at, m) in enumerate(parts):
            host[:m] = range(at, at + m)
            assert L.ssd_enqueue_cameras_surface_moments(det._h, C.c_void_p(buf.ptr + at * stride), stride, m, None, host.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                         ssd.INPUT_VERTICES, C.c_void_p(out.ptr + 4 * b * rec)) == 0
            host[:] = 0xFFFF                                                   # garbage as soon as the call has returned
        res = (ssd.FrameResult * 4)()
        for back, b in ((2, 0), (1, 1), (0, 2)):
            at, m = parts[b]
            assert L.ssd_fetch_back(det._h, res, m, back) == 0
            assert [bytes(res[k]) for k in range(m)] == [d["alone"][at + k][0] for k in range(m)], b
            got = out.download(rec * m, offset=4 * b * rec).tobytes()
            assert got == b"".join(d["alone"][at + k][1] for k in range(m)), b
        # the first batch's records are intact after the later ones
        assert out.download(rec * 4).tobytes() == b"".join(a[1] for a in d["alone"])
    finally:
        buf.free()
        out.free()
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_host_path_over_two_slice_boundaries_and_the_drift_of_its_moments(ssd, gpu_device, lanes):
    d = _vga(ssd, gpu_device)
    n = 70
    which = [(3 * k + k // 7) % 4 for k in range(n)]                           # the frame and its camera: changes across frames 32 and 64
    assert which[31] != which[32] and which[63] != which[64]
    frames = np.ascontiguousarray(np.stack([d["frames"][j] for j in which]), dtype=np.float32)
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=64, batches_in_flight=lanes)
    det = _identity_detector(ssd, cfg, gpu_device)
    try:
        det.set_cameras(d["trans"])
        res, fits, mom = det.process_host_cameras_surfaces(frames, which, min_points=sm.MIN_POINTS, moments=True)
        for k in range(n):
            assert bytes(res[k]) == d["alone"][which[k]][0] and bytes(mom[k]) == d["alone"][which[k]][1], k
        want_fits = [bytes(ssd.surface_fit_solve(ssd.FrameMoments.from_buffer_copy(a[1]), t, sm.MIN_POINTS)) for a, t in zip(d["alone"], d["trans"])]
        assert [bytes(f) for f in fits] == [want_fits[j] for j in which]
        assert any(f.s[k].status == ssd.GF_OK for f in fits for k in range(f.n_surfaces))
        res_n, fits_n = det.process_host_cameras_surfaces(frames, which, min_points=sm.MIN_POINTS)        # without the moments
        assert [bytes(f) for f in fits_n] == [bytes(f) for f in fits] and [bytes(r) for r in res_n] == [bytes(r) for r in res]
        res_d, drift = det.camera_drift(frames, which)
        want = ssd.camera_drift_fold(mom, which, d["trans"])
        assert [bytes(r) for r in res_d] == [bytes(r) for r in res]
        assert [bytes(x) for x in drift] == [bytes(x) for x in want] and len(drift) == 4
        assert [x.frames for x in drift] == [which.count(j) for j in range(4)] and all(x.frames_left == 0 for x in drift)
        assert sum(x.frames_ground for x in drift) > 0
    finally:
        det.close()


@pytest.mark.gpu
def test_the_contract(ssd, gpu_device):
    """the refusals, each before anything is launched: a following valid call gives the right bytes; records past nframes; the time"""
    d = _vga(ssd, gpu_device)
    rec = C.sizeof(ssd.FrameMoments)
    w, h = 256, 192
    scs = [ssd.make_scene(w, h, n_steps=3, seed=11 + j, **POSES[j]) for j in range(2)]
    trans = [ssd.transformation_for_scene(sc) for sc in scs]
    intr = ssd.intrinsics_for_scene(scs[0])
    depth = [ssd.synth_depth_host([sc])[0] for sc in scs]
    cfgd = ssd.default_config(w, h, max_frames_per_batch=F)
    det = _identity_detector(ssd, d["cfg"], gpu_device)
    detd = _identity_detector(ssd, cfgd, gpu_device)
    buf, stride = _upload(ssd, list(d["frames"]), 0, gpu_device)
    dbuf, dstride = _upload(ssd, depth, 0, gpu_device)
    out = ssd.DeviceBuffer(rec * 4, gpu_device)
    L = ssd.lib()
    idx = (C.c_uint16 * 4)(0, 1, 2, 3)
    want = b"".join(a[1] for a in d["alone"])

    def good(m=4):
        out.upload(np.full(rec * 4, 0xA5, dtype=np.uint8))
        det.enqueue_cameras_surface_moments(buf.ptr, m, list(range(m)), out.ptr)
        res = det.fetch_list(m)
        assert [bytes(r) for r in res] == [a[0] for a in d["alone"][:m]]
        raw = out.download(rec * 4).tobytes()
        assert raw[:rec * m] == want[:rec * m] and raw[rec * m:] == b"\xa5" * (rec * (4 - m)), "records past nframes are untouched"

    try:
        base = det.workspace_bytes
        with pytest.raises(ssd.SsdError, match="no camera table"):
            det.enqueue_cameras_surface_moments(buf.ptr, 4, [0, 1, 2, 3], out.ptr)
        det.set_cameras(d["trans"])
        with_table = det.workspace_bytes
        good()
        assert det.workspace_bytes == with_table > base, "the pass allocates nothing"
        assert L.ssd_enqueue_cameras_surface_moments(det._h, C.c_void_p(buf.ptr), stride, 4, None, idx, ssd.INPUT_VERTICES, None) == -1
        assert b"null" in L.ssd_last_error()
        good(3)
        with pytest.raises(ssd.SsdError, match="names camera 4 of 4"):
            det.enqueue_cameras_surface_moments(buf.ptr, 4, [0, 1, 4, 3], out.ptr)
        good()
        assert L.ssd_enqueue_cameras_surface_moments(det._h, C.c_void_p(buf.ptr), stride, 4, None, None, ssd.INPUT_VERTICES, C.c_void_p(out.ptr)) == -1
        assert L.ssd_enqueue_cameras_surface_moments(det._h, C.c_void_p(buf.ptr), stride, 4, None, idx, 2, C.c_void_p(out.ptr)) == -1
        assert L.ssd_enqueue_cameras_surface_moments(det._h, C.c_void_p(buf.ptr), stride, F + 1, None, idx, ssd.INPUT_VERTICES, C.c_void_p(out.ptr)) == -1
        good()
        # depth input naming a camera without intrinsics
        detd.set_cameras([(trans[0], intr), trans[1]])
        alone0 = _alone(ssd, cfgd, (trans[0], intr), depth[0], True, gpu_device)
        with pytest.raises(ssd.SsdError, match="intrinsics"):
            detd.enqueue_cameras_surface_moments(dbuf.ptr, 2, [0, 1], out.ptr, depth=True)
        out.upload(np.full(rec * 4, 0xA5, dtype=np.uint8))
        detd.enqueue_cameras_surface_moments(dbuf.ptr, 1, [0], out.ptr, depth=True)
        assert bytes(detd.fetch_list(1)[0]) == alone0[0]
        raw = out.download(rec * 2).tobytes()
        assert raw[:rec] == alone0[1] and raw[rec:] == b"\xa5" * rec
        # the pass's time of a timed cameras enqueue; 0 for one that gathers none
        det.set_timing(True)
        det.enqueue_cameras_surface_moments(buf.ptr, 4, [0, 1, 2, 3], out.ptr)
        det.fetch(4)
        assert det.surface_moments_time_ms(0) > 0.0
        det.enqueue_cameras(buf.ptr, 4, [0, 1, 2, 3])
        det.fetch(4)
        assert det.surface_moments_time_ms(0) == 0.0
    finally:
        buf.free()
        dbuf.free()
        out.free()
        det.close()
        detd.close()
