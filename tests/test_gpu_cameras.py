"""Per-frame calibration on the GPU (ssd_set_cameras / ssd_enqueue_cameras / ssd_process_host_cameras; include/ssd_hip.h, DESIGN.md
section 7b).  The contract under test: frame i of a cameras batch gives, byte for byte, what a handle created with that frame's camera
gives for the frame alone - result, debug record, labels, risers - on two passes and on the single pass, with one workspace and
with several.  Shapes: 640 x 480 (the strips walk of k_hist_planes) and 1024 x 768 (its tile loop), batches of 4 - 8 frames, 40
where the host path's 32-frame slice boundary is the point."""
import numpy as np
import pytest

import oracle_binding as ob
import parity
import test_gpu_prefilter_regimes as regimes
from test_cameras import SETS, scene_set

F = 8                                    # max_frames_per_batch of the handles here
ORDER = [2, 0, 3, 1, 2, 0]                 # frame -> camera: not monotonic, cameras repeated
_cache = {}


def _set(ssd, oracle, key):
    """the scene set once per session: frames, transformations, the oracle's full record per frame under its own camera, and the
    bytes a one-camera handle returns for each frame alone (result, labels, risers)"""
    if key in _cache:
        return _cache[key]
    w, h, scs = scene_set(ssd, key)
    trans = [ssd.transformation_for_scene(sc) for sc in scs]
    frames = ssd.synth_host(scs)
    cfg = ssd.default_config(w, h, max_frames_per_batch=F)
    ocfg = ob.to_oracle_config(cfg)
    ores = [oracle.process(ocfg, ob.to_oracle_calibration(t.constants), f)[0] for t, f in zip(trans, frames)]
    d = dict(w=w, h=h, scenes=scs, trans=trans, frames=frames, cfg=cfg, ores=ores, alone=None)
    _cache[key] = d
    return d


def _alone(ssd, d, device):
    """frame j through Detector(cfg, trans[j]) alone: bytes of the result, labels, risers (risers on: results do not depend on it)"""
    if d["alone"] is None:
        out = []
        wh = d["w"] * d["h"]
        for t, f in zip(d["trans"], d["frames"]):
            det = ssd.Detector(d["cfg"], t, device)
            buf, lbuf = ssd.DeviceBuffer(wh * 12, device), ssd.DeviceBuffer(wh, device)
            try:
                det.set_risers(True)
                buf.upload(f)
                det.enqueue_labels(buf.ptr, 1, lbuf.ptr)
                res = bytes(det.fetch_list(1)[0])
                out.append((res, lbuf.download(wh).tobytes(), bytes(det.fetch_risers(1)[0])))
            finally:
                buf.free()
                lbuf.free()
                det.close()
        d["alone"] = out
    return d["alone"]


def _upload(ssd, frames, device, dtype=np.float32):
    a = np.ascontiguousarray(np.stack(frames), dtype=dtype)
    buf = ssd.DeviceBuffer(a.nbytes, device)
    buf.upload(a)
    return buf


def _identity_detector(ssd, cfg, device):
    """the handle's OWN calibration is none of the cameras': a batch that fell back to it would be wrong everywhere"""
    return ssd.Detector(cfg, ssd.GeometricTransformation(), device)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("key", ["vga", "xga"])
def test_mixed_poses_every_intermediate(ssd, oracle, gpu_device, key, mode):
    d = _set(ssd, oracle, key)
    alone = _alone(ssd, d, gpu_device)
    det = _identity_detector(ssd, d["cfg"], gpu_device)
    buf = _upload(ssd, [d["frames"][j] for j in ORDER], gpu_device)
    try:
        det.set_cameras(d["trans"] + [ssd.GeometricTransformation()])          # the last: a camera nobody uses
        assert det.camera_count == len(d["trans"]) + 1
        det.single_pass(mode)
        det.set_debug(True, images=False)
        det.enqueue_cameras(buf.ptr, len(ORDER), ORDER)
        res = det.fetch_list(len(ORDER))
        report = {}
        for i, j in enumerate(ORDER):
            try:
                parity.compare_debug(det.debug(i), d["ores"][j], report)
                parity.compare_result(ssd, res[i], d["ores"][j], report)
            except parity.Mismatch as e:
                raise parity.Mismatch("frame %d (camera %d, %s): %s" % (i, j, SETS[key][2][j], e))
            assert bytes(res[i]) == alone[j][0], "frame %d: not the one-camera handle's result" % i
            assert d["ores"][j].n_steps >= 2
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
def test_depth16_cameras_differ_in_pose_fov_and_depth_units(ssd, oracle, gpu_device):
    w, h = 640, 480
    kw = [dict(n_steps=3, sigma=0.002, seed=2), dict(n_steps=3, sigma=0.001, seed=31, hfov_deg=60.0, pitch_deg=44.0, cam_height=0.9),
          dict(n_steps=4, sigma=0.003, seed=17, yaw_deg=6.0, rise=0.15, tread=0.26)]
    units = [0.00025, 0.0001, 0.00025]
    scs = [ssd.make_scene(w, h, **k) for k in kw]
    trans = [ssd.transformation_for_scene(sc) for sc in scs]
    intr = [ssd.intrinsics_for_scene(sc, depth_units=u) for sc, u in zip(scs, units)]
    depth = [ssd.synth_depth_host([sc], depth_units=u)[0] for sc, u in zip(scs, units)]
    cfg = ssd.default_config(w, h, max_frames_per_batch=F)
    order = [1, 0, 2, 1, 0]
    alone = []
    for t, i, f in zip(trans, intr, depth):
        one = ssd.Detector(cfg, t, gpu_device)
        try:
            one.set_intrinsics(i)
            alone.append(bytes(one.process_depth_host(f)[0]))
        finally:
            one.close()
    assert len(set(alone)) == 3
    det = _identity_detector(ssd, cfg, gpu_device)
    buf = _upload(ssd, [depth[j] for j in order], gpu_device, np.uint16)
    try:
        det.set_cameras([(t, i) for t, i in zip(trans, intr)] + [trans[0]])       # camera 3: no intrinsics
        for mode in (0, 1):
            det.single_pass(mode)
            det.enqueue_cameras(buf.ptr, len(order), order, depth=True)
            res = det.fetch_list(len(order))
            for k, j in enumerate(order):
                assert bytes(res[k]) == alone[j], (mode, k, j)
                assert res[k].n_steps >= 2
        with pytest.raises(ssd.SsdError, match="intrinsics"):
            det.enqueue_cameras(buf.ptr, len(order), [1, 0, 3, 1, 0], depth=True)
        det.enqueue_cameras(buf.ptr, len(order), order, depth=True)          # and the handle still works
        assert bytes(det.fetch_list(len(order))[0]) == alone[order[0]]
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
def test_labels_and_risers_equal_the_one_camera_handles(ssd, oracle, gpu_device):
    d = _set(ssd, oracle, "vga")
    alone = _alone(ssd, d, gpu_device)
    wh, pad, n = d["w"] * d["h"], 64, len(ORDER)
    det = _identity_detector(ssd, d["cfg"], gpu_device)
    buf = _upload(ssd, [d["frames"][j] for j in ORDER], gpu_device)
    lbuf = ssd.DeviceBuffer((wh + pad) * n, gpu_device)
    try:
        det.set_cameras(d["trans"])
        det.set_risers(True)
        lbuf.upload(np.full((wh + pad) * n, 0xA5, dtype=np.uint8))
        det.enqueue_cameras(buf.ptr, n, ORDER, d_labels=lbuf.ptr, label_stride=wh + pad)
        res = det.fetch_list(n)
        risers = det.fetch_risers(n)
        raw = lbuf.download((wh + pad) * n).reshape(n, wh + pad)
        assert np.all(raw[:, wh:] == 0xA5), "the padding of a label stride was written"
        for i, j in enumerate(ORDER):
            assert bytes(res[i]) == alone[j][0], i
            assert raw[i, :wh].tobytes() == alone[j][1], "labels of frame %d" % i
            assert bytes(risers[i]) == alone[j][2], "risers of frame %d" % i
        assert any(np.any(raw[i, :wh] > 1) for i in range(n)) and any(r.n_risers > 0 for r in risers)
    finally:
        buf.free()
        lbuf.free()
        det.close()


@pytest.mark.gpu
def test_mixed_prefilter_regimes_in_one_batch(ssd, oracle, gpu_device):
    """One table: a camera of the common regime, one that needs CHECKS (B-km: inputs beyond max_input in range) and one whose x / y
    test is all doubles (C-xy).  The batch runs the CHECKS instantiations; every frame's record is the oracle's even so."""
    d = _set(ssd, oracle, "vga")
    cases = [regimes.build_case(ssd, oracle, "B-km-aligned-640"), regimes.build_case(ssd, oracle, "C-xy-aligned-640")]
    cfg = d["cfg"]
    for c in cases:
        assert all(getattr(c["cfg"], f) == getattr(cfg, f) for f, _ in ssd.Config._fields_ if f != "max_frames_per_batch"), "the default configuration"
        assert c["src"] == "aligned"
    table = [d["trans"][0], cases[0]["trans"], cases[1]["trans"]]
    frames = [d["frames"][0], cases[0]["frame"], cases[1]["frame"]]
    ores = [d["ores"][0], cases[0]["res"], cases[1]["res"]]
    det = _identity_detector(ssd, cfg, gpu_device)
    try:
        det.set_cameras(table)
        det.set_debug(True, images=False)
        for order in ([0, 1, 0, 2], [2, 0, 1, 0]):
            buf = _upload(ssd, [np.asarray(frames[j]).reshape(480, 640, 3) for j in order], gpu_device)
            try:
                for mode in (0, 1):
                    det.single_pass(mode)
                    det.enqueue_cameras(buf.ptr, len(order), order)
                    res = det.fetch_list(len(order))
                    for i, j in enumerate(order):
                        try:
                            parity.compare_debug(det.debug(i), ores[j], {})
                            parity.compare_result(ssd, res[i], ores[j], {})
                        except parity.Mismatch as e:
                            raise parity.Mismatch("order %r mode %d frame %d (camera %d): %s" % (order, mode, i, j, e))
            finally:
                buf.free()
    finally:
        det.close()


@pytest.mark.gpu
def test_several_workspaces_and_the_index_is_copied_during_the_call(ssd, oracle, gpu_device):
    d = _set(ssd, oracle, "vga")
    alone = _alone(ssd, d, gpu_device)
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=F, batches_in_flight=3)
    det = _identity_detector(ssd, cfg, gpu_device)
    buf = _upload(ssd, d["frames"], gpu_device)                            # frames 0 .. 3 in scene order
    try:
        det.set_cameras(d["trans"])
        assert det.batches_in_flight == 3
        # the SAME frames under three indices: only index 0 names every frame's own camera
        indices = [[0, 1, 2, 3], [1, 1, 2, 3], [0, 1, 2, 0]]
        host = np.zeros(4, dtype=np.uint16)
        for idx in indices:
            host[:] = idx
            det.enqueue_cameras(buf.ptr, 4, host)
            host[:] = 0xFFFF                                               # garbage as soon as the call has returned
        one = {}
        for back, idx in zip((2, 1, 0), indices):
            res = [bytes(r) for r in det.fetch(4, back=back)]
            for i, j in enumerate(idx):
                if i == j:
                    assert res[i] == alone[j][0], (back, i)
                else:
                    if (i, j) not in one:                                   # frame i as camera j sees it: a one-camera handle's word
                        h1 = ssd.Detector(d["cfg"], d["trans"][j], gpu_device)
                        try:
                            one[(i, j)] = bytes(h1.process_host(d["frames"][i])[0])
                        finally:
                            h1.close()
                    assert res[i] == one[(i, j)] and res[i] != alone[i][0], (back, i, j)
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_host_path_slices_hand_on_their_part_of_the_index(ssd, oracle, gpu_device, lanes):
    d = _set(ssd, oracle, "vga")
    n = 40
    which = [(3 * k + k // 7) % 4 for k in range(n)]                         # the frame and its camera: changes across frame 32
    assert which[31] != which[32]
    frames = np.ascontiguousarray(np.stack([d["frames"][j] for j in which]), dtype=np.float32)
    cfg = ssd.default_config(d["w"], d["h"], max_frames_per_batch=64, batches_in_flight=lanes)
    det = _identity_detector(ssd, cfg, gpu_device)
    wh = d["w"] * d["h"]
    buf = _upload(ssd, list(frames), gpu_device)
    lbuf = ssd.DeviceBuffer(wh * n, gpu_device)
    pinned = ssd.PinnedArray(frames.shape, np.float32)
    try:
        det.set_cameras(d["trans"])
        det.enqueue_cameras(buf.ptr, n, which, d_labels=lbuf.ptr)
        want = [bytes(r) for r in det.fetch_list(n)]
        want_labels = lbuf.download(wh * n).tobytes()
        alone = _alone(ssd, d, gpu_device)
        assert all(want[k] == alone[which[k]][0] for k in range(n))
        pinned.array[...] = frames
        for src in (frames, pinned.array):
            res = det.process_host_cameras(src, which)
            assert [bytes(r) for r in res] == want
            res, lab = det.process_host_cameras(src, which, labels=True)
            assert [bytes(r) for r in res] == want and lab.tobytes() == want_labels
    finally:
        pinned.free()
        buf.free()
        lbuf.free()
        det.close()


@pytest.mark.gpu
def test_contracts(ssd, oracle, gpu_device):
    d = _set(ssd, oracle, "vga")
    alone = _alone(ssd, d, gpu_device)
    cfg, wh = d["cfg"], d["w"] * d["h"]
    det = ssd.Detector(cfg, d["trans"][0], gpu_device)
    buf = _upload(ssd, d["frames"], gpu_device)
    try:
        # the workspace of a handle without cameras: ssd_create's formula (two passes at this batch size: no planes)
        det.enqueue(buf.ptr, 1)
        det.fetch(1)
        state = det.frame_state(0)[1]["size"]                               # sizeof(FrameState)
        img = d["h"] * ((d["w"] + 63) // 64) * 8                            # one bit image
        records = (wh + 1023) // 1024 * 16 * 8                              # a frame's cell records
        base = det.workspace_bytes
        assert base == F * (state + (cfg.max_step_plateaus + 1) * img + records) + 2 * F * ssd.C.sizeof(ssd.FrameResult)
        with pytest.raises(ssd.SsdError, match="no camera table"):
            det.enqueue_cameras(buf.ptr, 4, [0, 0, 0, 0])
        det.enqueue(buf.ptr, 4)
        plain = [bytes(r) for r in det.fetch_list(4)]
        assert plain[0] == alone[0][0]
        with pytest.raises(ssd.SsdError):
            det.set_cameras([d["trans"][0]] * (ssd.MAX_CAMERAS + 1))
        assert det.camera_count == 0 and det.workspace_bytes == base
        det.set_cameras(d["trans"])
        with_table = det.workspace_bytes
        assert with_table > base and with_table - base < 65536
        # an index equal to the camera count: refused, and the batch before it is still there, unchanged
        det.enqueue_cameras(buf.ptr, 4, [0, 1, 2, 3])
        with pytest.raises(ssd.SsdError, match="names camera 4 of 4"):
            det.enqueue_cameras(buf.ptr, 4, [0, 1, 4, 3])
        got = [bytes(r) for r in det.fetch_list(4)]
        assert got == [alone[j][0] for j in range(4)]
        # plain enqueue keeps ssd_create's calibration whatever the table holds
        det.enqueue(buf.ptr, 4)
        assert [bytes(r) for r in det.fetch_list(4)] == plain
        # set_cameras while a batch is unfetched: it waits; the results are intact
        det.enqueue_cameras(buf.ptr, 4, [3, 2, 1, 0])
        det.set_cameras(list(reversed(d["trans"])))
        crossed = [bytes(r) for r in det.fetch_list(4)]
        det.enqueue_cameras(buf.ptr, 4, [0, 1, 2, 3])                       # the reversed table: the same pairing again
        assert [bytes(r) for r in det.fetch_list(4)] == crossed
        det.set_cameras([])
        assert det.camera_count == 0 and det.workspace_bytes == base
        with pytest.raises(ssd.SsdError, match="no camera table"):
            det.enqueue_cameras(buf.ptr, 4, [0, 0, 0, 0])
        det.enqueue(buf.ptr, 4)
        assert [bytes(r) for r in det.fetch_list(4)] == plain
    finally:
        buf.free()
        det.close()
