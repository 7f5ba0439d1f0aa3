"""Riser labels on the GPU (k_riser_labels; include/ssd_hip.h): the evidence pixels of every vertical face in
the label mask, against tests/riser_model.py on the handle's own debug record pixel for pixel, against the device's own riser records
and riser moments, through every entry point that writes labels, and with every switch that decides whether anything is marked.
Frames: ground_model's 256 x 192 scene and full_width's 640 x 480 (642 x 479) frames; the batches are uploaded at a stride that is no
multiple of 16, the labels go to poisoned buffers at a stride of W H + 37 with one frame of poison behind the batch."""
import numpy as np
import pytest

import clouds
import full_width as fw
import ground_model as gm
import riser_model as rm
import scenes

pytestmark = pytest.mark.gpu

POISON = 0xA5
LABEL_PAD = 37
TOL, SUPPORT = fw.TOL, fw.SUPPORT
FULL, NINE, BARE = 16, 8, 0
# the five layouts at 17 surfaces, the 9-surface frame, and the bare ground (no riser, wantedRisers == 0) between frames with risers
BATCH = [("ordered", FULL), ("scatter", FULL), ("lanes", FULL), ("slots", FULL), ("sparse", FULL), ("scatter", NINE), ("ordered", BARE), ("scatter", FULL)]
TWO_PASSES, SINGLE_PASS, NO_PLANES = (0, 0), (1, 0), (1, 2)     # Detector.single_pass(mode, sabotage)
Z = 0.5


class Got:
    """what one labelling enqueue returned: labels uint8 [n, W H], res / risers / rmom / dbg as lists of bytes (rmom, dbg: where asked)"""


def _upload(ssd, frames, device, depth=False):
    """frames at a stride of their size + 4 (depth: + 8) bytes, which is no multiple of 16 -> (buffer, stride)"""
    stride = frames[0].nbytes + (8 if depth else 4)
    assert stride % 16 != 0
    buf = ssd.DeviceBuffer(stride * len(frames), device)
    for i, f in enumerate(frames):
        buf.upload(np.ascontiguousarray(f), offset=i * stride)
    return buf, stride


def _label(ssd, det, src, stride, n, device, depth=False, order=None, moments=False, debug=False):
    """one enqueue with labels into a poisoned buffer of n + 1 frames at a stride of W H + 37: the padding and the frame past nframes
    must still be poison"""
    wh = det.cfg.width * det.cfg.height
    lstride = wh + LABEL_PAD
    lab = ssd.DeviceBuffer(lstride * (n + 1), device)
    try:
        lab.upload(np.full(lstride * (n + 1), POISON, dtype=np.uint8))
        if order is not None:
            det.enqueue_cameras(src.ptr, n, order, depth=depth, d_labels=lab.ptr, label_stride=lstride, stride_bytes=stride)
        elif depth:
            det.enqueue_depth_labels(src.ptr, n, lab.ptr, label_stride=lstride, stride_bytes=stride)
        else:
            det.enqueue_labels(src.ptr, n, lab.ptr, label_stride=lstride, stride_bytes=stride)
        out = Got()
        out.res = [bytes(r) for r in det.fetch_list(n)]
        raw = lab.download(lstride * (n + 1))
    finally:
        lab.free()
    for i in range(n):
        assert np.all(raw[i * lstride + wh:(i + 1) * lstride] == POISON), "label padding of frame %d was written" % i
    assert np.all(raw[n * lstride:] == POISON), "labels past nframes were written"
    out.labels = np.stack([raw[i * lstride:i * lstride + wh] for i in range(n)])
    out.risers = det.fetch_risers(n)
    if moments:
        out.rmom = det.fetch_riser_moments(n)
    if debug:
        out.dbg = [det.debug(i) for i in range(n)]
    return out


def _open(ssd, device, w, h, n, trans, riser_labels=True, risers=True, moments=False, debug=False, mode=None, workspaces=0, intr=None):
    det = ssd.Detector(ssd.default_config(w, h, max_frames_per_batch=n, batches_in_flight=workspaces), trans, device)
    if intr is not None:
        det.set_intrinsics(intr)
    if mode is not None:
        det.single_pass(*mode)
    if risers:
        det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
    if moments:
        det.set_riser_moments(True)
    if debug:
        det.set_debug(True, images=False)
    if riser_labels:
        det.set_riser_labels(True)
    return det


def _check_model(ssd, cfg, cal, xyz, got, plain, i, tol=TOL):
    """frame i of `got` (riser labels on, with debug records): the riser half is riser_model's word on the handle's own debug record at
    every pixel, the surface half the bytes of `plain` (the same frames with riser labels off), and the counts are the riser records'"""
    surfaces, risers = ssd.labels_split(got.labels[i])
    want = rm.riser_labels(cfg, cal, got.dbg[i], xyz, tol)
    diff = np.flatnonzero(risers != want)
    assert len(diff) == 0, "frame %d: %d pixels differ from riser_model, the first at %d: %d for %d" % (i, len(diff), diff[0], risers[diff[0]], want[diff[0]])
    assert np.array_equal(surfaces, plain.labels[i]), "frame %d: the surface labels moved" % i
    counts = np.bincount(got.labels[i], minlength=256)
    ris = got.risers[i]
    for k in range(ssd.MAX_RISERS):
        assert int(counts[ssd.LABEL_RISER_BASE + k]) == (ris.risers[k].n_points if k < ris.n_risers else 0), (i, k)
    assert not counts[ssd.MAX_STEPS + 1:ssd.LABEL_RISER_BASE].any() and not counts[ssd.LABEL_RISER_BASE + ssd.MAX_RISERS:].any(), i
    return risers


# ---- the main batch: run once with riser labels off and once with them on, on one handle -------------------------------------------
_MAIN = {}


def _frames(batch, w=fw.W, h=fw.H):
    return [fw.frame(layout, n_steps, w, h, Z) for layout, n_steps in batch]


def main_run(ssd, device):
    """BATCH behind a handle with risers, riser moments and debug records on: (off, on) - the same enqueue with riser labels off, then on"""
    if "run" not in _MAIN:
        frames = _frames(BATCH)
        det = _open(ssd, device, fw.W, fw.H, len(frames), clouds.calibration(ssd, Z), riser_labels=False, moments=True, debug=True)
        src = None
        try:
            src, stride = _upload(ssd, frames, device)
            off = _label(ssd, det, src, stride, len(frames), device, moments=True, debug=True)
            det.set_riser_labels(True)
            on = _label(ssd, det, src, stride, len(frames), device, moments=True, debug=True)
            _MAIN["run"] = (off, on)
        except BaseException as e:                      # a batch that failed, or faulted, is not started again by the next test
            _MAIN["run"] = e
        finally:
            if src is not None:
                src.free()
            det.close()
    if isinstance(_MAIN["run"], BaseException):
        raise _MAIN["run"]
    return _MAIN["run"]


def test_every_pixel_is_the_models(ssd, gpu_device):
    """1. the riser half of the mask equals riser_model.riser_labels on the handle's debug record at every pixel of every frame, the
    surface half the label bytes of the same enqueue with riser labels off; the bare ground between staircases carries none"""
    off, on = main_run(ssd, gpu_device)
    cfg, cal = ssd.default_config(fw.W, fw.H), clouds.calibration(ssd, Z).constants
    frames = _frames(BATCH)
    for i, (layout, n_steps) in enumerate(BATCH):
        risers = _check_model(ssd, cfg, cal, frames[i], on, off, i)
        assert on.risers[i].n_risers == n_steps and int(risers.max(initial=0)) == n_steps, (i, layout)
        assert int(off.labels[i].max(initial=0)) == (n_steps + 1 if n_steps else 0), "riser labels off: surface labels alone"
        if n_steps:
            assert np.bincount(risers, minlength=n_steps + 1)[1:].min() > 0, "frame %d: a riser without a pixel" % i
    assert not on.labels[6].any() and on.labels[5].max() == ssd.LABEL_RISER_BASE + 7 and on.labels[7].max() == ssd.LABEL_RISER_BASE + 15
    assert np.array_equal(on.labels[1], on.labels[7]), "the same frame twice in a batch"


def test_counts_and_moments_against_the_devices_own_records(ssd, gpu_device):
    """2. per frame and riser the count of label 32 + i is risers[i].n_points, and ssd_surface_moments_host over the split riser labels
    is the frame's ssd_fetch_riser_moments record, byte for byte, all 16 risers"""
    off, on = main_run(ssd, gpu_device)
    cfg = ssd.default_config(fw.W, fw.H)
    frames = _frames(BATCH)
    for i, (layout, n_steps) in enumerate(BATCH):
        ris = on.risers[i]
        counts = np.bincount(on.labels[i], minlength=256)
        assert ris.n_risers == n_steps
        for k in range(ssd.MAX_RISERS):
            assert int(counts[ssd.LABEL_RISER_BASE + k]) == (ris.risers[k].n_points if k < n_steps else 0), (i, k)
            assert k >= n_steps or ris.risers[k].n_points >= SUPPORT, (i, k)
        risers = ssd.labels_split(on.labels[i])[1]
        want = ssd.surface_moments_host(cfg, frames[i], risers, ris.n_risers, 0)
        got = on.rmom[i]
        for k in range(ssd.MAX_STEPS):
            assert bytes(got.s[k]) == bytes(want.s[k]), "frame %d (%s), riser %d: the moments are not the host's sums over the device's labels" % (i, layout, k)
        assert bytes(got) == bytes(want), i
    assert on.rmom[1].n_surfaces == 16 and on.rmom[1].s[15].m.n > 0


def test_nothing_else_moves(ssd, gpu_device):
    """3. results, risers, riser moments and debug records are the same bytes with riser labels on and off"""
    off, on = main_run(ssd, gpu_device)
    assert on.res == off.res
    assert [bytes(r) for r in on.risers] == [bytes(r) for r in off.risers]
    assert [bytes(m) for m in on.rmom] == [bytes(m) for m in off.rmom]
    assert [bytes(d) for d in on.dbg] == [bytes(d) for d in off.dbg]
    assert any(l.max() >= ssd.LABEL_RISER_BASE for l in on.labels) and all(l.max() <= ssd.MAX_STEPS for l in off.labels)


# ---- input forms and modes -----------------------------------------------------------------------------------------------------------
def _small_scenes(ssd):
    """ground_model's 256 x 192 three-step scene, the bare floor of the same pose, and the scene once more with other noise"""
    return [gm.scene(ssd, "steps"), gm.scene(ssd, "floor"), gm.scene(ssd, "steps", seed=8, sigma=0.0015)]


_SMALL = {}


def small_run(ssd, device):
    """the three small frames as vertices: (frames, off, on) as main_run"""
    if "run" not in _SMALL:
        scs = _small_scenes(ssd)
        frames = list(ssd.synth_host(scs))
        det = _open(ssd, device, gm.W, gm.H, len(frames), ssd.transformation_for_scene(scs[0]), riser_labels=False, moments=True, debug=True)
        src = None
        try:
            src, stride = _upload(ssd, frames, device)
            off = _label(ssd, det, src, stride, len(frames), device, moments=True, debug=True)
            det.set_riser_labels(True)
            on = _label(ssd, det, src, stride, len(frames), device, moments=True, debug=True)
            _SMALL["run"] = (frames, off, on)
        except BaseException as e:
            _SMALL["run"] = e
        finally:
            if src is not None:
                src.free()
            det.close()
    if isinstance(_SMALL["run"], BaseException):
        raise _SMALL["run"]
    return _SMALL["run"]


def test_the_small_scene_and_sixteen_bit_depth(ssd, gpu_device):
    """4a. ground_model's scene as vertices and as 16-bit depth (deprojected for the model as ssd_deproject_host does): every pixel the
    model's, two risers with evidence, the floor frame between them without a riser label; the depth host call gives the same bytes"""
    scs = _small_scenes(ssd)
    cfg, trans = ssd.default_config(gm.W, gm.H), ssd.transformation_for_scene(scs[0])
    frames, off, on = small_run(ssd, gpu_device)
    for i in range(3):
        _check_model(ssd, cfg, trans.constants, frames[i], on, off, i)
    assert [r.n_risers for r in on.risers] == [2, 0, 2] and not on.labels[1].any()
    assert all(on.risers[i].risers[k].n_points > 0 for i in (0, 2) for k in range(2))
    intr = ssd.intrinsics_for_scene(scs[0])
    depth = list(ssd.synth_depth_host(scs))
    xyz = [ssd.deproject_host(intr, d) for d in depth]
    det = _open(ssd, gpu_device, gm.W, gm.H, 3, trans, riser_labels=False, debug=True, intr=intr)
    src = None
    try:
        src, stride = _upload(ssd, depth, gpu_device, depth=True)
        d_off = _label(ssd, det, src, stride, 3, gpu_device, depth=True, debug=True)
        det.set_riser_labels(True)
        d_on = _label(ssd, det, src, stride, 3, gpu_device, depth=True, debug=True)
        for i in range(3):
            _check_model(ssd, cfg, trans.constants, xyz[i], d_on, d_off, i)
        assert [r.n_risers for r in d_on.risers] == [2, 0, 2] and d_on.labels[0].max() == ssd.LABEL_RISER_BASE + 1
        det.set_debug(False)
        res, lab = det.process_depth_host_labels(np.stack(depth))
        assert np.array_equal(lab.reshape(3, -1), d_on.labels) and [bytes(r) for r in res] == d_on.res
    finally:
        if src is not None:
            src.free()
        det.close()


@pytest.mark.parametrize("mode", [TWO_PASSES, SINGLE_PASS, NO_PLANES], ids=["two_passes", "single_pass", "no_planes"])
def test_behind_every_mode_of_k1(ssd, gpu_device, mode):
    """4b. three frames of the main batch behind K1's two passes, its single pass and a predictor that hands out no planes: the bytes
    of the main batch's frames"""
    picks = [1, 6, 4]
    frames = _frames([BATCH[i] for i in picks])
    off, on = main_run(ssd, gpu_device)
    det = _open(ssd, gpu_device, fw.W, fw.H, 3, clouds.calibration(ssd, Z), mode=mode)
    src = None
    try:
        src, stride = _upload(ssd, frames, gpu_device)
        got = _label(ssd, det, src, stride, 3, gpu_device)
        st = det.single_pass_stats(3)
        assert st["ran"] == (mode != TWO_PASSES), st
        if mode == NO_PLANES:
            assert st["covered"] == 0 and st["planes"] == 0, st
        for j, i in enumerate(picks):
            assert np.array_equal(got.labels[j], on.labels[i]), "frame %d: not the main batch's bytes" % i
            assert got.res[j] == on.res[i] and bytes(got.risers[j]) == bytes(on.risers[i])
    finally:
        if src is not None:
            src.free()
        det.close()


def test_a_handle_with_three_workspaces(ssd, gpu_device):
    """4c. batches_in_flight = 3: two labelling enqueues in a row, then one with riser labels off, then one more with them on - each
    the bytes of the one-workspace handle"""
    frames, off, on = small_run(ssd, gpu_device)
    scs = _small_scenes(ssd)
    det = _open(ssd, gpu_device, gm.W, gm.H, 3, ssd.transformation_for_scene(scs[0]), workspaces=3)
    src = None
    try:
        assert det.batches_in_flight == 3
        src, stride = _upload(ssd, frames, gpu_device)
        for want, switch in ((on, None), (on, None), (off, False), (on, True)):
            if switch is not None:
                det.set_riser_labels(switch)
            got = _label(ssd, det, src, stride, 3, gpu_device)
            assert np.array_equal(got.labels, want.labels) and got.res == want.res
            assert [bytes(r) for r in got.risers] == [bytes(r) for r in want.risers]
    finally:
        if src is not None:
            src.free()
        det.close()


def test_the_ragged_frame(ssd, gpu_device):
    """4d. 642 x 479 = 307,518 points, no multiple of 4 or of 64 (the 12-byte load path, a partial last cell, label rows at odd
    addresses), 17 surfaces, scattered and with every second cell empty: every pixel the model's"""
    w, h = 642, 479
    batch = [("scatter", FULL), ("sparse", FULL), ("lanes", FULL)]
    frames = _frames(batch, w, h)
    assert (w * h) % 4 != 0 and frames[0].reshape(-1, 3)[w * h // 64 * 64:, 2].any(), "the partial last cell holds a point"
    cfg, trans = ssd.default_config(w, h), clouds.calibration(ssd, Z)
    det = _open(ssd, gpu_device, w, h, 3, trans, riser_labels=False, debug=True)
    src = None
    try:
        src, stride = _upload(ssd, frames, gpu_device)
        off = _label(ssd, det, src, stride, 3, gpu_device, debug=True)
        det.set_riser_labels(True)
        on = _label(ssd, det, src, stride, 3, gpu_device, debug=True)
        for i in range(3):
            risers = _check_model(ssd, cfg, trans.constants, frames[i], on, off, i)
            assert on.risers[i].n_risers == 16 and np.bincount(risers, minlength=17)[1:].min() > 0
    finally:
        if src is not None:
            src.free()
        det.close()


def test_a_host_call_across_a_slice_boundary(ssd, gpu_device):
    """4e. 33 frames through ssd_process_host_labels on a handle of 32 frames per batch: two slices; every frame's labels, results and
    risers are those of the resident batch"""
    frames, off, on = small_run(ssd, gpu_device)
    scs = _small_scenes(ssd)
    n = 33
    det = ssd.Detector(ssd.default_config(gm.W, gm.H, max_frames_per_batch=32), ssd.transformation_for_scene(scs[0]), gpu_device)
    try:
        det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
        det.set_riser_labels(True)
        xyz = np.stack([frames[i % 3] for i in range(n)])
        res, lab = det.process_host_labels(xyz)
        ris = det.fetch_risers(n)
        for i in range(n):
            assert np.array_equal(lab[i].reshape(-1), on.labels[i % 3]), "frame %d" % i
            assert bytes(res[i]) == on.res[i % 3] and bytes(ris[i]) == bytes(on.risers[i % 3]), i
        det.set_riser_labels(False)
        res, lab = det.process_host_labels(xyz)
        for i in range(n):
            assert np.array_equal(lab[i].reshape(-1), off.labels[i % 3]), "frame %d, riser labels off" % i
    finally:
        det.close()


# ---- camera batches ------------------------------------------------------------------------------------------------------------------
# three mountings that differ in pitch, roll and height; for depth input the first two also differ in optics and depth units
POSES = [dict(pitch_deg=50.0, roll_deg=25.0, cam_height=1.0), dict(pitch_deg=46.0, roll_deg=-20.0, cam_height=0.92),
         dict(pitch_deg=52.0, roll_deg=18.0, cam_height=1.06)]
OPTICS = [dict(hfov_deg=70.0), dict(hfov_deg=62.0)]
UNITS = [0.00025, 0.0001]


def test_camera_batches_equal_the_one_camera_handles(ssd, gpu_device):
    """5. three cameras whose calibrations differ, six frames in mixed order (vertices from all three, 16-bit depth from the two with
    intrinsics): each frame's label bytes are those of a handle created with that frame's camera, resident and through the host entry
    point.  The handle's own calibration is the identity: a fall-back to it would be wrong everywhere."""
    W, H = gm.W, gm.H
    det = _open(ssd, gpu_device, W, H, 8, ssd.GeometricTransformation())
    bufs = []
    try:
        for depth, order in ((False, [2, 0, 1, 2, 0, 1]), (True, [1, 0, 0, 1, 1, 0])):
            ncam = 2 if depth else 3
            scs = [ssd.make_scene(W, H, n_steps=3, seed=11 + j, sigma=0.001 + 0.0005 * j, **POSES[j], **(OPTICS[j] if depth else {})) for j in range(ncam)]
            trans = [ssd.transformation_for_scene(sc) for sc in scs]
            intr = [ssd.intrinsics_for_scene(sc, depth_units=u) for sc, u in zip(scs, UNITS)] if depth else [None] * ncam
            frames = [ssd.synth_depth_host([sc], depth_units=u)[0] for sc, u in zip(scs, UNITS)] if depth else list(ssd.synth_host(scs))
            alone = []
            for j in range(ncam):
                one = _open(ssd, gpu_device, W, H, 1, trans[j], intr=intr[j])
                try:
                    buf, stride = _upload(ssd, [frames[j]], gpu_device, depth=depth)
                    bufs.append(buf)
                    alone.append(_label(ssd, one, buf, stride, 1, gpu_device, depth=depth))
                finally:
                    one.close()
                assert alone[j].risers[0].n_risers >= 2 and alone[j].labels[0].max() >= ssd.LABEL_RISER_BASE + 1, "camera %d: riser labels" % j
            assert len(set(a.labels[0].tobytes() for a in alone)) == ncam, "as many different masks as cameras"
            table = ([(t, i) for t, i in zip(trans, intr)] if depth else trans) + [ssd.GeometricTransformation()]
            det.set_cameras(table)
            n = len(order)
            buf, stride = _upload(ssd, [frames[j] for j in order], gpu_device, depth=depth)
            bufs.append(buf)
            got = _label(ssd, det, buf, stride, n, gpu_device, depth=depth, order=order)
            for i, j in enumerate(order):
                assert np.array_equal(got.labels[i], alone[j].labels[0]), "frame %d (camera %d): not the one-camera handle's labels" % (i, j)
                assert got.res[i] == alone[j].res[0] and bytes(got.risers[i]) == bytes(alone[j].risers[0]), (i, j)
            res_h, lab_h = det.process_host_cameras(np.stack([frames[j] for j in order]), order, depth=depth, labels=True)
            assert np.array_equal(lab_h.reshape(n, -1), got.labels) and [bytes(r) for r in res_h] == got.res
    finally:
        for b in bufs:
            b.free()
        det.close()


# ---- the switches --------------------------------------------------------------------------------------------------------------------
def test_the_switches(ssd, gpu_device):
    """6a-c. on one handle: riser labels on before risers are (nothing marked); risers on (marked, and the kernel's time is reported
    beside k_labels'); risers off again straight after that batch, so that the state k_final left is stale (nothing marked, time 0);
    riser labels off with risers on (nothing marked)"""
    frames, off, on = small_run(ssd, gpu_device)
    scs = _small_scenes(ssd)
    det = _open(ssd, gpu_device, gm.W, gm.H, 3, ssd.transformation_for_scene(scs[0]), riser_labels=False, risers=False)
    src = None

    def plain_label():
        """risers off: ssd_fetch_risers is refused, so the enqueue by hand"""
        wh = gm.W * gm.H
        lab = ssd.DeviceBuffer((wh + LABEL_PAD) * 4, gpu_device)
        try:
            lab.upload(np.full((wh + LABEL_PAD) * 4, POISON, dtype=np.uint8))
            det.enqueue_labels(src.ptr, 3, lab.ptr, label_stride=wh + LABEL_PAD, stride_bytes=stride)
            res = [bytes(r) for r in det.fetch_list(3)]
            raw = lab.download((wh + LABEL_PAD) * 4).reshape(4, -1)
        finally:
            lab.free()
        assert np.all(raw[:3, wh:] == POISON) and np.all(raw[3] == POISON)
        return res, raw[:3, :wh]

    try:
        src, stride = _upload(ssd, frames, gpu_device)
        det.set_timing(True)
        det.set_riser_labels(True)                       # legal while risers are off ...
        res, lab = plain_label()
        assert np.array_equal(lab, off.labels) and res == off.res, "riser labels on, risers off: the bytes without them"
        assert det.riser_labels_time_ms() == 0.0 and det.labels_time_ms() > 0.0
        det.set_risers(True, tolerance=TOL, min_support=SUPPORT)      # ... and takes effect when they come on
        got = _label(ssd, det, src, stride, 3, gpu_device)
        assert np.array_equal(got.labels, on.labels) and got.res == on.res
        assert det.riser_labels_time_ms() > 0.0 and det.labels_time_ms() > 0.0
        det.set_risers(False)                            # the state of the batch above still names risers
        res, lab = plain_label()
        assert np.array_equal(lab, off.labels) and res == off.res, "risers off behind a risers-on batch: stale state must not be read"
        assert det.riser_labels_time_ms() == 0.0 and det.riser_labels_time_ms(back=1) > 0.0
        det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
        det.set_riser_labels(False)
        got = _label(ssd, det, src, stride, 3, gpu_device)
        assert np.array_equal(got.labels, off.labels) and got.res == off.res, "riser labels off, risers on: the bytes without them"
        assert [bytes(r) for r in got.risers] == [bytes(r) for r in on.risers] and det.riser_labels_time_ms() == 0.0
        det.enqueue(src.ptr, 3, stride_bytes=stride)     # a call that writes no labels marks nothing
        det.set_riser_labels(True)
        det.enqueue(src.ptr, 3, stride_bytes=stride)
        assert [bytes(r) for r in det.fetch_list(3)] == on.res and det.riser_labels_time_ms() == 0.0
    finally:
        if src is not None:
            src.free()
        det.close()


def test_the_tolerance_at_an_evidence_points_distance(ssd, gpu_device):
    """6d. the tolerance set to exactly |s| of an evidence point of riser 7 and to the next double below it: exactly the pixels with
    that |s| change, from 32 + 7 to 0, and each mask is the model's at its tolerance"""
    off, on = main_run(ssd, gpu_device)
    xyz = fw.frame("scatter", FULL, fw.W, fw.H, Z)
    cfg, trans = ssd.default_config(fw.W, fw.H), clouds.calibration(ssd, Z)
    dbg = on.dbg[1]
    labels, s = rm.evidence(cfg, trans.constants, dbg, xyz, TOL)
    mine = np.abs(s[labels == 8])
    assert len(mine) == on.risers[1].risers[7].n_points
    edge = float(np.sort(mine)[len(mine) // 2])                      # a point in the middle: half the evidence lies beyond it
    below = float(np.nextafter(edge, 0.0))
    at_edge = np.flatnonzero((labels == 8) & (np.abs(s) == edge))
    assert 0.0 < below < edge < TOL and len(at_edge) >= 1
    det = _open(ssd, gpu_device, fw.W, fw.H, 1, trans)
    src = None
    try:
        src, stride = _upload(ssd, [xyz], gpu_device)
        masks = []
        for tol in (edge, below):
            det.set_risers(True, tolerance=tol, min_support=SUPPORT)
            got = _label(ssd, det, src, stride, 1, gpu_device)
            assert np.array_equal(ssd.labels_split(got.labels[0])[1], rm.riser_labels(cfg, trans.constants, dbg, xyz, tol)), tol
            masks.append(got.labels[0])
        moved = np.flatnonzero(masks[0] != masks[1])
        assert np.array_equal(moved, at_edge), "exactly the pixels at the tolerance move"
        assert np.all(masks[0][moved] == ssd.LABEL_RISER_BASE + 7) and np.all(masks[1][moved] == 0)
    finally:
        if src is not None:
            src.free()
        det.close()


# ---- frames without risers -----------------------------------------------------------------------------------------------------------
def test_a_frame_with_one_emitted_surface_carries_no_riser_label(ssd, gpu_device):
    """7a. a step plateau with the face under it and no ground - one emitted surface, the face's points in bins of no plateau - between
    two frames of ground + step (two surfaces, one riser): label 1 alone in the middle frame, 32 in its neighbours"""
    w, h = gm.W, gm.H
    cls = fw.classes(1, w, h)
    two = fw.place(cls, w, h, "scatter", z_shift=Z)[0]
    one = fw.place(cls[1:], w, h, "scatter", z_shift=Z)[0]
    det = _open(ssd, gpu_device, w, h, 3, clouds.calibration(ssd, Z))
    src = None
    try:
        src, stride = _upload(ssd, [two, one, two], gpu_device)
        got = _label(ssd, det, src, stride, 3, gpu_device)
        n_steps = [ssd.FrameResult.from_buffer_copy(r).n_steps for r in got.res]
        assert n_steps == [2, 1, 2] and [r.n_risers for r in got.risers] == [1, 0, 1]
        assert sorted(set(got.labels[1].tolist())) == [0, 1], "one emitted surface: no label at or above 32"
        for i in (0, 2):
            assert sorted(set(got.labels[i].tolist())) == [0, 1, 2, ssd.LABEL_RISER_BASE]
            assert int((got.labels[i] == ssd.LABEL_RISER_BASE).sum()) == got.risers[i].risers[0].n_points > 0
    finally:
        if src is not None:
            src.free()
        det.close()


def test_a_frame_the_reference_throws_on_carries_no_label(ssd, gpu_device):
    """7b. a frame whose status has SSD_ST_THROW: every byte zero, no riser - beside a staircase at the same resolution, which is marked"""
    throws, stairs = scenes.make(ssd, "vga_yaw50_throws"), scenes.make(ssd, "vga_3steps_noise2mm")
    frames = [ssd.synth_host([sc])[0] for sc in (stairs, throws)]
    for sc, frame, status in ((stairs, frames[0], 0), (throws, frames[1], ssd.ST_THROW)):
        det = _open(ssd, gpu_device, sc.width, sc.height, 1, ssd.transformation_for_scene(sc))
        src = None
        try:
            src, stride = _upload(ssd, [frame], gpu_device)
            got = _label(ssd, det, src, stride, 1, gpu_device)
            res = ssd.FrameResult.from_buffer_copy(got.res[0])
            assert res.status & ssd.ST_THROW == status
            if status:
                assert not got.labels[0].any() and got.risers[0].n_risers == 0, "a frame with SSD_ST_THROW carries no label"
            else:
                assert got.labels[0].max() >= ssd.LABEL_RISER_BASE and got.risers[0].n_risers == res.n_steps - 1 >= 2
        finally:
            if src is not None:
                src.free()
            det.close()
