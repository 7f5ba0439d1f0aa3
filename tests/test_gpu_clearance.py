"""Tread clearance on the GPU (k_clearance, k_clearance_cams; include/ssd_hip.h): the device's records and masks
byte for byte ssd_clearance_host on the handle's OWN fetched result, the host sums over the device's mask (ssd_surface_moments_host) equal
to the device's records, and the entry points' contract.  Every pass runs into poisoned buffers, the mask at a stride of W H + 37, the
frames at a stride that is no multiple of 16, with one record and one mask row of poison behind the batch.  No tolerance anywhere: the
sums are integers and the decisions are one text.  Frames: tests/clearance_model.py's."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as cm
import clouds
import full_width as fw
import ground_model as gm
import oracle_binding as ob
from test_labels import expected_labels

pytestmark = pytest.mark.gpu

POISON = 0xA5
MASK_PAD = 37
TWO_PASSES, SINGLE_PASS, NO_PLANES = (0, 0), (1, 0), (1, 2)     # Detector.single_pass(mode, sabotage)


class Resident:
    """frames resident on the device behind one detector; every pass into freshly poisoned buffers"""

    def __init__(self, ssd, device, cfg, trans, frames, depth=False, intr=None, mode=None, cameras=None, order=None, pad=None, fill=None):
        self.ssd, self.cfg, self.depth, self.intr, self.order = ssd, cfg, depth, intr, order
        self.frames, self.n, self.wh = frames, len(frames), cfg.width * cfg.height
        self.cal = trans.constants
        self.det = ssd.Detector(cfg, trans, device)
        self.device = device
        self.bufs = []
        if cameras is not None:
            self.det.set_cameras(cameras)
        elif depth:
            self.det.set_intrinsics(intr)
        if mode is not None:
            self.det.single_pass(*mode)
        fb = frames[0].nbytes
        self.stride = fb + ((8 if depth else 4) if pad is None else pad)       # pad: for a frame size that + 8 brings to a multiple of 16
        assert self.stride % 16 != 0
        self.src = ssd.DeviceBuffer(self.stride * self.n, device)
        self.bufs.append(self.src)
        if fill is not None:                                           # a large batch: fill(buffer, stride) makes the frames on the device
            fill(self.src, self.stride)
        else:
            for i, f in enumerate(frames):
                self.src.upload(np.ascontiguousarray(f), offset=i * self.stride)
        self.rec = C.sizeof(ssd.FrameMoments)
        self.mstride = self.wh + MASK_PAD
        self.out = ssd.DeviceBuffer(self.rec * (self.n + 1), device)
        self.mask = ssd.DeviceBuffer(self.mstride * (self.n + 1), device)
        self.bufs += [self.out, self.mask]

    def close(self):
        for b in self.bufs:
            b.free()
        self.det.close()

    def enqueue(self, n=None):
        n = self.n if n is None else n
        if self.order is not None:
            self.det.enqueue_cameras(self.src.ptr, n, self.order[:n], depth=self.depth, stride_bytes=self.stride)
        else:
            (self.det.enqueue_depth if self.depth else self.det.enqueue)(self.src.ptr, n, stride_bytes=self.stride)

    def detect(self, n=None):
        self.enqueue(n)
        self.res = self.det.fetch_list(self.n if n is None else n)
        return self.res

    def clear(self, rule, mask=True, n=None):
        """the pass behind the last enqueue -> (records, masks [n, W H] or None); checks the poison around what it may write"""
        n = self.n if n is None else n
        self.out.upload(np.full(self.rec * (self.n + 1), POISON, dtype=np.uint8))
        self.mask.upload(np.full(self.mstride * (self.n + 1), POISON, dtype=np.uint8))
        self.det.enqueue_clearance(self.src.ptr, n, self.out.ptr, cm.rule_of(self.ssd, rule), self.mask.ptr if mask else None, self.mstride,
                                   depth=self.depth, stride_bytes=self.stride, cameras=self.order is not None)
        self.det.fetch_clearance()
        raw = self.out.download(self.rec * (self.n + 1))
        assert np.all(raw[self.rec * n:] == POISON), "a record past nframes was written"
        recs = list((self.ssd.FrameMoments * n).from_buffer_copy(raw[:self.rec * n].tobytes()))
        m = self.mask.download(self.mstride * (self.n + 1)).reshape(self.n + 1, self.mstride)
        if not mask:
            assert np.all(m == POISON), "a pass without a mask wrote one"
            return recs, None
        assert np.all(m[:n, self.wh:] == POISON) and np.all(m[n:] == POISON), "bytes beyond W H of a stride, or past nframes, were written"
        return recs, m[:n, :self.wh].copy()

    def cal_of(self, i):
        return self.cal if self.order is None else self.cameras_cal[self.order[i]]

    def check(self, rule, recs, masks, res=None, frames=None, ground=None):
        """records and masks byte for byte the host's on the handle's own results; the host sums over the device's mask = the records.
        ground: per frame whether its surface 0 is the ground (None: every live frame's is, as in this file's scenes)"""
        ssd, res, frames = self.ssd, res or self.res, frames or self.frames
        for i, r in enumerate(recs):
            live = res[i].n_steps > 0 and not (res[i].status & ssd.ST_THROW)
            flag = (1 if live else 0) if ground is None else ground[i]
            want, wmask = ssd.clearance_host(self.cfg, self.cal_of(i), frames[i], res[i], flag, cm.rule_of(ssd, rule), intr=self.intr_of(i))
            assert bytes(r) == bytes(want), (i, cm.sums_of_record(r, ssd.MAX_STEPS), cm.sums_of_record(want, ssd.MAX_STEPS))
            if masks is not None:
                assert np.array_equal(masks[i], wmask.reshape(-1)), i
                sums = ssd.surface_moments_host(self.cfg, frames[i], masks[i], r.n_surfaces, r.ground, intr=self.intr_of(i))
                assert bytes(sums) == bytes(r), i

    def intr_of(self, i):
        return self.intr if self.depth else None


def _kept(rec, k):
    return int(rec.s[k].m.n + rec.s[k].n_far)


def _scene_batch(ssd, oracle, depth):
    """the 256 x 192 scene (sigma 1 mm and 3 mm) with a patch on tread 1 and on the top tread, and the clean frame: five frames"""
    frames, pulled = [], []
    for sigma in (0.001, 0.003):
        _, trans, frame = cm.scene_frame(ssd, sigma, 7)
        cfg = ssd.default_config(gm.W, gm.H, max_frames_per_batch=5)      # the caller's own: it may change the batch size
        sc = gm.scene(ssd, "steps", sigma=sigma, seed=7)
        intr = ssd.intrinsics_for_scene(sc)
        cal = trans.constants
        if depth:
            d = ssd.synth_depth_host([sc])[0]
            pts = ssd.deproject_host(intr, d)
        else:
            pts = frame
        res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), pts)[0]
        fr = cm.result_of_oracle(ssd, res)
        labels = expected_labels(oracle, cfg, cal, res, pts)
        for surface in (1, fr.n_steps - 1):
            f2, sel = cm.patched(cfg, cal, fr, pts, labels, surface)
            if depth:
                f2 = d.copy()
                f2[sel] = np.round(f2[sel] * 0.9).astype(np.uint16)
            frames.append(f2)
            pulled.append((surface, sel.reshape(-1)))
    frames.append(d if depth else np.array(frame))
    pulled.append((None, None))
    return cfg, trans, intr, frames, pulled


@pytest.mark.parametrize("depth", [False, True])
def test_the_scenes_with_a_patch_equal_the_host(ssd, oracle, gpu_device, depth):
    """vertices and 16-bit depth; the pass repeated with another rule; without a mask; results, workspace bytes untouched"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, depth)
    cfg.max_frames_per_batch = len(frames)
    r = Resident(ssd, gpu_device, cfg, trans, frames, depth=depth, intr=intr)
    try:
        res = r.detect()
        before = r.det.workspace_bytes
        assert all(x.n_steps == 3 and not (x.status & ssd.ST_THROW) for x in res)
        recs, masks = r.clear(cm.RULE)
        r.check(cm.RULE, recs, masks)
        for i, (surface, sel) in enumerate(pulled):
            if surface is None:
                assert not masks[i].any() and all(_kept(recs[i], k) == 0 for k in range(ssd.MAX_STEPS)), "the clean frame holds nothing"
            elif surface == 1:
                assert np.count_nonzero(masks[i][sel] == surface + 1) >= 0.95 * np.count_nonzero(sel) and not masks[i][~sel].any()
            else:
                assert _kept(recs[i], surface) >= 50, "the patch on the top tread"
        # again with another rule (no margin: the riser faces leak in), and without a mask
        rule0 = (0.0, 0.02, 0.4)
        recs0, masks0 = r.clear(rule0)
        r.check(rule0, recs0, masks0)
        assert max(_kept(recs0[-1], k) for k in range(3)) > 500
        recs1, none = r.clear(cm.RULE, mask=False)
        assert [bytes(x) for x in recs1] == [bytes(x) for x in recs]
        assert r.det.workspace_bytes == before, "the pass allocates nothing that counts"
        assert [bytes(x) for x in r.det.fetch_list(r.n)] == [bytes(x) for x in res], "the results are still the enqueue's"
    finally:
        r.close()


def _wide_frames(ssd, oracle, w=fw.W, h=fw.H, layouts=fw.LAYOUTS):
    """the five full-width layouts with the raised points, the 9-surface frame and the bare ground"""
    refs = [fw.reference(ssd, oracle, l, fw.N_STEPS, w, h) for l in layouts]
    frames = [cm.raised(ref)[0] for ref in refs]
    if w == fw.W:
        frames += [np.array(fw.frame("scatter", 8)), np.array(fw.frame("ordered", 0))]
    return refs, frames


@pytest.mark.parametrize("mode", [TWO_PASSES, SINGLE_PASS, NO_PLANES], ids=["two-passes", "single-pass", "no-planes"])
def test_the_full_width_batch_in_all_three_k1_modes(ssd, oracle, gpu_device, mode):
    refs, frames = _wide_frames(ssd, oracle)
    cfg = ssd.default_config(fw.W, fw.H, max_frames_per_batch=len(frames))
    r = Resident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames, mode=mode)
    try:
        res = r.detect()
        assert [x.n_steps for x in res] == [17] * 5 + [9, res[-1].n_steps] and res[-1].n_steps <= 1
        recs, masks = r.clear(cm.WIDE_RULE)
        r.check(cm.WIDE_RULE, recs, masks)
        for i in range(4):                                             # the layouts that hold every point of the frame
            assert min(_kept(recs[i], k) for k in range(17)) >= 100, [_kept(recs[i], k) for k in range(17)]
        assert len({bytes(x) for x in recs[:4]}) == 1, "the layouts of one frame place the same points: one record"
    finally:
        r.close()


def test_the_ragged_frame(ssd, oracle, gpu_device):
    """642 x 479: no multiple of 4 or of 64 (the 12-byte load path, a partial last cell, mask rows at odd addresses)"""
    w, h = 642, 479
    refs, frames = _wide_frames(ssd, oracle, w, h, ("scatter", "sparse", "lanes"))
    cfg = ssd.default_config(w, h, max_frames_per_batch=len(frames))
    r = Resident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames)
    try:
        res = r.detect()
        assert [x.n_steps for x in res] == [17] * 3
        recs, masks = r.clear(cm.WIDE_RULE)
        r.check(cm.WIDE_RULE, recs, masks)
        assert all(min(_kept(recs[i], k) for k in range(17)) > 0 for i in (0, 2))
    finally:
        r.close()


def test_three_workspaces_and_a_wider_batch_before(ssd, oracle, gpu_device):
    """three workspaces: each pass behind its own batch; then, on one handle, a pass behind a batch of two frames after one of seven"""
    refs, frames = _wide_frames(ssd, oracle)
    cfg = ssd.default_config(fw.W, fw.H, max_frames_per_batch=len(frames), batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    r = Resident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames)
    try:
        want = None
        for turn in range(4):                                          # every workspace, and the first one again
            res = r.detect()
            recs, masks = r.clear(cm.WIDE_RULE)
            r.check(cm.WIDE_RULE, recs, masks)
            want = want or [bytes(x) for x in recs]
            assert [bytes(x) for x in recs] == want
        res2 = r.detect(2)
        recs, masks = r.clear(cm.WIDE_RULE, n=2)
        r.check(cm.WIDE_RULE, recs, masks, res=res2)
        assert [bytes(x) for x in recs] == want[:2]
    finally:
        r.close()


def test_lo_and_hi_at_exactly_one_occupants_height(ssd, oracle, gpu_device):
    """the band's ends moved onto one occupant's height above its surface and to the next double: exactly those pixels move"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    cfg.max_frames_per_batch = 1
    r = Resident(ssd, gpu_device, cfg, trans, frames[:1])
    try:
        res = r.detect()
        recs, masks = r.clear(cm.RULE)
        r.check(cm.RULE, recs, masks)
        _, _, _, wz = cm.world(cfg, r.cal, frames[0])
        occ = np.flatnonzero(masks[0] == 2)
        above = np.sort((wz[occ] + r.cal.world_z) - res[0].steps[1].height)
        assert len(occ) >= 285
        mid = float(above[len(above) // 2])
        # hi on that height and on the next double; lo likewise from below: each pass the host's and the model's, pixel by pixel
        counts = {}
        for rule in ((0.03, 0.03, mid), (0.03, 0.03, float(np.nextafter(mid, 9.0))), (0.03, mid, 0.5), (0.03, float(np.nextafter(mid, 0.0)), 0.5)):
            got, gmask = r.clear(rule)
            r.check(rule, got, gmask)
            assert np.array_equal(gmask[0], cm.occupants(cfg, r.cal, res[0], frames[0], rule))
            counts[rule] = (_kept(got[0], 1), gmask[0])
        (a, ma), (b, mb), (c, mc), (d, md) = counts.values()
        assert 0 < a <= b < len(occ) and b - a <= 1 and np.count_nonzero(ma != mb) == b - a, "hi: only a point on the band's end moves"
        assert 0 < c <= d < len(occ) and d - c <= 1 and np.count_nonzero(mc != md) == d - c, "lo: only a point on the band's end moves"
        assert a + c <= len(occ), "the two bands share no point"
    finally:
        r.close()


def test_a_cameras_batch_in_mixed_order_against_one_camera_handles(ssd, oracle, gpu_device):
    """three cameras (poses a little apart), frames in mixed order: frame i byte for byte a one-camera handle's"""
    poses = [dict(), dict(pitch_deg=52.0), dict(cam_height=1.05, roll_deg=1.0)]
    scs = [gm.scene(ssd, "steps", seed=7 + c, **kw) for c, kw in enumerate(poses)]
    cfg0 = ssd.default_config(gm.W, gm.H)
    trs = [ssd.transformation_for_scene(sc) for sc in scs]
    cams = [ssd.Camera() for _ in scs]
    for cam, tr in zip(cams, trs):
        cam.cal = tr.constants
    order = [2, 0, 1, 1, 2, 0]
    per_cam = []
    for sc, tr in zip(scs, trs):
        frame = ssd.synth_host([sc])[0]
        res = oracle.process(ob.to_oracle_config(cfg0), ob.to_oracle_calibration(tr.constants), frame)[0]
        fr = cm.result_of_oracle(ssd, res)
        per_cam.append(cm.patched(cfg0, tr.constants, fr, frame, expected_labels(oracle, cfg0, tr.constants, res, frame), 1)[0])
    frames = [per_cam[c] for c in order]
    cfg = ssd.default_config(gm.W, gm.H, max_frames_per_batch=len(frames))
    r = Resident(ssd, gpu_device, cfg, trs[0], frames, cameras=cams, order=order)
    r.cameras_cal = [tr.constants for tr in trs]
    try:
        res = r.detect()
        recs, masks = r.clear(cm.RULE)
        r.check(cm.RULE, recs, masks)
        assert all(_kept(recs[i], 1) >= 285 for i in range(len(frames)))
        for c, tr in enumerate(trs):
            cfg1 = ssd.default_config(gm.W, gm.H, max_frames_per_batch=1)
            one = Resident(ssd, gpu_device, cfg1, tr, [per_cam[c]])
            try:
                res1 = one.detect()
                recs1, masks1 = one.clear(cm.RULE)
                for i in (i for i, o in enumerate(order) if o == c):
                    assert bytes(res[i]) == bytes(res1[0]) and bytes(recs[i]) == bytes(recs1[0]) and np.array_equal(masks[i], masks1[0]), (c, i)
            finally:
                one.close()
        # the same frames from host memory through ssd_process_host_cameras_clearance: the resident pass's bytes, each frame solved
        # against its own camera
        res_h, out_h, mom_h, mask_h = r.det.process_host_cameras_clearance(np.stack(frames), order, cm.rule_of(ssd, cm.RULE), moments=True, mask=True)
        for i in range(len(frames)):
            assert bytes(res_h[i]) == bytes(res[i]) and bytes(mom_h[i]) == bytes(recs[i]) and np.array_equal(mask_h[i].reshape(-1), masks[i]), i
            assert bytes(out_h[i]) == bytes(ssd.clearance_solve(recs[i], res[i], trs[order[i]].constants, 50)) and out_h[i].s[1].status == ssd.CL_OCCUPIED, i
        r.detect()
        # the one-calibration entry point refuses a cameras batch, and ssd_set_cameras withdraws it
        L = ssd.lib()
        rule = ssd.ClearanceRule()
        args = (r.src.ptr, r.stride, r.n, None, 0, C.byref(rule), r.out.ptr, None, 0)
        assert L.ssd_enqueue_clearance(r.det._h, *args) == -1 and b"cameras batch" in L.ssd_last_error()
        r.det.set_cameras(cams)
        assert L.ssd_enqueue_cameras_clearance(r.det._h, *args) == -1 and b"no whole cameras enqueue" in L.ssd_last_error()
    finally:
        r.close()


def test_a_host_call_of_two_slices_against_the_resident_pass(ssd, oracle, gpu_device):
    """33 frames through ssd_process_host_clearance (slices of 32 and 1) against ssd_process_host and the resident pass"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    frames = [frames[i % len(frames)] for i in range(33)]
    cfg = ssd.default_config(gm.W, gm.H, max_frames_per_batch=32)
    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        plain = det.process_host(np.stack(frames))
        res, out, mom, mask = det.process_host_clearance(np.stack(frames), cm.rule_of(ssd, cm.RULE), moments=True, mask=True)
        assert [bytes(x) for x in res] == [bytes(x) for x in plain]
        res_b, out_b = det.process_host_clearance(np.stack(frames))
        assert [bytes(x) for x in out_b] == [bytes(x) for x in out]
    finally:
        det.close()
    cfg5 = ssd.default_config(gm.W, gm.H, max_frames_per_batch=5)
    r = Resident(ssd, gpu_device, cfg5, trans, frames[:5])
    try:
        res5 = r.detect()
        recs, masks = r.clear(cm.RULE)
        r.check(cm.RULE, recs, masks)
    finally:
        r.close()
    for i in range(33):
        assert bytes(res[i]) == bytes(res5[i % 5]) and bytes(mom[i]) == bytes(recs[i % 5]) and np.array_equal(mask[i].reshape(-1), masks[i % 5]), i
        assert bytes(out[i]) == bytes(ssd.clearance_solve(mom[i], res[i], trans.constants, 50)), i
    assert [out[i].s[1].status for i in range(5)] == [1, 0, 1, 0, 0] and [out[i].s[2].status for i in range(5)] == [0, 1, 0, 1, 0]


def test_every_refusal_and_what_the_pass_leaves_alone(ssd, oracle, gpu_device):
    """SSD_E_ARG before anything is launched (the poisoned buffers stay poison), the withdrawal by ssd_set_intrinsics; results, risers,
    labels and debug records are the same bytes with and without the pass; ssd_workspace_bytes is unchanged"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    frames = frames[:2]
    cfg.max_frames_per_batch = 2
    L = ssd.lib()
    r = Resident(ssd, gpu_device, cfg, trans, frames)
    try:
        det, wh = r.det, r.wh
        rule = ssd.ClearanceRule()
        ms = C.c_float(0.0)

        def call(ptr=r.src.ptr, stride=r.stride, n=2, inp=0, rule=rule, out=r.out.ptr, mask=r.mask.ptr, mstride=r.mstride, fn=L.ssd_enqueue_clearance):
            return fn(det._h, ptr, stride, n, None, inp, C.byref(rule) if rule else None, out, mask, mstride)

        def refused(match, **kw):
            assert call(**kw) == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        r.out.upload(np.full(r.rec * 3, POISON, dtype=np.uint8))
        r.mask.upload(np.full(r.mstride * 3, POISON, dtype=np.uint8))
        refused(b"no whole enqueue")                                   # nothing enqueued yet
        assert L.ssd_fetch_clearance(det._h, None) == -1 and L.ssd_get_clearance_time(det._h, C.byref(ms)) == -1
        before = det.workspace_bytes
        det.set_risers(True, tolerance=0.03, min_support=200)
        det.set_debug(True, images=False)
        lab = ssd.DeviceBuffer(wh * 2, gpu_device)
        r.bufs.append(lab)
        det.enqueue_labels(r.src.ptr, 2, lab.ptr, stride_bytes=r.stride)
        res = det.fetch_list(2)
        kept = dict(res=[bytes(x) for x in res], risers=[bytes(x) for x in det.fetch_risers(2)], labels=lab.download(wh * 2).tobytes(),
                    debug=[bytes(det.debug(i)) for i in range(2)])
        grown = det.workspace_bytes
        refused(b"null", rule=None)
        refused(b"null", out=None)
        refused(b"null", ptr=None)
        refused(b"mask_stride", mstride=wh - 1)
        for bad in ((-0.01, 0.03, 0.5), (1.5, 0.03, 0.5), (0.03, 0.0, 0.5), (0.03, 1.5, 0.5), (0.03, 0.03, 0.03), (0.03, 0.03, 8.5), (float("nan"), 0.03, 0.5)):
            refused(b"rule", rule=ssd.ClearanceRule(*bad))
        refused(b"nframes", n=1)
        refused(b"not the last enqueue's", stride=r.stride + 4)
        refused(b"not the last enqueue's", ptr=r.src.ptr + r.stride)
        refused(b"input must be", inp=2)
        refused(b"ssd_set_intrinsics", inp=1)
        refused(b"one-calibration batch", fn=L.ssd_enqueue_cameras_clearance)
        assert np.all(r.out.download(r.rec * 3) == POISON) and np.all(r.mask.download(r.mstride * 3) == POISON), "a refused call wrote something"
        assert call(mask=None, mstride=0) == 0                         # no mask: its stride is not looked at
        det.fetch_clearance()
        assert det.clearance_time_ms() == 0.0, "timing is off"
        recs, masks = r.clear(cm.RULE)
        res_now = det.fetch_list(2)
        r.check(cm.RULE, recs, masks, res=res_now)
        now = dict(res=[bytes(x) for x in res_now], risers=[bytes(x) for x in det.fetch_risers(2)], labels=lab.download(wh * 2).tobytes(),
                   debug=[bytes(det.debug(i)) for i in range(2)])
        assert now == kept, "results, risers, labels and debug records are the same bytes with and without the pass"
        assert det.workspace_bytes == grown and grown >= before
        # a timed pass
        det.set_timing(True)
        det.enqueue_labels(r.src.ptr, 2, lab.ptr, stride_bytes=r.stride)
        det.fetch_list(2)
        r.clear(cm.RULE)
        assert det.clearance_time_ms() > 0.0
        assert det.workspace_bytes == grown, "the pass made events only"
        # a partial run is no whole enqueue; ssd_set_intrinsics withdraws one
        det.set_debug(False)
        det.set_risers(False)
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride, stages=ssd.STAGE_ALL & ~64)
        refused(b"no whole enqueue")
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride)
        det.fetch_list(2)
        assert call() == 0
        det.fetch_clearance()
        det.set_intrinsics(intr)
        refused(b"no whole enqueue")
    finally:
        r.close()
