"""The tread grid on the GPU (k_tread_grid, k_tread_grid_cams; include/ssd_hip.h): the device's records byte for
byte ssd_tread_grid_host on the handle's OWN fetched result, the occupant identity against the device's own clearance records, and the
entry points' contract.  Every pass runs into a poisoned buffer with one record of poison behind the batch, the frames at a stride that is
no multiple of 16.  No tolerance anywhere: the counts and maxima are integers and the decisions are one text.  Frames and the resident
harness: tests/test_gpu_clearance.py's and tests/clearance_model.py's."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as cm
import clouds
import full_width as fw
import ground_model as gm
import oracle_binding as ob
import tread_grid_model as tg
from test_gpu_clearance import NO_PLANES, POISON, SINGLE_PASS, TWO_PASSES, Resident, _kept, _scene_batch, _wide_frames
from test_labels import expected_labels

pytestmark = pytest.mark.gpu


class GridResident(Resident):
    """test_gpu_clearance's resident frames, with the tread grid pass into a freshly poisoned buffer of one record more than the batch"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.grec = C.sizeof(self.ssd.FrameTreadGrid)
        self.gout = self.ssd.DeviceBuffer(self.grec * (self.n + 1), self.device)
        self.bufs.append(self.gout)

    def grid(self, rule, n=None):
        """the pass behind the last enqueue -> the records; checks the poison behind them"""
        n = self.n if n is None else n
        self.gout.upload(np.full(self.grec * (self.n + 1), POISON, dtype=np.uint8))
        self.det.enqueue_tread_grid(self.src.ptr, n, self.gout.ptr, tg.rule_of(self.ssd, rule), depth=self.depth, stride_bytes=self.stride,
                                    cameras=self.order is not None)
        self.det.fetch_tread_grid()
        raw = self.gout.download(self.grec * (self.n + 1))
        assert np.all(raw[self.grec * n:] == POISON), "a record past nframes was written"
        return list((self.ssd.FrameTreadGrid * n).from_buffer_copy(raw[:self.grec * n].tobytes()))

    def check_grid(self, rule, recs, res=None, frames=None, ground=None):
        """records byte for byte the host's on the handle's own results; ground: as Resident.check's"""
        ssd, res, frames = self.ssd, res or self.res, frames or self.frames
        for i, r in enumerate(recs):
            live = res[i].n_steps > 0 and not (res[i].status & ssd.ST_THROW)
            flag = (1 if live else 0) if ground is None else ground[i]
            want = ssd.tread_grid_host(self.cfg, self.cal_of(i), frames[i], res[i], flag, tg.rule_of(ssd, rule), intr=self.intr_of(i))
            if bytes(r) != bytes(want):
                bad = [k for k in range(ssd.MAX_STEPS) if not tg.same_grid(tg.grid_of_record(r, k), tg.grid_of_record(want, k))]
                raise AssertionError((i, (r.n_surfaces, r.ground), (want.n_surfaces, want.ground), bad))

    def identity(self, rule, recs, clear):
        """sum(occ) + n_occ_out = n + n_far of the device's own clearance record for the same rule"""
        for r, c in zip(recs, clear):
            for k in range(self.ssd.MAX_STEPS):
                g = tg.grid_of_record(r, k)
                assert int(g["occ"].sum()) + g["n_occ_out"] == _kept(c, k), k


def _totals(rec, k):
    g = tg.grid_of_record(rec, k)
    return int(g["seen"].sum()) + g["n_seen_out"], int(g["occ"].sum()) + g["n_occ_out"]


@pytest.mark.parametrize("depth", [False, True])
def test_the_scenes_with_a_patch_equal_the_host(ssd, oracle, gpu_device, depth):
    """vertices and 16-bit depth; the pass repeated with another rule and another cell, and with a cell at each end of its range; the
    identity against the device's clearance pass; results and workspace bytes untouched"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, depth)
    cfg.max_frames_per_batch = len(frames)
    r = GridResident(ssd, gpu_device, cfg, trans, frames, depth=depth, intr=intr)
    try:
        res = r.detect()
        before = r.det.workspace_bytes
        assert all(x.n_steps == 3 and not (x.status & ssd.ST_THROW) for x in res)
        recs = r.grid(tg.RULE)
        r.check_grid(tg.RULE, recs)
        clear, _ = r.clear(tg.RULE[:3], mask=False)
        r.identity(tg.RULE, recs, clear)
        for i, (surface, sel) in enumerate(pulled):
            assert all(_totals(recs[i], k)[0] > 1000 for k in range(3)), "nearly every point of a tread is a tread point"
            if surface is None:
                assert all(_totals(recs[i], k)[1] == 0 for k in range(ssd.MAX_STEPS)), "the clean frame holds nothing"
            else:
                assert _totals(recs[i], surface)[1] >= 50 and tg.grid_of_record(recs[i], surface)["top"].max() > 0.03 * 65536
        # again with another rule and another cell (no margin: the riser faces leak in; the grid is too shallow for the tread)
        rule0 = (0.0, 0.02, 0.4, 0.02)
        recs0 = r.grid(rule0)
        r.check_grid(rule0, recs0)
        clear0, _ = r.clear(rule0[:3], mask=False)
        r.identity(rule0, recs0, clear0)
        assert recs0[-1].s[1].n_seen_out > 0 and max(_totals(recs0[-1], k)[1] for k in range(3)) > 500
        # a cell at each end of the range: everything outside the grid but a corner / everything in one cell
        for cell in (0.005, 1.0):
            rule = tg.RULE[:3] + (cell,)
            got = r.grid(rule)
            r.check_grid(rule, got)
            assert [_totals(got[i], k) for i in range(r.n) for k in range(3)] == [_totals(recs[i], k) for i in range(r.n) for k in range(3)]
        assert all(np.count_nonzero(tg.grid_of_record(got[-1], k)["seen"]) == 1 for k in range(3)), "a cell of 1 m holds the tread"
        again = r.grid(tg.RULE)
        assert [bytes(x) for x in again] == [bytes(x) for x in recs]
        assert r.det.workspace_bytes == before, "the pass allocates nothing that counts"
        assert [bytes(x) for x in r.det.fetch_list(r.n)] == [bytes(x) for x in res], "the results are still the enqueue's"
    finally:
        r.close()


@pytest.mark.parametrize("mode", [TWO_PASSES, SINGLE_PASS, NO_PLANES], ids=["two-passes", "single-pass", "no-planes"])
def test_the_full_width_batch_in_all_three_k1_modes(ssd, oracle, gpu_device, mode):
    refs, frames = _wide_frames(ssd, oracle)
    cfg = ssd.default_config(fw.W, fw.H, max_frames_per_batch=len(frames))
    r = GridResident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames, mode=mode)
    try:
        res = r.detect()
        assert [x.n_steps for x in res] == [17] * 5 + [9, res[-1].n_steps] and res[-1].n_steps <= 1
        recs = r.grid(tg.WIDE_RULE)
        r.check_grid(tg.WIDE_RULE, recs)
        clear, _ = r.clear(tg.WIDE_RULE[:3], mask=False)
        r.identity(tg.WIDE_RULE, recs, clear)
        for i in range(4):                                             # the layouts that hold every point of the frame
            assert min(_totals(recs[i], k)[1] for k in range(17)) >= 100 and min(_totals(recs[i], k)[0] for k in range(17)) > 0
        assert len({bytes(x) for x in recs[:4]}) == 1, "the layouts of one frame place the same points: one record"
    finally:
        r.close()


def test_the_ragged_frame(ssd, oracle, gpu_device):
    """642 x 479: no multiple of 4 or of 64 (the 12-byte load path, a partial last cell)"""
    w, h = 642, 479
    refs, frames = _wide_frames(ssd, oracle, w, h, ("scatter", "sparse", "lanes"))
    cfg = ssd.default_config(w, h, max_frames_per_batch=len(frames))
    r = GridResident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames)
    try:
        res = r.detect()
        assert [x.n_steps for x in res] == [17] * 3
        recs = r.grid(tg.WIDE_RULE)
        r.check_grid(tg.WIDE_RULE, recs)
        assert all(min(_totals(recs[i], k)[0] for k in range(17)) > 0 for i in (0, 2))
    finally:
        r.close()


def test_three_workspaces_and_a_wider_batch_before(ssd, oracle, gpu_device):
    """three workspaces: each pass behind its own batch; then, on one handle, a pass behind a batch of two frames after one of seven"""
    refs, frames = _wide_frames(ssd, oracle)
    cfg = ssd.default_config(fw.W, fw.H, max_frames_per_batch=len(frames), batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    r = GridResident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames)
    try:
        want = None
        for turn in range(4):                                          # every workspace, and the first one again
            r.detect()
            recs = r.grid(tg.WIDE_RULE)
            if turn == 0:
                r.check_grid(tg.WIDE_RULE, recs)
            want = want or [bytes(x) for x in recs]
            assert [bytes(x) for x in recs] == want
        res2 = r.detect(2)
        recs = r.grid(tg.WIDE_RULE, n=2)
        r.check_grid(tg.WIDE_RULE, recs, res=res2)
        assert [bytes(x) for x in recs] == want[:2]
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
    r = GridResident(ssd, gpu_device, cfg, trs[0], frames, cameras=cams, order=order)
    r.cameras_cal = [tr.constants for tr in trs]
    try:
        res = r.detect()
        recs = r.grid(tg.RULE)
        r.check_grid(tg.RULE, recs)
        assert all(_totals(recs[i], 1)[1] >= 285 for i in range(len(frames)))
        for c, tr in enumerate(trs):
            cfg1 = ssd.default_config(gm.W, gm.H, max_frames_per_batch=1)
            one = GridResident(ssd, gpu_device, cfg1, tr, [per_cam[c]])
            try:
                res1 = one.detect()
                recs1 = one.grid(tg.RULE)
                for i in (i for i, o in enumerate(order) if o == c):
                    assert bytes(res[i]) == bytes(res1[0]) and bytes(recs[i]) == bytes(recs1[0]), (c, i)
            finally:
                one.close()
        # the same frames from host memory through ssd_process_host_cameras_tread_grid: the resident pass's bytes, each frame solved
        rule = tg.rule_of(ssd, tg.RULE)
        res_h, out_h, grids_h = r.det.process_host_cameras_tread_grid(np.stack(frames), order, rule, 3, 3, 0.2, 0.1, grids=True)
        for i in range(len(frames)):
            assert bytes(res_h[i]) == bytes(res[i]) and bytes(grids_h[i]) == bytes(recs[i]), i
            assert bytes(out_h[i]) == bytes(ssd.tread_grid_solve(recs[i], res[i], rule, 3, 3, 0.2, 0.1)) and out_h[i].s[1].n_occupied >= 1, i
        r.detect()
        # the one-calibration entry point refuses a cameras batch, and ssd_set_cameras withdraws it
        L = ssd.lib()
        args = (r.src.ptr, r.stride, r.n, None, 0, C.byref(rule), r.gout.ptr)
        assert L.ssd_enqueue_tread_grid(r.det._h, *args) == -1 and b"cameras batch" in L.ssd_last_error()
        r.det.set_cameras(cams)
        assert L.ssd_enqueue_cameras_tread_grid(r.det._h, *args) == -1 and b"no whole cameras enqueue" in L.ssd_last_error()
    finally:
        r.close()


def test_a_host_call_of_two_slices_against_the_resident_pass(ssd, oracle, gpu_device):
    """33 frames through ssd_process_host_tread_grid (slices of 32 and 1) against ssd_process_host and the resident pass.  A slice's records
    (32 x 52.5 KB) are more than the 256 x 192 bytes per frame the label staging buffers would hold: the pass stages them in its own"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    frames = [frames[i % len(frames)] for i in range(33)]
    cfg = ssd.default_config(gm.W, gm.H, max_frames_per_batch=32)
    rule = tg.rule_of(ssd, tg.RULE)
    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        plain = det.process_host(np.stack(frames))
        labelled = det.process_host_clearance(np.stack(frames[:2]), mask=True)            # makes the label staging buffers, small ones
        res, out, grids = det.process_host_tread_grid(np.stack(frames), rule, 3, 3, 0.2, 0.1, grids=True)
        assert [bytes(x) for x in res] == [bytes(x) for x in plain]
        res_b, out_b = det.process_host_tread_grid(np.stack(frames), rule, 3, 3, 0.2, 0.1)
        assert [bytes(x) for x in out_b] == [bytes(x) for x in out]
    finally:
        det.close()
    cfg5 = ssd.default_config(gm.W, gm.H, max_frames_per_batch=5)
    r = GridResident(ssd, gpu_device, cfg5, trans, frames[:5])
    try:
        res5 = r.detect()
        recs = r.grid(tg.RULE)
        r.check_grid(tg.RULE, recs)
    finally:
        r.close()
    for i in range(33):
        assert bytes(res[i]) == bytes(res5[i % 5]) and bytes(grids[i]) == bytes(recs[i % 5]), i
        assert bytes(out[i]) == bytes(ssd.tread_grid_solve(grids[i], res[i], rule, 3, 3, 0.2, 0.1)), i
    assert [out[i].s[1].n_occupied > 0 for i in range(5)] == [True, False, True, False, False]
    assert all(out[4].s[k].foothold == 1 and out[4].s[k].n_occupied == 0 for k in range(3)), "the clean frame: a foothold on every tread"


def test_every_refusal_and_what_the_pass_leaves_alone(ssd, oracle, gpu_device):
    """SSD_E_ARG before anything is launched (the poisoned buffer stays poison), the withdrawal by ssd_set_intrinsics; results, risers,
    labels, clearance records and debug records are the same bytes with and without the pass; ssd_workspace_bytes is unchanged"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    frames = frames[:2]
    cfg.max_frames_per_batch = 2
    L = ssd.lib()
    r = GridResident(ssd, gpu_device, cfg, trans, frames)
    try:
        det, wh = r.det, r.wh
        rule = ssd.TreadGridRule()
        ms = C.c_float(0.0)

        def call(ptr=r.src.ptr, stride=r.stride, n=2, inp=0, rule=rule, out=r.gout.ptr, fn=L.ssd_enqueue_tread_grid):
            return fn(det._h, ptr, stride, n, None, inp, C.byref(rule) if rule else None, out)

        def refused(match, **kw):
            assert call(**kw) == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        r.gout.upload(np.full(r.grec * 3, POISON, dtype=np.uint8))
        refused(b"no whole enqueue")                                   # nothing enqueued yet
        assert L.ssd_fetch_tread_grid(det._h, None) == -1 and L.ssd_get_tread_grid_time(det._h, C.byref(ms)) == -1
        before = det.workspace_bytes
        det.set_risers(True, tolerance=0.03, min_support=200)
        det.set_debug(True, images=False)
        lab = ssd.DeviceBuffer(wh * 2, gpu_device)
        r.bufs.append(lab)
        det.enqueue_labels(r.src.ptr, 2, lab.ptr, stride_bytes=r.stride)
        res = det.fetch_list(2)
        clear, masks = r.clear(cm.RULE)

        def outputs():
            return dict(res=[bytes(x) for x in det.fetch_list(2)], risers=[bytes(x) for x in det.fetch_risers(2)], labels=lab.download(wh * 2).tobytes(),
                        debug=[bytes(det.debug(i)) for i in range(2)], clear=r.out.download(r.rec * 3).tobytes(),
                        mask=r.mask.download(r.mstride * 3).tobytes())

        kept = outputs()
        grown = det.workspace_bytes
        refused(b"null", rule=None)
        refused(b"null", out=None)
        refused(b"null", ptr=None)
        for bad in ((-0.01, 0.03, 0.5, 0.02), (1.5, 0.03, 0.5, 0.02), (0.03, 0.0, 0.5, 0.02), (0.03, 1.5, 0.5, 0.02), (0.03, 0.03, 0.03, 0.02),
                    (0.03, 0.03, 8.5, 0.02), (float("nan"), 0.03, 0.5, 0.02), (0.03, 0.03, 0.5, 0.004), (0.03, 0.03, 0.5, 1.5), (0.03, 0.03, 0.5, float("nan"))):
            refused(b"rule", rule=ssd.TreadGridRule(*bad))
        refused(b"nframes", n=1)
        refused(b"not the last enqueue's", stride=r.stride + 4)
        refused(b"not the last enqueue's", ptr=r.src.ptr + r.stride)
        refused(b"input must be", inp=2)
        refused(b"ssd_set_intrinsics", inp=1)
        refused(b"one-calibration batch", fn=L.ssd_enqueue_cameras_tread_grid)
        assert np.all(r.gout.download(r.grec * 3) == POISON), "a refused call wrote something"
        assert call() == 0
        det.fetch_tread_grid()
        assert det.tread_grid_time_ms() == 0.0, "timing is off"
        recs = r.grid(tg.RULE)
        r.check_grid(tg.RULE, recs, res=res)
        r.identity(tg.RULE, recs, clear)
        assert outputs() == kept, "results, risers, labels, clearance and debug records are the same bytes with and without the pass"
        assert det.workspace_bytes == grown and grown >= before
        # a timed pass
        det.set_timing(True)
        det.enqueue_labels(r.src.ptr, 2, lab.ptr, stride_bytes=r.stride)
        det.fetch_list(2)
        r.grid(tg.RULE)
        assert det.tread_grid_time_ms() > 0.0
        assert det.workspace_bytes == grown, "the pass made events only"
        # a partial run is no whole enqueue; ssd_set_intrinsics withdraws one
        det.set_debug(False)
        det.set_risers(False)
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride, stages=ssd.STAGE_ALL & ~64)
        refused(b"no whole enqueue")
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride)
        det.fetch_list(2)
        assert call() == 0
        det.fetch_tread_grid()
        det.set_intrinsics(intr)
        refused(b"no whole enqueue")
    finally:
        r.close()
