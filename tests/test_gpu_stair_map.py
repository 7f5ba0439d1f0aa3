"""The stair map on the GPU (k_stair_map, k_stair_map_cams; include/ssd_hip.h): the record of every map byte for
byte the fold, by ssd_tread_grid_add, of ssd_tread_grid_host over the frames that name the map, each against the MAP's staircase under
its own calibration - never the frame's own result.  Every pass runs into a poisoned buffer with one record of poison behind nmaps, the
frames at a stride that is no multiple of 16.  No tolerance anywhere: the counts and maxima are integers and the decisions are one text.
Frames and the resident harness: tests/test_gpu_tread_grid.py's."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as cm
import clouds
import full_width as fw
import ground_model as gm
import oracle_binding as ob
import tread_grid_model as tg
from test_gpu_clearance import NO_PLANES, POISON, SINGLE_PASS, TWO_PASSES, _scene_batch, _wide_frames
from test_gpu_follow_passes import two_streams                          # noqa: F401 (a fixture)
from test_gpu_tread_grid import GridResident
from test_labels import expected_labels

pytestmark = pytest.mark.gpu

NONE = 0xffff


def header_of(ssd, m):
    """what ssd_tread_grid_host writes into the header for a map's staircase"""
    n = 0 if (m.stairs.status & ssd.ST_THROW) else m.stairs.n_steps
    return n, 1 if (n > 0 and m.ground) else 0


def stair_map(ssd, result, ground=1):
    m = ssd.StairMap()
    C.memmove(C.byref(m.stairs), C.byref(result), C.sizeof(ssd.FrameResult))
    m.ground = ground
    return m


class MapResident(GridResident):
    """GridResident with the stair map pass into a freshly poisoned buffer of one record more than the maps"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.mout = self.ssd.DeviceBuffer(self.grec * (self.ssd.MAX_STAIR_MAPS + 1), self.device)
        self.bufs.append(self.mout)

    def poison(self, nmaps):
        self.mout.upload(np.full(self.grec * (nmaps + 1), POISON, dtype=np.uint8))

    def download(self, nmaps):
        raw = self.mout.download(self.grec * (nmaps + 1))
        assert np.all(raw[self.grec * nmaps:] == POISON), "a record past nmaps was written"
        return list((self.ssd.FrameTreadGrid * nmaps).from_buffer_copy(raw[:self.grec * nmaps].tobytes()))

    def fold(self, maps, rule, index=None, n=None, accumulate=False, stream=None):
        """the pass behind the last enqueue -> the nmaps records; checks the poison behind them"""
        n = self.n if n is None else n
        if not accumulate:
            self.poison(len(maps))
        self.det.enqueue_stair_map(self.src.ptr, n, maps, self.mout.ptr, index, tg.rule_of(self.ssd, rule), accumulate, depth=self.depth,
                                   stride_bytes=self.stride, stream=stream, cameras=self.order is not None)
        self.det.fetch_stair_map()
        return self.download(len(maps))

    def want(self, maps, rule, index=None, n=None, times=1, frames=None):
        """the fold of the host function over the frames that name each map, `times` times over"""
        ssd, n, frames = self.ssd, self.n if n is None else n, frames or self.frames
        out = []
        for m, sm in enumerate(maps):
            acc = ssd.FrameTreadGrid()
            acc.n_surfaces, acc.ground = header_of(ssd, sm)
            for i in range(n):
                if (0 if index is None else index[i]) != m:
                    continue
                g = ssd.tread_grid_host(self.cfg, self.cal_of(i), frames[i], sm.stairs, sm.ground, tg.rule_of(ssd, rule), intr=self.intr_of(i))
                assert (g.n_surfaces, g.ground) == (acc.n_surfaces, acc.ground)
                for _ in range(times):
                    ssd.tread_grid_add(g, acc)
            out.append(acc)
        return out

    def check(self, got, want):
        assert len(got) == len(want)
        for m, (g, w) in enumerate(zip(got, want)):
            if bytes(g) != bytes(w):
                bad = [k for k in range(self.ssd.MAX_STEPS) if not tg.same_grid(tg.grid_of_record(g, k), tg.grid_of_record(w, k))]
                raise AssertionError((m, (g.n_surfaces, g.ground), (w.n_surfaces, w.ground), bad))


def _seen(rec, k):
    g = tg.grid_of_record(rec, k)
    return int(g["seen"].sum()) + g["n_seen_out"]


@pytest.fixture(scope="module")
def wide(ssd, oracle):
    return _wide_frames(ssd, oracle)


@pytest.mark.parametrize("depth", [False, True])
def test_the_scene_frames_fold_into_the_maps_they_name(ssd, oracle, gpu_device, depth):
    """one map for all five frames; three maps mixed with SSD_STAIR_MAP_NONE, one of which nobody names; accumulate; no index; another rule
    and cell; what the handle's other outputs are; ssd_workspace_bytes moves on the first call only"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, depth)
    cfg.max_frames_per_batch = len(frames)
    r = MapResident(ssd, gpu_device, cfg, trans, frames, depth=depth, intr=intr)
    try:
        res = r.detect()
        grids = r.grid(tg.RULE)
        clear, _ = r.clear(tg.RULE[:3], mask=False)
        before = r.det.workspace_bytes
        clean = stair_map(ssd, res[4])
        got = r.fold([clean], tg.RULE)
        grown = r.det.workspace_bytes
        assert grown > before, "the maps and the index are counted from the first call on"
        one = r.want([clean], tg.RULE)
        r.check(got, one)
        assert (got[0].n_surfaces, got[0].ground) == (3, 1) and all(_seen(got[0], k) > 5000 for k in range(3)), "five frames' tread points"
        # three maps: the clean frame's, another frame's, and one nobody names
        maps = [clean, stair_map(ssd, res[1], ground=0), stair_map(ssd, res[3])]
        index = [0, NONE, 1, 0, 1]
        got3 = r.fold(maps, tg.RULE, index)
        want3 = r.want(maps, tg.RULE, index)
        r.check(got3, want3)
        assert (got3[1].ground, got3[2].n_surfaces, got3[2].ground) == (0, 3, 1)
        assert bytes(got3[2])[8:] == bytes(len(bytes(got3[2])) - 8), "a map no frame names: the header and zeros"
        # the call again on top: every count doubles, every top stays
        twice = r.fold(maps, tg.RULE, index, accumulate=True)
        r.check(twice, r.want(maps, tg.RULE, index, times=2))
        for a, b in zip(got3, twice):
            for k in range(3):
                ga, gb = tg.grid_of_record(a, k), tg.grid_of_record(b, k)
                assert np.array_equal(2 * ga["seen"], gb["seen"]) and np.array_equal(2 * ga["occ"], gb["occ"]) and np.array_equal(ga["top"], gb["top"])
        # no index: every frame names map 0, whatever else is in the table
        r.check(r.fold(maps, tg.RULE), r.want(maps, tg.RULE, [0] * 5))
        # another rule and another cell
        rule0 = (0.0, 0.02, 0.4, 0.02)
        r.check(r.fold(maps, rule0, index), r.want(maps, rule0, index))
        r.check(r.fold([clean], tg.RULE), one)
        # a map that threw and an empty one: all zero, header included
        thrown = stair_map(ssd, res[4])
        thrown.stairs.status |= ssd.ST_THROW
        empty = ssd.StairMap()
        empty.ground = 1
        dead = r.fold([thrown, empty, clean], tg.RULE, [0, 1, 2, 0, 1])
        r.check(dead, r.want([thrown, empty, clean], tg.RULE, [0, 1, 2, 0, 1]))
        assert bytes(dead[0]) == bytes(dead[1]) == bytes(len(bytes(dead[0])))
        assert r.det.workspace_bytes == grown, "ssd_workspace_bytes moves on the first call only"
        assert [bytes(x) for x in r.det.fetch_list(r.n)] == [bytes(x) for x in res], "the results are still the enqueue's"
        assert [bytes(x) for x in r.grid(tg.RULE)] == [bytes(x) for x in grids], "the tread grid's records are what they were"
        assert [bytes(x) for x in r.clear(tg.RULE[:3], mask=False)[0]] == [bytes(x) for x in clear]
    finally:
        r.close()


@pytest.mark.parametrize("mode", [TWO_PASSES, SINGLE_PASS, NO_PLANES], ids=["two-passes", "single-pass", "no-planes"])
def test_the_full_width_batch_in_all_three_k1_modes(ssd, oracle, gpu_device, wide, mode):
    """17 surfaces, seven frames into one map - the last frame finds at most one step of its own and still contributes -, then two maps
    (17 and 9 surfaces) with the frames dealt alternately"""
    refs, frames = wide
    cfg = ssd.default_config(fw.W, fw.H, max_frames_per_batch=len(frames))
    r = MapResident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames, mode=mode)
    try:
        res = r.detect()
        assert [x.n_steps for x in res] == [17] * 5 + [9, res[-1].n_steps] and res[-1].n_steps <= 1
        m17, m9 = stair_map(ssd, res[0]), stair_map(ssd, res[5])
        got = r.fold([m17], tg.WIDE_RULE)
        r.check(got, r.want([m17], tg.WIDE_RULE))
        alone = r.want([m17], tg.WIDE_RULE, [NONE] * 6 + [0])
        assert sum(_seen(alone[0], k) for k in range(17)) > 0, "the frame too poor for a detection of its own adds its points to the map"
        assert min(_seen(got[0], k) for k in range(17)) > 0
        index = [0, 1, 0, 1, 0, 1, 0]
        got2 = r.fold([m17, m9], tg.WIDE_RULE, index)
        r.check(got2, r.want([m17, m9], tg.WIDE_RULE, index))
        assert (got2[0].n_surfaces, got2[1].n_surfaces) == (17, 9)
    finally:
        r.close()


def test_the_ragged_frames(ssd, oracle, gpu_device):
    """642 x 479: no multiple of 4 or of 64 (the 12-byte load path, a partial last cell)"""
    w, h = 642, 479
    refs, frames = _wide_frames(ssd, oracle, w, h, ("scatter", "sparse", "lanes"))
    cfg = ssd.default_config(w, h, max_frames_per_batch=len(frames))
    r = MapResident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames)
    try:
        res = r.detect()
        assert [x.n_steps for x in res] == [17] * 3
        maps, index = [stair_map(ssd, res[0]), stair_map(ssd, res[1])], [1, 0, 0]
        got = r.fold(maps, tg.WIDE_RULE, index)
        r.check(got, r.want(maps, tg.WIDE_RULE, index))
        assert min(_seen(got[0], k) for k in range(17)) > 0
    finally:
        r.close()


def test_three_workspaces_and_a_wider_batch_before(ssd, oracle, gpu_device, wide):
    """three workspaces: each pass behind its own batch; then, on one handle, a pass behind a batch of two frames after one of seven"""
    refs, frames = wide
    cfg = ssd.default_config(fw.W, fw.H, max_frames_per_batch=len(frames), batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    r = MapResident(ssd, gpu_device, cfg, clouds.calibration(ssd, clouds.Z_SHIFT), frames)
    try:
        index, want = [0, 1, 0, 1, 0, 1, 0], None
        for turn in range(4):                                          # every workspace, and the first one again
            res = r.detect()
            maps = [stair_map(ssd, res[0]), stair_map(ssd, res[5])]
            got = r.fold(maps, tg.WIDE_RULE, index)
            want = want or r.want(maps, tg.WIDE_RULE, index)
            r.check(got, want)
        r.detect(2)
        got = r.fold(maps, tg.WIDE_RULE, [1, 0], n=2)
        r.check(got, r.want(maps, tg.WIDE_RULE, [1, 0], n=2))
    finally:
        r.close()


def test_a_cameras_batch_against_one_map_from_camera_0(ssd, oracle, gpu_device):
    """three cameras (poses a little apart), frames in mixed order, one map in the world they share: the record is the fold of the host
    function per frame under its own camera, and the tread_grid_add of three one-camera handles' records"""
    poses = [dict(), dict(pitch_deg=52.0), dict(cam_height=1.05, roll_deg=1.0)]
    scs = [gm.scene(ssd, "steps", seed=7 + c, **kw) for c, kw in enumerate(poses)]
    cfg0 = ssd.default_config(gm.W, gm.H)
    trs = [ssd.transformation_for_scene(sc) for sc in scs]
    cams = [ssd.Camera() for _ in scs]
    for cam, tr in zip(cams, trs):
        cam.cal = tr.constants
    order = [2, 0, 1, 1, 2, 0]
    per_cam, own = [], []
    for sc, tr in zip(scs, trs):
        frame = ssd.synth_host([sc])[0]
        res = oracle.process(ob.to_oracle_config(cfg0), ob.to_oracle_calibration(tr.constants), frame)[0]
        fr = cm.result_of_oracle(ssd, res)
        own.append(fr)
        per_cam.append(cm.patched(cfg0, tr.constants, fr, frame, expected_labels(oracle, cfg0, tr.constants, res, frame), 1)[0])
    frames = [per_cam[c] for c in order]
    cfg = ssd.default_config(gm.W, gm.H, max_frames_per_batch=len(frames))
    r = MapResident(ssd, gpu_device, cfg, trs[0], frames, cameras=cams, order=order)
    r.cameras_cal = [tr.constants for tr in trs]
    try:
        res = r.detect()
        m = stair_map(ssd, own[0])                                     # camera 0's clean staircase
        got = r.fold([m], tg.RULE)
        r.check(got, r.want([m], tg.RULE))
        assert int(tg.grid_of_record(got[0], 1)["occ"].sum()) > 0, "the box on tread 1"
        acc = ssd.FrameTreadGrid()
        for c, tr in enumerate(trs):
            mine = [per_cam[c]] * order.count(c)
            cfg1 = ssd.default_config(gm.W, gm.H, max_frames_per_batch=len(mine))
            one = MapResident(ssd, gpu_device, cfg1, tr, mine)
            try:
                one.detect()
                ssd.tread_grid_add(one.fold([m], tg.RULE)[0], acc)
            finally:
                one.close()
        assert bytes(acc) == bytes(got[0])
        # the same frames from host memory through ssd_process_host_cameras_stair_map
        rule = tg.rule_of(ssd, tg.RULE)
        res_h, out_h, grids_h = r.det.process_host_cameras_stair_map(np.stack(frames), order, [m], None, rule, 3, 3, 0.2, 0.1, grids=True)
        assert [bytes(x) for x in res_h] == [bytes(x) for x in res] and bytes(grids_h[0]) == bytes(got[0])
        assert bytes(out_h[0]) == bytes(ssd.tread_grid_solve(got[0], m.stairs, rule, 3, 3, 0.2, 0.1)) and out_h[0].s[1].n_occupied >= 1
        r.detect()
        # the one-calibration entry point refuses a cameras batch, and ssd_set_cameras withdraws it
        L = ssd.lib()
        args = (r.src.ptr, r.stride, r.n, None, 0, C.byref(m), 1, None, C.byref(rule), 0, r.mout.ptr)
        assert L.ssd_enqueue_stair_map(r.det._h, *args) == -1 and b"cameras batch" in L.ssd_last_error()
        r.det.set_cameras(cams)
        assert L.ssd_enqueue_cameras_stair_map(r.det._h, *args) == -1 and b"no whole cameras enqueue" in L.ssd_last_error()
    finally:
        r.close()


def test_a_host_call_of_two_slices_against_the_resident_pass(ssd, oracle, gpu_device):
    """33 frames through ssd_process_host_stair_map (slices of 32 and 1) against ssd_process_host and the resident pass with accumulate"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    many = [frames[i % len(frames)] for i in range(33)]
    index = [(0, 1, NONE, 0, 1)[i % 5] for i in range(33)]
    rule = tg.rule_of(ssd, tg.RULE)
    cfg5 = ssd.default_config(gm.W, gm.H, max_frames_per_batch=5)
    r = MapResident(ssd, gpu_device, cfg5, trans, frames)
    try:
        res5 = r.detect()
        maps = [stair_map(ssd, res5[4]), stair_map(ssd, res5[0]), stair_map(ssd, res5[2])]
        # the resident pass: six times over the five frames, then over the first three (33 = 6 x 5 + 3)
        r.fold(maps, tg.RULE, index[:5])
        for turn in range(1, 6):
            r.fold(maps, tg.RULE, index[:5], accumulate=True)
        r.detect(3)
        resident = r.fold(maps, tg.RULE, index[30:], n=3, accumulate=True)
    finally:
        r.close()
    det = ssd.Detector(ssd.default_config(gm.W, gm.H, max_frames_per_batch=32), trans, gpu_device)
    try:
        plain = det.process_host(np.stack(many))
        res, out, grids = det.process_host_stair_map(np.stack(many), maps, index, rule, 3, 3, 0.2, 0.1, grids=True)
        res_b, out_b = det.process_host_stair_map(np.stack(many), maps, index, rule, 3, 3, 0.2, 0.1)
    finally:
        det.close()
    assert [bytes(x) for x in res] == [bytes(x) for x in plain] == [bytes(x) for x in res_b]
    assert [bytes(x) for x in grids] == [bytes(x) for x in resident]
    assert [bytes(x) for x in out_b] == [bytes(x) for x in out]
    for m in range(3):
        assert bytes(out[m]) == bytes(ssd.tread_grid_solve(grids[m], maps[m].stairs, rule, 3, 3, 0.2, 0.1)), m
    assert out[2].n_surfaces == 3 and all(out[2].s[k].n_free == 0 for k in range(3)), "the map nobody names: nothing seen"
    assert out[0].s[1].n_occupied > 0, "frame 0's box on tread 1 is in map 0"


def test_every_refusal_and_what_the_pass_leaves_alone(ssd, oracle, gpu_device):
    """SSD_E_ARG before anything is launched or copied (the poisoned buffer stays poison), the withdrawals, a partial run, the fetch and
    the time before any call, a timed pass; results, risers, labels and debug records are the same bytes with and without the pass"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    frames = frames[:2]
    cfg.max_frames_per_batch = 2
    L = ssd.lib()
    r = MapResident(ssd, gpu_device, cfg, trans, frames)
    try:
        det, wh = r.det, r.wh
        rule = tg.rule_of(ssd, tg.RULE)
        ms = C.c_float(0.0)
        m = stair_map(ssd, cm.result_of_oracle(ssd, oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(r.cal), frames[1])[0]))
        maps = (ssd.StairMap * 2)(m, m)
        idx = (C.c_uint16 * 2)(0, 1)

        def call(ptr=r.src.ptr, stride=r.stride, n=2, inp=0, maps=maps, nmaps=2, index=idx, rule=rule, acc=0, out=r.mout.ptr, fn=L.ssd_enqueue_stair_map):
            return fn(det._h, ptr, stride, n, None, inp, maps, nmaps, index, C.byref(rule) if rule else None, acc, out)

        def refused(match, **kw):
            assert call(**kw) == -1 and match in L.ssd_last_error(), L.ssd_last_error()

        r.poison(2)
        refused(b"no whole enqueue")                                   # nothing enqueued yet
        assert L.ssd_fetch_stair_map(det._h, None) == -1 and L.ssd_get_stair_map_time(det._h, C.byref(ms)) == -1
        before = det.workspace_bytes
        det.set_risers(True, tolerance=0.03, min_support=200)
        det.set_debug(True, images=False)
        lab = ssd.DeviceBuffer(wh * 2, gpu_device)
        r.bufs.append(lab)
        det.enqueue_labels(r.src.ptr, 2, lab.ptr, stride_bytes=r.stride)
        det.fetch_list(2)

        def outputs():
            return dict(res=[bytes(x) for x in det.fetch_list(2)], risers=[bytes(x) for x in det.fetch_risers(2)], labels=lab.download(wh * 2).tobytes(),
                        debug=[bytes(det.debug(i)) for i in range(2)])

        kept = outputs()
        assert det.workspace_bytes >= before
        before = det.workspace_bytes
        refused(b"null", rule=None)
        refused(b"null", out=None)
        refused(b"null", ptr=None)
        refused(b"null maps", maps=None)
        for bad in ((-0.01, 0.03, 0.5, 0.02), (0.03, 0.03, 8.5, 0.02), (float("nan"), 0.03, 0.5, 0.02), (0.03, 0.03, 0.5, 0.004),
                    (0.03, 0.03, 0.5, float("nan"))):
            refused(b"rule", rule=ssd.TreadGridRule(*bad))
        refused(b"nmaps", nmaps=0)
        refused(b"nmaps", nmaps=ssd.MAX_STAIR_MAPS + 1)
        refused(b"neither below nmaps", index=(C.c_uint16 * 2)(0, 2))
        refused(b"neither below nmaps", index=(C.c_uint16 * 2)(0xfffe, 0))
        refused(b"neither below nmaps", nmaps=1)
        deep = (ssd.StairMap * 2)(m, m)
        deep[1].stairs.n_steps = ssd.MAX_STEPS + 1
        refused(b"n_steps", maps=deep)
        refused(b"nframes", n=1)
        refused(b"nframes", n=3)
        refused(b"not the last enqueue's", stride=r.stride + 4)
        refused(b"not the last enqueue's", ptr=r.src.ptr + r.stride)
        refused(b"input must be", inp=2)
        refused(b"ssd_set_intrinsics", inp=1)
        refused(b"one-calibration batch", fn=L.ssd_enqueue_cameras_stair_map)
        assert np.all(r.mout.download(r.grec * 3) == POISON), "a refused call wrote something"
        assert det.workspace_bytes == before, "a refused call allocated nothing"
        assert call() == 0
        det.fetch_stair_map()
        assert det.stair_map_time_ms() == 0.0, "timing is off"
        grown = det.workspace_bytes
        assert grown > before
        r.check(r.download(2), r.want([m, m], tg.RULE, [0, 1]))
        assert call(index=(C.c_uint16 * 2)(NONE, NONE)) == 0           # nobody names a map: headers and zeros
        det.fetch_stair_map()
        none = r.download(2)
        assert all((x.n_surfaces, x.ground) == (3, 1) and bytes(x)[8:] == bytes(r.grec - 8) for x in none)
        assert outputs() == kept, "results, risers, labels and debug records are the same bytes with and without the pass"
        # a timed pass
        det.set_timing(True)
        det.enqueue_labels(r.src.ptr, 2, lab.ptr, stride_bytes=r.stride)
        det.fetch_list(2)
        r.fold([m], tg.RULE)
        assert det.stair_map_time_ms() > 0.0
        assert det.workspace_bytes == grown
        # a partial run is no whole enqueue; ssd_set_intrinsics withdraws one
        det.set_debug(False)
        det.set_risers(False)
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride, stages=ssd.STAGE_ALL & ~64)
        refused(b"no whole enqueue")
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride)
        det.fetch_list(2)
        assert call() == 0
        det.fetch_stair_map()
        det.set_intrinsics(intr)
        refused(b"no whole enqueue")
    finally:
        r.close()


def test_the_host_forms_check_the_whole_call_before_the_first_slice(ssd, oracle, gpu_device):
    """an index past nmaps in the SECOND slice is refused before the first slice runs; the host forms' own refusals"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    det = ssd.Detector(ssd.default_config(gm.W, gm.H, max_frames_per_batch=2), trans, gpu_device)
    try:
        three = np.stack(frames[:3])
        res = det.process_host(three)
        m = stair_map(ssd, res[0])
        with pytest.raises(ssd.SsdError, match="neither below nmaps"):
            det.process_host_stair_map(three, [m], [0, 0, 1])
        with pytest.raises(ssd.SsdError, match="nmaps"):
            det.process_host_stair_map(three, [])
        with pytest.raises(ssd.SsdError, match="foot size"):
            det.process_host_stair_map(three, [m], foot_along=-1.0)
        got = det.process_host_stair_map(three, [m], [0, NONE, 0], grids=True)
        assert [bytes(x) for x in got[0]] == [bytes(x) for x in res] and got[2][0].n_surfaces == 3
    finally:
        det.close()


def test_the_host_forms_hold_the_overflow_bound_over_the_whole_call(ssd, oracle, gpu_device):
    """(frames naming one map) x width x height may not pass 2^32 - 1, in 64 bits, over the WHOLE call.  At 256 x 192 = 49152 points the
    bound lies between 87381 frames (4,294,950,912 points) and 87382 (4,295,000,064, which is 32,768 modulo 2^32: a 32-bit product would
    let it through).  The host forms check the maps and the index before they read a byte of `frames`, so the calls below name far more
    frames than the one-frame buffer holds: the refused ones must touch nothing, and the ones within the bound are sent with a foot size
    below 0, which is refused BEHIND the maps and the bound - that refusal shows that they got past the check"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    assert gm.W * gm.H == 49152 and 87381 * 49152 <= 0xffffffff < 87382 * 49152
    L = ssd.lib()
    det = ssd.Detector(ssd.default_config(gm.W, gm.H, max_frames_per_batch=2), trans, gpu_device)
    try:
        one = np.ascontiguousarray(frames[0], dtype=np.float32)
        res = det.process_host(one[None])
        maps = (ssd.StairMap * 2)(stair_map(ssd, res[0]), stair_map(ssd, res[0]))
        rule = tg.rule_of(ssd, tg.RULE)
        results, out = (ssd.FrameResult * 1)(), (ssd.FrameFootholds * 2)()
        grids = (ssd.FrameTreadGrid * 2)()
        C.memset(grids, POISON, C.sizeof(grids))
        C.memset(out, POISON, C.sizeof(out))
        C.memset(results, POISON, C.sizeof(results))
        kept = bytes(grids), bytes(out), bytes(results)
        before = det.workspace_bytes

        def call(n, nmaps=1, index=None, foot=0.0):
            idx = None if index is None else np.ascontiguousarray(index, dtype=np.uint16).ctypes.data_as(C.POINTER(C.c_uint16))
            rc = L.ssd_process_host_stair_map(det._h, one.ctypes.data_as(C.c_void_p), n, 0, maps, nmaps, idx, C.byref(rule), 3, 3, foot, 0.0,
                                              results, grids, out)
            return rc, L.ssd_last_error()

        def over(*a, **kw):
            rc, msg = call(*a, **kw)
            assert rc == -1 and b"more than 2^32 - 1 points" in msg, (rc, msg)

        def within(*a, **kw):
            rc, msg = call(*a, foot=-1.0, **kw)
            assert rc == -1 and b"foot size" in msg, (rc, msg)

        over(87382)                                                    # no index: every frame names map 0
        over(87382, foot=-1.0)                                         # ... and the bound is refused in front of the foot size
        within(87381)
        idx = np.zeros(87382, dtype=np.uint16)
        over(87382, index=idx)
        idx[40000] = NONE                                              # one frame names no map: 87381 are left
        within(87382, index=idx)
        # per map, not per call: two maps dealt alternately hold 87381 frames each, then 87382
        dealt = (np.arange(2 * 87382) % 2).astype(np.uint16)
        within(2 * 87381, nmaps=2, index=dealt[:2 * 87381])
        over(2 * 87382, nmaps=2, index=dealt)
        over(2 * 87381 + 1, nmaps=2, index=dealt[:2 * 87381 + 1])      # the odd frame is map 0's
        assert (bytes(grids), bytes(out), bytes(results)) == kept, "a refused call wrote something"
        assert det.workspace_bytes == before, "a refused call allocated something that counts"
        # the handle is as it was: a call of one frame runs
        res1, out1, grids1 = det.process_host_stair_map(one[None], [maps[0]], None, rule, 3, 3, grids=True)
        assert bytes(res1[0]) == bytes(res[0]) and grids1[0].n_surfaces == 3
    finally:
        det.close()


def test_two_calls_on_two_streams_into_one_buffer_hold_the_sum_of_both(ssd, oracle, gpu_device, two_streams):           # noqa: F811
    """no host wait between the calls: the first zeroes and adds on stream B, the second accumulates on stream A.  The library has to order
    the second behind the first (one set of device maps, one record); what the fetch finds is the sum of both.  As
    tests/test_gpu_follow_passes.py: this guards the order, it cannot prove it"""
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    cfg.max_frames_per_batch = 2
    cfg.batches_in_flight = 1
    a, b = two_streams
    r = MapResident(ssd, gpu_device, cfg, trans, frames[:2])
    try:
        r.det.enqueue(r.src.ptr, 2, stride_bytes=r.stride, stream=a)
        res = r.det.fetch_list(2)
        first, second = [stair_map(ssd, res[0])], [stair_map(ssd, res[1])]
        r.poison(1)
        rule = tg.rule_of(ssd, tg.RULE)
        r.det.enqueue_stair_map(r.src.ptr, 2, first, r.mout.ptr, [0, NONE], rule, False, stride_bytes=r.stride, stream=b)
        r.det.enqueue_stair_map(r.src.ptr, 2, second, r.mout.ptr, [NONE, 0], rule, True, stride_bytes=r.stride, stream=a)
        r.det.fetch_stair_map()
        want = r.want(first, tg.RULE, [0, NONE])[0]
        ssd.tread_grid_add(r.want(second, tg.RULE, [NONE, 0])[0], want)
        r.check(r.download(1), [want])
    finally:
        r.close()
