"""The follow-on passes at the block geometry production batches run: the riser pass with its records, the riser
labels, the riser moments, the surface labels, the surface moments, two trimmed refit passes chained on the device, clearance with its
mask, the tread grid and the stair map (accumulate off, then on), behind whole enqueues whose chunk_plan(...).chunk is 32, 17 and 5
tiles - tests/follow_geometry.py names the three geometries and what each reaches.  The rest of the GPU suite runs these passes at 1 and
2 tiles, where a block's list holds at most one group of cells per wave.

A batch is D = 8 template frames repeated in the order (7 i) % D (follow_geometry.Templates: live staircases with visible risers, two of
them with a box - one on the ground surface in front of the stairs, one on the top tread -, a many-step one, a bare floor, an all-zero
frame and one the detector throws on; thrown and empty frames sit between live ones).  A pass's record for frame i depends on frame i's bytes, its result, its
camera and the rule alone, so every host statement is computed once per template, on the handle's OWN fetched result of the template's
first copy, and EVERY frame's device bytes are compared with its template's: no sampling, no tolerance - everything compared is integers,
label bytes or one text of correctly rounded doubles.  The results of all copies of a template are asserted byte-equal first.

The batch is filled on the device (ssd.synth_device / synth_depth_device over the repeated scene list; the D distinct frames are downloaded
once and must be synth_host's bits); the hand-patched templates (the boxes, the all-zero frame) are uploaded over their copies.  Frames
lie at a stride that is no multiple of 16 bytes; every record, mask and label buffer is poisoned first, with one record (one label or mask
row) of poison behind the batch and 37 bytes of poison between label and mask rows, all of which must still be poison afterwards.  One
workspace throughout.  Case B also runs the cameras form: three cameras with poses a little apart, frames in mixed order, a table entry
nobody names, a handle whose own calibration is the identity (as tests/test_gpu_sweep.py).

Each batch first asserts on the CPU that chunk_plan gives its tile count and one frame fewer the smaller one (tests/chunk_plan_main.cpp),
whether it qualifies for the single pass, what its templates hold and, for case B, that some chunk of 272 cells holds a tread in more
than 256 of them (the second pass of the cell list runs part-filled); a precondition that is not met fails the batch's tests.

Out of scope: the ground fit and the stair pose take their launch geometry from the frame-pass unit, not from `chunk`.
Harnesses: tests/test_gpu_stair_map.py's MapResident (test_gpu_tread_grid.py, test_gpu_clearance.py), test_gpu_riser_labels.py's _label
and _check_model."""
import ctypes as C
import functools

import numpy as np
import pytest

import clearance_model as cm
import follow_geometry as fg
import surface_model as sm
import tread_grid_model as tg
from test_gpu_clearance import POISON
from test_gpu_riser_labels import SUPPORT, TOL, _check_model, _label
from test_gpu_stair_map import NONE, MapResident, header_of, stair_map

pytestmark = pytest.mark.gpu

CASES = [("A", False, False), ("A", True, False), ("B", False, False), ("B", True, False), ("B", False, True), ("B", True, True),
         ("C", False, False), ("C", True, False)]
REFIT = dict(min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0)
_STOP = []                                               # a device call failed (batch set-up or test body): nothing more is started on the device


# ---- the host statements, once per template ----------------------------------------------------------------------------------------------------
def ground_flags(T):
    """per template whether surface 0 of its result is the ground: the oracle's word, as tests/test_gpu_sweep.py"""
    return [1 if T.live(t) and T.records[t].ground_ind >= 0 else 0 for t in range(fg.D)]


def live_of(ssd, res):
    return res.n_steps > 0 and not (res.status & ssd.ST_THROW)


def want_surface_moments(ssd, T, cfg, res, labels, ground):
    out = []
    for t in range(fg.D):
        live = live_of(ssd, res[t])
        out.append(ssd.surface_moments_host(cfg, T.frames[t], labels[t], res[t].n_steps if live else 0, ground[t] if live else 0, intr=T.intr))
    return out


def want_refit_chain(ssd, T, cfg, labels, first, passes=2):
    """`passes` host-gated refit passes on top of the first-pass records -> (records, points the gates trimmed)"""
    out, trimmed = [], 0
    for t in range(fg.D):
        cur = first[t]
        for _ in range(passes):
            gates = ssd.surface_gates_from_moments(cur, **REFIT)
            nxt = ssd.surface_refit_moments_host(cfg, T.frames[t], labels[t], gates, first[t].n_surfaces, first[t].ground, intr=T.intr)
            trimmed += sum(int(cur.s[k].m.n) - int(nxt.s[k].m.n) for k in range(cur.n_surfaces))
            cur = nxt
        out.append(cur)
    return out, trimmed


def want_clearance(ssd, T, cfg, res, ground, rule):
    """-> (records, masks [W H]) of ssd_clearance_host; the host sums over each mask are the record"""
    recs, masks = [], []
    for t in range(fg.D):
        rec, mask = ssd.clearance_host(cfg, T.cal_of(t), T.frames[t], res[t], ground[t], cm.rule_of(ssd, rule), intr=T.intr)
        sums = ssd.surface_moments_host(cfg, T.frames[t], mask.reshape(-1), rec.n_surfaces, rec.ground, intr=T.intr)
        assert bytes(sums) == bytes(rec), t
        recs.append(rec)
        masks.append(np.ascontiguousarray(mask.reshape(-1)))
    return recs, masks


def want_tread_grid(ssd, T, cfg, res, ground, rule):
    return [ssd.tread_grid_host(cfg, T.cal_of(t), T.frames[t], res[t], ground[t], tg.rule_of(ssd, rule), intr=T.intr) for t in range(fg.D)]


def map_of_template(T):
    """which map the frames of template t name: their own, the thrown template none, template 7 the map of template 0 (another
    staircase's frames under a map that is not theirs), so that map 7 is nobody's"""
    return [NONE if T.thrown[t] else 0 if t == 7 else t for t in range(fg.D)]


def want_stair_map(ssd, T, cfg, maps, names, copies, rule, times=1):
    """the fold by ssd_tread_grid_add of ssd_tread_grid_host, per template and map once, added as often as the template has copies"""
    out = []
    for m, sm_ in enumerate(maps):
        acc = ssd.FrameTreadGrid()
        acc.n_surfaces, acc.ground = header_of(ssd, sm_)
        for t in range(fg.D):
            if names[t] != m:
                continue
            g = ssd.tread_grid_host(cfg, T.cal_of(t), T.frames[t], sm_.stairs, sm_.ground, tg.rule_of(ssd, rule), intr=T.intr)
            assert (g.n_surfaces, g.ground) == (acc.n_surfaces, acc.ground)
            for _ in range(copies[t] * times):
                ssd.tread_grid_add(g, acc)
        out.append(acc)
    return out


# ---- one batch behind one handle ------------------------------------------------------------------------------------------------------------
class Follow:
    """a geometry's batch resident behind one handle: the CPU preconditions, the device fill, the first plain enqueue"""

    def __init__(self, ssd, oracle, device, exe, case, depth, cameras):
        self.ssd, self.case, self.depth, self.cameras = ssd, case, depth, cameras
        w, h, n, tiles, below = fg.GEOMETRY[(case, depth)]
        self.n, self.wh = n, w * h
        # the CPU preconditions: the plan, the single pass, the templates
        tile, _, plans = fg.chunk_plans(exe, [(w * h, n), (w * h, n - 1)])
        assert tile == fg.TILE and plans[(w * h, n)]["chunk"] == tiles * tile, plans
        assert plans[(w * h, n - 1)]["chunk"] == below * tile, "one frame fewer gives the smaller chunk"
        self.single = not depth and n * w * h >= fg.SINGLE_PASS_MIN_POINTS
        assert (n * w * h >= fg.SINGLE_PASS_MIN_POINTS) == (case in ("A", "B")), "A and B qualify for the single pass, C does not"
        self.T = T = fg.templates(ssd, oracle, w, h, depth, cameras)
        T.check_layout(n)
        if case == "B":                                    # the row's claim: a chunk whose list runs into the second pass, part-filled
            dense = T.dense_cells(3, tiles * tile)
            assert fg.FIRST_PASS_CELLS < max(dense) <= tiles * tile // fg.CELL, dense
        self.which = fg.which(n)
        self.first = [self.which.index(t) for t in range(fg.D)]
        self.copies = [self.which.count(t) for t in range(fg.D)]
        self.cfg = type(T.cfg).from_buffer_copy(T.cfg)
        self.cfg.max_frames_per_batch = n
        assert self.cfg.batches_in_flight == 0, "one workspace"
        frames = [T.frames[t] for t in self.which]
        pad = 16 if depth and (frames[0].nbytes + 8) % 16 == 0 else None
        if cameras:
            entries = len(fg.CAMERA_POSES) + 1
            table, cals = [None] * entries, [None] * entries
            for c, e in enumerate(fg.TABLE_OF_CAMERA):
                table[e], cals[e] = (T.trans[c], T.intr) if depth else T.trans[c], T.cals[c]
            table[fg.UNUSED], cals[fg.UNUSED] = ssd.GeometricTransformation(), ssd.GeometricTransformation().constants
            order = [fg.TABLE_OF_CAMERA[T.camera[t]] for t in self.which]
            assert fg.UNUSED not in order and len(set(order)) == 3 and order != sorted(order)
            self.r = MapResident(ssd, device, self.cfg, ssd.GeometricTransformation(), frames, depth=depth, intr=T.intr, cameras=table, order=order,
                                 pad=pad, fill=self.fill)
            self.r.cameras_cal = cals
        else:
            self.r = MapResident(ssd, device, self.cfg, T.trans[0], frames, depth=depth, intr=T.intr, pad=pad, fill=self.fill)
        self.det = self.r.det
        self.lab = None
        # the first enqueue: the plain one, and the pass it took
        self.res_all = self.r.detect()
        self.ran_single = self.det.single_pass_stats(n, scan_planes=False)["ran"]
        self.res = [self.res_all[j] for j in self.first]
        self.res_bytes = [bytes(x) for x in self.res_all]

    def fill(self, src, stride):
        """the frames made on the device from the repeated scene list; the distinct ones are synth_host's; the patched ones uploaded"""
        ssd, T = self.ssd, self.T
        scs = [T.scenes[t] for t in self.which]
        (ssd.synth_depth_device if self.depth else ssd.synth_device)(scs, src.ptr, stride_bytes=stride, device=src.device)
        fb = T.frames[0].nbytes
        for t in range(fg.D):
            got = src.download(fb, offset=self.first[t] * stride)
            assert got.tobytes() == T.generated[t].tobytes(), "template %d: the device's frame is not synth_host's" % t
        for i, t in enumerate(self.which):
            if T.patched[t]:
                src.upload(T.frames[t], offset=i * stride)

    def close(self):
        self.r.close()

    def plain(self):
        """a plain whole enqueue (no risers, no debug records) in front of a pass: the results are the first enqueue's"""
        self.det.set_debug(False)
        self.det.set_risers(False)
        self.det.set_riser_labels(False)
        self.det.set_riser_moments(False)
        assert [bytes(x) for x in self.r.detect()] == self.res_bytes

    def unchanged(self):
        assert [bytes(x) for x in self.det.fetch_list(self.n)] == self.res_bytes, "the results are still the enqueue's"

    def tiled(self, got, want, what):
        """every frame's bytes against its template's"""
        assert len(got) == self.n
        for i, t in enumerate(self.which):
            assert bytes(got[i]) == bytes(want[t]), "frame %d (template %d): %s" % (i, t, what)

    def tiled_rows(self, got, want, what):
        assert got.shape[0] == self.n
        for i, t in enumerate(self.which):
            if not np.array_equal(got[i], want[t]):
                raise AssertionError("frame %d (template %d): %s: %d pixels differ" % (i, t, what, int(np.count_nonzero(got[i] != want[t]))))

    def labelled(self):
        """the enqueue with labels, risers, riser moments and debug records, riser labels off and then on (made once)"""
        if self.lab is None:
            det, r = self.det, self.r
            det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
            det.set_riser_moments(True)
            det.set_debug(True, images=False)
            det.set_riser_labels(False)
            off = _label(self.ssd, det, r.src, r.stride, self.n, r.device, depth=self.depth, order=r.order, moments=True, debug=True)
            det.set_riser_labels(True)
            on = _label(self.ssd, det, r.src, r.stride, self.n, r.device, depth=self.depth, order=r.order, moments=True, debug=True)
            self.lab = (off, on)
        return self.lab


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    return fg.build_chunk_plan(tmp_path_factory.mktemp("chunk_plan"))


def refusal(e):
    """SSD_E_ARG (-1): a call that refused its arguments before it did anything - a host statement handed labels the device left wrong,
    for one - is a failed test, not an error of the device"""
    return " error -1:" in str(e)


def stops_the_file(test):
    """a test body whose device call fails (SsdError other than a refused argument, from any enqueue, fetch or copy) stops every test
    behind it, of this batch and of the batches that follow: nothing more is started on a device that has reported an error"""
    @functools.wraps(test)
    def run(ssd, batch):
        assert not _STOP, "an earlier test of this file ended in an error of the device: nothing more is started on it"
        try:
            test(ssd, batch)
        except ssd.SsdError as e:
            if not refusal(e):
                _STOP.append(test.__name__)
            raise
    return run


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s%s" % (c, "depth16" if d else "vertices", "-cameras" if k else "") for c, d, k in CASES])
def batch(request, ssd, oracle, gpu_device, plan_exe):
    assert not _STOP, "an earlier batch of this file ended in an error of the device: nothing more is started on it"
    case, depth, cameras = request.param
    try:
        b = Follow(ssd, oracle, gpu_device, plan_exe, case, depth, cameras)
    except ssd.SsdError as e:
        if not refusal(e):
            _STOP.append(request.param)
        raise
    yield b
    b.close()


# ---- the tests -------------------------------------------------------------------------------------------------------------------------------------
@stops_the_file
def test_the_results_of_every_copy_and_the_pass_taken(ssd, batch):
    """the plain enqueue: every copy of a template reports the template's bytes, which are the oracle's count and throw; the handle took
    the single pass exactly where vertex input qualifies for it"""
    b, T = batch, batch.T
    assert b.ran_single == b.single, "the pass the handle took"
    b.tiled(b.res_all, b.res, "the result differs from the template's first copy")
    for t in range(fg.D):
        assert bool(b.res[t].status & ssd.ST_THROW) == T.thrown[t] and b.res[t].n_steps == T.steps[t], t
    b.plain()                                              # a second enqueue of the same frames gives the same bytes


@stops_the_file
def test_labels_riser_labels_riser_records_and_riser_moments(ssd, batch):
    """surface labels: expected_labels on the oracle's record, every pixel of every frame.  Riser labels: riser_model's word on the
    handle's own debug record, and per riser the count of its label is the riser record's n_points (K6).  Riser moments:
    ssd_surface_moments_host over the device's riser labels.  Results, risers, riser moments and debug records do not move with the riser
    labels, and every copy of a template holds the template's bytes"""
    b, T = batch, batch.T
    off, on = b.labelled()
    assert on.res == off.res == b.res_bytes
    assert [bytes(m) for m in on.rmom] == [bytes(m) for m in off.rmom] and [bytes(x) for x in on.risers] == [bytes(x) for x in off.risers]
    b.tiled_rows(off.labels, T.labels, "the surface labels are not expected_labels'")
    found = 0
    for t, j in enumerate(b.first):
        risers = _check_model(ssd, b.cfg, T.cal_of(t), T.pts[t], on, off, j)
        ris = on.risers[j]
        assert ris.n_risers == max((0 if T.thrown[t] else T.steps[t]) - 1, 0), t
        want = ssd.surface_moments_host(b.cfg, T.frames[t], risers, ris.n_risers, 0, intr=T.intr)
        assert bytes(on.rmom[j]) == bytes(want), "template %d: the riser moments are not the host's sums over the device's labels" % t
        if ris.n_risers == 0:
            assert bytes(on.rmom[j]) == bytes(C.sizeof(ssd.FrameMoments)) and not risers.any()
        found += sum(1 for k in range(ris.n_risers) if ris.risers[k].detected)
    evidence = sum(int(np.count_nonzero(ssd.labels_split(on.labels[j])[1])) for j in b.first)
    assert evidence > 10000 and (found > 0 or b.case == "C"), "riser pixels in the masks; detected risers where a frame is large enough for the support"
    b.tiled_rows(on.labels, [on.labels[j] for j in b.first], "the labels with riser labels differ from the template's first copy")
    b.tiled(on.risers, [on.risers[j] for j in b.first], "the riser records")
    b.tiled(on.rmom, [on.rmom[j] for j in b.first], "the riser moments")
    b.tiled(on.dbg, [on.dbg[j] for j in b.first], "the debug record")
    assert [bytes(d) for d in on.dbg] == [bytes(d) for d in off.dbg]


@stops_the_file
def test_surface_moments_and_two_refit_passes_chained_on_the_device(ssd, batch):
    """the first-pass records are ssd_surface_moments_host over the device's own label mask; enqueue_surface_refit_device(first -> out),
    then (out -> out), with no fetch between, is ssd_surface_refit_moments_host under ssd_surface_gates_from_moments, pass by pass"""
    b, T, r, det, n = batch, batch.T, batch.r, batch.det, batch.n
    off, _ = b.labelled()
    labels = [off.labels[j] for j in b.first]
    ground = [1 if off.dbg[j].ground_ind >= 0 else 0 for j in b.first]
    rec = C.sizeof(ssd.FrameMoments)
    first_buf, out_buf = (ssd.DeviceBuffer(rec * (n + 1), r.device) for _ in range(2))
    r.bufs += [first_buf, out_buf]

    def first_pass():
        if b.cameras:
            det.enqueue_cameras_surface_moments(r.src.ptr, n, r.order, first_buf.ptr, depth=b.depth, stride_bytes=r.stride)
        else:
            det.enqueue_surface_moments(r.src.ptr, n, first_buf.ptr, depth=b.depth, stride_bytes=r.stride)

    def refit(prev):
        fn = det.enqueue_cameras_surface_refit_device if b.cameras else det.enqueue_surface_refit_device
        fn(r.src.ptr, n, prev.ptr, out_buf.ptr, depth=b.depth, stride_bytes=r.stride, **REFIT)

    def records(buf):
        raw = buf.download(rec * (n + 1))
        assert np.all(raw[rec * n:] == POISON), "a record past nframes was written"
        return list((ssd.FrameMoments * n).from_buffer_copy(raw[:rec * n].tobytes()))

    for buf in (first_buf, out_buf):
        buf.upload(np.full(rec * (n + 1), POISON, dtype=np.uint8))
    first_pass()
    b.unchanged()
    want = want_surface_moments(ssd, T, b.cfg, b.res, labels, ground)
    b.tiled(records(first_buf), want, "the first pass is not the host's sums over the device's labels")
    for t in range(fg.D):
        assert live_of(ssd, b.res[t]) or bytes(want[t]) == bytes(rec), "a thrown or empty frame: the all-zero record"
    assert sum(int(want[t].s[k].m.n) for t in range(fg.D) for k in range(want[t].n_surfaces)) > 0
    refit(first_buf)
    refit(out_buf)
    b.unchanged()
    det.fetch_surface_refit()
    chain, trimmed = want_refit_chain(ssd, T, b.cfg, labels, want)
    b.tiled(records(out_buf), chain, "two chained passes are not the host's")
    b.tiled(records(first_buf), want, "the chain wrote into the first pass's records")
    assert trimmed > 0, "the gates trim something"


@stops_the_file
def test_clearance_with_its_mask(ssd, batch):
    """records and masks under clearance_model.RULE are ssd_clearance_host's on the handle's own results, the host sums over the mask the
    record; the two templates with a box hold occupants"""
    b, T = batch, batch.T
    b.plain()
    ground = ground_flags(T)
    recs, masks = b.r.clear(cm.RULE)
    want, wmasks = want_clearance(ssd, T, b.cfg, b.res, ground, cm.RULE)
    b.tiled(recs, want, "the clearance record is not the host's")
    b.tiled_rows(masks, wmasks, "the clearance mask is not the host's")
    for t in fg.OCCUPANT_SURFACE:
        assert sum(int(want[t].s[k].m.n + want[t].s[k].n_far) for k in range(ssd.MAX_STEPS)) >= 40, "template %d: the box on its tread" % t
    for t in range(fg.D):
        assert live_of(ssd, b.res[t]) or (bytes(want[t]) == bytes(C.sizeof(ssd.FrameMoments)) and not wmasks[t].any())
    b.unchanged()


@stops_the_file
def test_the_tread_grid(ssd, batch):
    """the records under tread_grid_model.RULE are ssd_tread_grid_host's on the handle's own results"""
    b, T = batch, batch.T
    b.plain()
    ground = ground_flags(T)
    want = want_tread_grid(ssd, T, b.cfg, b.res, ground, tg.RULE)
    b.tiled(b.r.grid(tg.RULE), want, "the tread grid is not the host's")
    seen = sum(int(tg.grid_of_record(want[t], k)["seen"].sum()) for t in range(fg.D) for k in range(want[t].n_surfaces))
    assert seen > 1000, "tread points in the grids"
    b.unchanged()


@stops_the_file
def test_the_stair_map_and_a_second_call_on_top(ssd, batch):
    """a map per template (its own result), every frame naming its template's map, the thrown template none and template 7 the map of
    template 0: the records are the fold by ssd_tread_grid_add of ssd_tread_grid_host; the same call again with accumulate on doubles
    every count and leaves every top"""
    b, T = batch, batch.T
    b.plain()
    ground = ground_flags(T)
    maps = [stair_map(ssd, b.res[t], ground=ground[t]) for t in range(fg.D)]
    names = map_of_template(T)
    index = [names[t] for t in b.which]
    assert NONE in index and 7 not in index
    once = b.r.fold(maps, tg.RULE, index)
    b.r.check(once, want_stair_map(ssd, T, b.cfg, maps, names, b.copies, tg.RULE))
    assert bytes(once[7])[8:] == bytes(len(bytes(once[7])) - 8), "a map no frame names: the header and zeros"
    assert sum(int(tg.grid_of_record(g, k)["seen"].sum()) for g in once for k in range(g.n_surfaces)) > 1000 * b.n // fg.D
    twice = b.r.fold(maps, tg.RULE, index, accumulate=True)
    b.r.check(twice, want_stair_map(ssd, T, b.cfg, maps, names, b.copies, tg.RULE, times=2))
    b.unchanged()
