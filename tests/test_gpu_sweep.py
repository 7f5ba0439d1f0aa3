"""The follow-on passes on the GPU over the sweep's scene list (tests/sweep_scenes.py): every pass that runs behind a whole enqueue, on
every frame of the list, byte for byte its host statement on the handle's OWN fetched results - labels, riser labels, surface moments,
riser moments, device gates, the chained refit, ground fit, clearance, tread grid, stair map and stair pose.  The host statements are in
turn held to their numpy models on the same frames by tests/test_sweep_scenes.py, which also asserts what the list holds: staircases
turned by up to 35 degrees, 0 to 6 reported steps, thrown and empty frames, 15 % outliers, 20 % invalid pixels.

Batches: one calibration - the eight staircases' frames of one view, a batch per view; cameras - the views 0 to 2, and 3 to 5, of all
staircases (24 frames each), one camera per view in a table that is visited out of order and holds an entry nobody names, behind a
handle whose own calibration is the identity.  Either way thrown, empty and many-step frames sit between live ones.  The ragged part
(250 x 190 vertices, 252 x 191 depth) is one more batch.  Every pass writes into poisoned buffers with a poisoned record behind the
batch, from frames at a stride that is no multiple of 16 bytes (ground fit and stair pose, whose loads are wide: both kinds).
No tolerance anywhere: everything compared is integers or one text of correctly rounded double operations.  Besides the rules the issue
names, clearance, tread grid and stair pose run under rules made so that a point of the batch lies exactly ON an inequality
(sweep_scenes.edge_*, from the handle's own results): what a comparison turned from > to >= in a kernel changes.
Harnesses: tests/test_gpu_clearance.py, test_gpu_tread_grid.py, test_gpu_stair_map.py, test_gpu_stair_pose.py, test_gpu_riser_labels.py."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as cm
import ground_model as gm
import stair_pose_model as spm
import surface_model as sm
import sweep_scenes as ss
import tread_grid_model as tg
from test_gpu_clearance import POISON, Resident
from test_gpu_riser_labels import _check_model, _label
from test_gpu_stair_map import NONE, MapResident
from test_gpu_stair_pose import Frames, _check
from test_sweep_scenes import CELLS, CLEAR_RULES, POSE_RULES, RISER_SUPPORT, RISER_TOLS, off_prior, pose_prior

pytestmark = pytest.mark.gpu

INPUTS = pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])
FORMS = pytest.mark.parametrize("cameras", [False, True], ids=["one-calibration", "cameras"])
ALIGNED = pytest.mark.parametrize("aligned", [False, True], ids=["stride-odd", "stride-16B-multiple"])
# the cameras form: view v is table entry TABLE_OF_VIEW[v]; entry UNUSED is nobody's
TABLE_OF_VIEW, UNUSED = (3, 5, 1, 6, 4, 0), 2
MAX_BATCH = 24


def batches(sw, cameras):
    """the sweep's frames as batches: [frame indices]"""
    if sw.n <= ss.G:
        return [list(range(sw.n))]
    if not cameras:
        return [[i for i in range(sw.n) if sw.view[i] == v] for v in range(ss.V)]
    order = sorted(range(sw.n), key=lambda i: (sw.view[i], sw.group[i]))
    return [order[at:at + MAX_BATCH] for at in range(0, sw.n, MAX_BATCH)]


def resident(ssd, device, sw, idx, cameras, reverse=False):
    """the frames `idx` of the sweep resident behind one handle (tests/test_gpu_stair_map.py's harness), one calibration or cameras"""
    idx = idx[::-1] if reverse else idx
    frames = [sw.frames[i] for i in idx]
    cfg = type(sw.cfg).from_buffer_copy(sw.cfg)
    cfg.max_frames_per_batch = max(len(idx), 2)
    pad = 16 if (frames[0].nbytes + 8) % 16 == 0 else None          # 252 x 191 depth: + 8 is a multiple of 16, and depth wants one of 8
    if cameras:
        table, cals = [None] * (ss.V + 1), [None] * (ss.V + 1)
        for v, t in enumerate(TABLE_OF_VIEW):
            table[t], cals[t] = (sw.trans[v], sw.intr) if sw.depth else sw.trans[v], sw.cals[v]
        table[UNUSED], cals[UNUSED] = ssd.GeometricTransformation(), ssd.GeometricTransformation().constants
        order = [TABLE_OF_VIEW[sw.view[i]] for i in idx]
        r = MapResident(ssd, device, cfg, ssd.GeometricTransformation(), frames, depth=sw.depth, intr=sw.intr, cameras=table, order=order, pad=pad)
        r.cameras_cal = cals
    else:
        views = {sw.view[i] for i in idx}
        assert len(views) == 1, "a one-calibration batch is one view's"
        r = MapResident(ssd, device, cfg, sw.trans[views.pop()], frames, depth=sw.depth, intr=sw.intr, pad=pad)
    assert r.stride % 16 != 0 and r.n <= MAX_BATCH
    r.idx = idx
    return r


def every_batch(ssd, oracle, depth, cameras):
    """(sweep, frame indices) of every batch of the list and of its ragged part"""
    for ragged in (False, True):
        sw = ss.sweep(ssd, oracle, depth, ragged)
        for idx in batches(sw, cameras):
            yield sw, idx


def test_the_batches_hold_every_frame_and_mix_the_staircases(ssd, oracle):
    for cameras in (False, True):
        sw = ss.sweep(ssd, oracle)
        parts = batches(sw, cameras)
        assert sorted(i for p in parts for i in p) == list(range(sw.n)), "no frame of the list is left out"
        for p in parts:
            assert len(p) <= MAX_BATCH
            kinds = ["throw" if sw.thrown[i] else "empty" if sw.records[i].n_steps == 0 else "live" for i in p]
            assert {"throw", "empty", "live"} <= set(kinds) and max(sw.records[i].n_steps for i in p) >= 4
            assert kinds[0] == "live" and kinds[-1] == "live", "thrown and empty frames sit between live ones"
        if cameras:
            used = [TABLE_OF_VIEW[sw.view[i]] for i in parts[0]]
            assert used != sorted(used) and UNUSED not in TABLE_OF_VIEW and len(set(TABLE_OF_VIEW)) == ss.V


def edge_rules(ssd, sw, r, idx):
    """the rules that put a point of this batch exactly on an inequality (tests/sweep_scenes.py), made from the handle's OWN results:
    (a clearance rule whose margin is an occupant's distance inside a side, a tread grid rule whose lo is a tread point's distance from
    its surface, one whose cell splits v / cell from v * (1 / cell))"""
    def first(find):
        for j, i in enumerate(idx):
            if r.res[j].n_steps > 0 and not (r.res[j].status & ssd.ST_THROW):
                got = find(r.cal_of(j), r.res[j], sw.pts[i])
                if got is not None:
                    return got[0]
        raise AssertionError("no frame of the batch reaches the edge")
    margin = first(lambda cal, res, pts: ss.edge_margin(sw.cfg, cal, res, pts, *cm.RULE[1:]))
    lo = first(lambda cal, res, pts: ss.edge_lo(sw.cfg, cal, res, pts, tg.RULE))
    cell = first(lambda cal, res, pts: ss.edge_cell(sw.cfg, cal, res, pts, tg.RULE))
    return (margin,) + cm.RULE[1:], (tg.RULE[0], lo) + tg.RULE[2:], tg.RULE[:3] + (cell,)


def _moments(ssd, raw, n):
    return list((ssd.FrameMoments * n).from_buffer_copy(np.ascontiguousarray(raw).tobytes()))


# ---- labels, riser labels, riser moments ----------------------------------------------------------------------------------------------------
@INPUTS
@FORMS
def test_labels_riser_labels_and_riser_moments(ssd, oracle, gpu_device, depth, cameras):
    """the surface labels are expected_labels' on the oracle's record, pixel for pixel, and the results the oracle's counts; the riser
    half of the mask is riser_model's word on the handle's own debug record under two tolerances; the riser moments are
    ssd_surface_moments_host over the device's own riser labels; the support leaves risers with evidence and risers without"""
    found = missed = 0
    for sw, idx in every_batch(ssd, oracle, depth, cameras):
        r = resident(ssd, gpu_device, sw, idx, cameras)
        try:
            det = r.det
            det.set_riser_moments(True)
            det.set_debug(True, images=False)
            first = None
            for tol in RISER_TOLS:
                det.set_risers(True, tolerance=tol, min_support=RISER_SUPPORT)
                det.set_riser_labels(False)
                off = _label(ssd, det, r.src, r.stride, r.n, gpu_device, depth=depth, order=r.order, moments=True, debug=True)
                det.set_riser_labels(True)
                on = _label(ssd, det, r.src, r.stride, r.n, gpu_device, depth=depth, order=r.order, moments=True, debug=True)
                assert on.res == off.res and [bytes(m) for m in on.rmom] == [bytes(m) for m in off.rmom]
                first = first or off.res
                assert off.res == first, "the tolerance moves no result"
                for j, i in enumerate(idx):
                    res = ssd.FrameResult.from_buffer_copy(off.res[j])
                    assert bool(res.status & ssd.ST_THROW) == sw.thrown[i] and res.n_steps == sw.records[i].n_steps, i
                    assert np.array_equal(off.labels[j], sw.labels[i]), "frame %d: the labels are not expected_labels'" % i
                    risers = _check_model(ssd, sw.cfg, r.cal_of(j), sw.pts[i], on, off, j, tol)
                    ris = on.risers[j]
                    assert ris.n_risers == max((0 if sw.thrown[i] else res.n_steps) - 1, 0), i
                    want = ssd.surface_moments_host(sw.cfg, sw.frames[i], risers, ris.n_risers, 0, intr=sw.intr)
                    assert bytes(on.rmom[j]) == bytes(want), "frame %d: the riser moments are not the host's sums over the device's labels" % i
                    if ris.n_risers == 0:
                        assert bytes(on.rmom[j]) == bytes(C.sizeof(ssd.FrameMoments)) and not risers.any()
                    found += sum(1 for k in range(ris.n_risers) if ris.risers[k].detected)
                    missed += sum(1 for k in range(ris.n_risers) if not ris.risers[k].detected)
        finally:
            r.close()
    assert found > 10 and missed > 10, "risers with evidence and risers without"


# ---- surface moments, device gates, the chained refit ------------------------------------------------------------------------------------------
@INPUTS
@FORMS
def test_surface_moments_gates_and_the_refit_chain(ssd, oracle, gpu_device, depth, cameras):
    """the first-pass records are ssd_surface_moments_host over the device's own label mask; ssd_enqueue_surface_gates of them is
    ssd_surface_gates_from_moments; two refit passes chained on the device with no fetch between are ssd_surface_refit_moments_host
    under those gates, pass by pass"""
    kw = dict(min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0)
    rec, gsz = C.sizeof(ssd.FrameMoments), C.sizeof(ssd.FrameGates)
    trimmed = 0
    for sw, idx in every_batch(ssd, oracle, depth, cameras):
        r = resident(ssd, gpu_device, sw, idx, cameras)
        n, det = r.n, r.det
        bufs = [ssd.DeviceBuffer(rec * (n + 1), gpu_device) for _ in range(2)] + [ssd.DeviceBuffer(gsz * (n + 1), gpu_device)]
        first_buf, out_buf, gate_buf = bufs
        r.bufs += bufs
        try:
            det.set_risers(True, tolerance=RISER_TOLS[0], min_support=RISER_SUPPORT)
            det.set_debug(True, images=False)
            lab = _label(ssd, det, r.src, r.stride, n, gpu_device, depth=depth, order=r.order, debug=True)
            ground = [1 if d.ground_ind >= 0 else 0 for d in lab.dbg]

            def first_pass():
                if cameras:
                    det.enqueue_cameras_surface_moments(r.src.ptr, n, r.order, first_buf.ptr, depth=depth, stride_bytes=r.stride)
                else:
                    det.enqueue_surface_moments(r.src.ptr, n, first_buf.ptr, depth=depth, stride_bytes=r.stride)

            def refit(prev):
                fn = det.enqueue_cameras_surface_refit_device if cameras else det.enqueue_surface_refit_device
                fn(r.src.ptr, n, prev.ptr, out_buf.ptr, depth=depth, stride_bytes=r.stride, **kw)

            def poisoned(buf, size):
                buf.upload(np.full(size * (n + 1), POISON, dtype=np.uint8))

            def records(buf):
                raw = buf.download(rec * (n + 1))
                assert np.all(raw[rec * n:] == POISON), "a record past nframes was written"
                return _moments(ssd, raw[:rec * n], n)

            poisoned(first_buf, rec)
            first_pass()
            res = det.fetch_list(n)
            assert [bytes(x) for x in res] == lab.res
            first = records(first_buf)
            want = []
            for j, i in enumerate(idx):
                live = res[j].n_steps > 0 and not (res[j].status & ssd.ST_THROW)
                w = ssd.surface_moments_host(sw.cfg, sw.frames[i], lab.labels[j], res[j].n_steps if live else 0, ground[j] if live else 0, intr=sw.intr)
                assert bytes(first[j]) == bytes(w), "frame %d: the first pass is not the host's sums over the device's labels" % i
                assert live or bytes(first[j]) == bytes(rec), "a thrown or empty frame: the all-zero record"
                want.append(w)
            # the gates of the first pass, by the kernel
            poisoned(gate_buf, gsz)
            det.enqueue_surface_gates(first_buf.ptr, n, gate_buf.ptr, **kw)
            ssd.lib().ssd_device_sync(gpu_device)
            raw = gate_buf.download(gsz * (n + 1)).tobytes()
            assert raw[gsz * n:] == bytes([POISON]) * gsz, "gates past nframes were written"
            for j in range(n):
                assert raw[j * gsz:(j + 1) * gsz] == bytes(ssd.surface_gates_from_moments(want[j], **kw)), idx[j]
            # one pass, then two passes chained with no fetch between
            for passes in (1, 2):
                poisoned(out_buf, rec)
                first_pass()
                refit(first_buf)
                if passes == 2:
                    refit(out_buf)
                again = det.fetch_list(n)
                det.fetch_surface_refit()
                got = records(out_buf)
                assert [bytes(x) for x in again] == lab.res, "the batch's results are still the enqueue's"
                for j, i in enumerate(idx):
                    cur = want[j]
                    for _ in range(passes):
                        gates = ssd.surface_gates_from_moments(cur, **kw)
                        nxt = ssd.surface_refit_moments_host(sw.cfg, sw.frames[i], lab.labels[j], gates, want[j].n_surfaces, want[j].ground, intr=sw.intr)
                        trimmed += sum(int(cur.s[k].m.n) - int(nxt.s[k].m.n) for k in range(cur.n_surfaces))
                        cur = nxt
                    assert bytes(got[j]) == bytes(cur), "frame %d, %d passes: the chain is not the host's" % (i, passes)
        finally:
            r.close()
    assert trimmed > 0, "the gates trim something"


# ---- clearance and tread grid ---------------------------------------------------------------------------------------------------------------
@INPUTS
@FORMS
def test_clearance_and_the_tread_grid(ssd, oracle, gpu_device, depth, cameras):
    """clearance under two rules, and one with an occupant exactly on a shrunk side: records and masks ssd_clearance_host's, and the host
    sums over the device's mask the records; the tread grid under three cells, a lo that is a tread point's distance from its surface and a
    cell that splits the division from its reciprocal: ssd_tread_grid_host's, and sum(occ) + n_occ_out the clearance records' counts
    under the same rule; a second round of every pass
    gives the first round's bytes, allocates nothing, and leaves the detection's results what they were"""
    occupants = 0
    for sw, idx in every_batch(ssd, oracle, depth, cameras):
        r = resident(ssd, gpu_device, sw, idx, cameras)
        try:
            res = r.detect()
            on_margin, on_lo, on_cell = edge_rules(ssd, sw, r, idx)
            # the list holds live frames WITHOUT a ground (one reported surface, a step): the header's flag is the oracle's word
            ground = [1 if sw.live[i] and sw.records[i].ground_ind >= 0 else 0 for i in idx]
            kept, before = [], None
            for turn in range(2):
                now = []
                for rule in CLEAR_RULES + (on_margin,):
                    recs, masks = r.clear(rule)
                    now += [bytes(x) for x in recs] + [masks.tobytes()]
                    if turn == 0:
                        Resident.check(r, rule, recs, masks, ground=ground)        # (MapResident's own check is the stair map's)
                        occupants += sum(int(x.s[k].m.n) for x in recs for k in range(ssd.MAX_STEPS))
                for rule in [tg.RULE[:3] + (cell,) for cell in CELLS] + [on_lo, on_cell]:
                    grids = r.grid(rule)
                    now += [bytes(x) for x in grids]
                    if turn == 0:
                        r.check_grid(rule, grids, ground=ground)
                        r.identity(rule, grids, r.clear(rule[:3], mask=False)[0])
                if turn == 0:
                    kept, before = now, r.det.workspace_bytes
            assert now == kept, "the second round of passes gives the first one's bytes"
            assert r.det.workspace_bytes == before, "the second round of passes allocates nothing that counts"
            assert [bytes(x) for x in r.det.fetch_list(r.n)] == [bytes(x) for x in res], "the results are still the enqueue's"
            for j, i in enumerate(idx):
                if sw.thrown[i] or sw.records[i].n_steps == 0:
                    assert kept[j] == bytes(C.sizeof(ssd.FrameMoments)), "a thrown or empty frame: the all-zero record"
        finally:
            r.close()
    assert occupants > 1000, "outliers above the treads"


# ---- stair map ----------------------------------------------------------------------------------------------------------------------------------
@INPUTS
@FORMS
def test_the_stair_map(ssd, oracle, gpu_device, depth, cameras):
    """one map per staircase (ssd_stair_map_from_results over its live views), every frame of a batch in one call naming its
    staircase's map, thrown frames none: the records are the fold by ssd_tread_grid_add of ssd_tread_grid_host; then the same frames
    in reverse order behind a second handle, accumulated on top: every count twice, every top the same"""
    seen = 0
    for sw, idx in every_batch(ssd, oracle, depth, cameras):
        maps = sw.stair_maps(ssd)
        assert sum(1 for m in maps if m.stairs.n_steps > 0) >= 4 and any(m.stairs.n_steps == 0 for m in maps)
        r = resident(ssd, gpu_device, sw, idx, cameras)
        back = resident(ssd, gpu_device, sw, idx, cameras, reverse=True)
        try:
            res = r.detect()
            index = [NONE if sw.thrown[i] else sw.group[i] for i in idx]
            assert NONE in index and len(set(index)) >= 6
            got = r.fold(maps, tg.RULE, index)
            once = r.want(maps, tg.RULE, index)
            r.check(got, once)
            for m, g in zip(maps, got):
                if m.stairs.n_steps == 0:
                    assert bytes(g) == bytes(C.sizeof(ssd.FrameTreadGrid)), "a staircase no view finds: all zero, the header too"
            seen += sum(int(tg.grid_of_record(g, k)["seen"].sum()) for g in got for k in range(g.n_surfaces))
            back.detect()
            own, back.mout = back.mout, r.mout                     # the second call adds to the first one's records
            try:
                twice = back.fold(maps, tg.RULE, index[::-1], accumulate=True)
            finally:
                back.mout = own
            r.check(twice, r.want(maps, tg.RULE, index, times=2))
            r.check(twice, [ssd.tread_grid_add(b, a) for a, b in zip(once, back.want(maps, tg.RULE, index[::-1]))])
            assert [bytes(x) for x in r.det.fetch_list(r.n)] == [bytes(x) for x in res], "the results are still the enqueue's"
        finally:
            r.close()
            back.close()
    assert seen > 10000


# ---- ground fit and stair pose: no enqueue in front, wide loads ---------------------------------------------------------------------------------
def _frames(ssd, device, sw, aligned):
    return Frames(ssd, device, sw.cfg, sw.cals[0], sw.frames, sw.depth, sw.intr, aligned, batch=sw.n)


@INPUTS
@ALIGNED
def test_the_ground_fit(ssd, oracle, gpu_device, depth, aligned):
    """every frame of the list in one call, a prior per frame: its view's calibration, and the same moved by ground_model.PRIOR_OFF;
    the three tolerances of ground_model.TOLERANCES; the moments are ssd_ground_moments_host's"""
    floors = 0
    for ragged in (False, True):
        sw = ss.sweep(ssd, oracle, depth, ragged)
        offs = [off_prior(ssd, sw, v) for v in range(ss.V)]
        r = _frames(ssd, gpu_device, sw, aligned)
        try:
            for cals in ([sw.cal_of(i) for i in range(sw.n)], [offs[sw.view[i]] for i in range(sw.n)]):
                priors = [(c, sw.intr) if depth else c for c in cals]
                for tol in gm.TOLERANCES:
                    r.det.enqueue_ground_fit(r.ptr, sw.n, tol, priors=priors, depth=depth, stride_bytes=r.stride)
                    fits = r.det.fetch_ground_fit(sw.n, min_points=gm.MIN_POINTS)
                    for i in range(sw.n):
                        want = ssd.ground_moments_host(sw.cfg, priors[i], sw.frames[i], tol, depth=depth)
                        assert bytes(fits[i].m) == bytes(want), (i, tol, gm.moments_tuple(fits[i].m), gm.moments_tuple(want))
                        floors += want.n > gm.MIN_POINTS
        finally:
            r.close()
    assert floors > ss.G * ss.V


@INPUTS
@ALIGNED
def test_the_stair_pose(ssd, oracle, gpu_device, depth, aligned):
    """every frame of the list in one call, under two rules and one with a point on the reach's edge.  A target per staircase and view - its staircase's map under a prior that is
    the view's calibration turned by 2 degrees of yaw and moved 3 cm -, which every frame but the thrown ones names; and a target per
    staircase under view 2's prior, which all six views of the staircase fold into.  Records against ssd_stair_pose_host, poses against
    ssd_stair_pose_solve of the host fold (tests/test_gpu_stair_pose.py's check)"""
    solved = 0
    for ragged in (False, True):
        sw = ss.sweep(ssd, oracle, depth, ragged)
        maps = sw.stair_maps(ssd)
        priors = [pose_prior(ssd, cal) for cal in sw.cals]
        per_view = [spm.target(ssd, priors[v], maps[g], sw.intr) for g in range(ss.G) for v in range(ss.V)]
        per_stair = [spm.target(ssd, priors[2], maps[g], sw.intr) for g in range(ss.G)]
        r = _frames(ssd, gpu_device, sw, aligned)
        try:
            _, (reach, _) = ss.first_edge(sw, lambda i: ss.edge_reach(sw.cfg, priors[sw.view[i]], maps[sw.group[i]], sw.pts[i], spm.RULE)
                                          if maps[sw.group[i]].stairs.n_steps else None)
            for rule in POSE_RULES + (spm.RULE[:3] + (reach,),):        # the last: a riser point exactly reach from its riser's plane
                for targets, index in ((per_view, [NONE if sw.thrown[i] else sw.group[i] * ss.V + sw.view[i] for i in range(sw.n)]),
                                       (per_stair, [NONE if sw.thrown[i] else sw.group[i] for i in range(sw.n)])):
                    recs, poses = _check(ssd, r, targets, index, sw.frames, spm.rule_of(ssd, rule))
                    solved += sum(1 for p in poses if p.status == ssd.GF_OK)
                    for i in range(sw.n):
                        if sw.thrown[i] or maps[sw.group[i]].stairs.n_steps == 0:
                            assert bytes(recs[i]) == bytes(C.sizeof(ssd.StairPoseMoments)), "a frame that names no map, or an empty one: all zero"
        finally:
            r.close()
    assert solved > 10, "staircases whose pose is found"
