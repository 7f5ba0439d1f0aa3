"""The label, moment, refit, gate and riser passes at their full width on the GPU: SSD_MAX_STEPS = 17 surfaces and SSD_MAX_RISERS = 16
risers per frame, on the hand-built frames of tests/full_width.py, whose pixel layouts decide what a wave meets in a point slot (one
surface all through; another surface at every slot; 8 to 17 surfaces in every slot; cells regrouped by the cell list).  Every
comparison is byte for byte against references that owe nothing to the GPU (the oracle, test_labels.expected_labels, the host sums
ssd_surface_moments_host / ssd_surface_refit_moments_host / ssd_surface_gates_from_moments, riser_model), the batches are uploaded at
a stride of frame bytes + 4, and poison lies behind every output.  tests/test_full_width.py checks the frames themselves on the CPU;
profiles/full_width_sabotage.txt records which of these tests fail on builds whose sums are wrong."""
import ctypes as C

import numpy as np
import pytest

import full_width as fw
import parity
import riser_model as rm

pytestmark = pytest.mark.gpu

POISON = 0xA5
FULL, NINE, THREE, BARE = 16, 8, 2, 0
MIN_POINTS, K_SIGMA = 200, 2.5
LABEL_PAD = 37
# one batch: the 9-surface frame and the bare ground sit between 17-surface frames
BATCH = [("ordered", FULL), ("scatter", FULL), ("lanes", FULL), ("slots", FULL), ("sparse", FULL), ("scatter", NINE), ("ordered", BARE), ("scatter", FULL)]
TWO_PASSES, SINGLE_PASS, NO_PLANES = (0, 0), (1, 0), (1, 2)     # Detector.single_pass(mode, sabotage)


def _refs(ssd, oracle, frames=BATCH, w=fw.W, h=fw.H, z=0.5):
    return [fw.reference(ssd, oracle, layout, n_steps, w, h, z) for layout, n_steps in frames]


def _poisoned(ssd, nbytes, device):
    buf = ssd.DeviceBuffer(nbytes, device)
    buf.upload(np.full(nbytes, POISON, dtype=np.uint8))
    return buf


def _moments(ssd, raw, n):
    return list((ssd.FrameMoments * n).from_buffer_copy(np.ascontiguousarray(raw).tobytes()))


def _kept(m, k):
    return int(m.s[k].m.n + m.s[k].n_far)


class Run:
    """everything one handle returns for one batch, as bytes / arrays (see run_on)"""

    PARTS = ("res", "first", "gates", "refit1", "refit2", "chain1", "chain2", "risers", "rmom", "risers_plain")

    def frame_bytes(self, i):
        """frame i's outputs, for comparisons between handles"""
        out = {p: bytes(getattr(self, p)[i]) for p in self.PARTS}
        out["labels"] = self.labels[i].tobytes()
        return out


def open_detector(ssd, device, w, h, n, trans, mode=None, cameras=None):
    det = ssd.Detector(ssd.default_config(w, h, max_frames_per_batch=n), trans, device)
    if cameras is not None:
        det.set_cameras(cameras)
    if mode is not None:
        det.single_pass(*mode)
    return det


def run_on(ssd, det, refs, device, order=None):
    """The batch `refs` through every pass on `det` (order: the camera of each frame - the cameras entry points; None: the one-calibration
    ones): labels; first-pass moments with debug records; the device's gates of them; two host-gated refit passes; one and two refit
    passes chained on the device with no fetch between; risers and riser moments; risers with the moments off.  Checks on the way that
    the poison behind every output is intact and that what must not depend on the pass does not."""
    n, w, h = len(refs), refs[0].width, refs[0].height
    wh, fb = w * h, w * h * 12
    rec, gsz = C.sizeof(ssd.FrameMoments), C.sizeof(ssd.FrameGates)
    stride, lstride = fb + 4, wh + LABEL_PAD
    cam = order is not None
    out = Run()
    bufs = []

    def poisoned(nbytes):
        bufs.append(_poisoned(ssd, nbytes, device))
        return bufs[-1]

    def records(buf):
        raw = buf.download(rec * (n + 1))
        assert np.all(raw[rec * n:] == POISON), "a record past nframes was written"
        return _moments(ssd, raw[:rec * n], n)

    def enqueue_moments(dst):
        if cam:
            det.enqueue_cameras_surface_moments(src.ptr, n, order, dst.ptr, stride_bytes=stride)
        else:
            det.enqueue_surface_moments(src.ptr, n, dst.ptr, stride_bytes=stride)

    def refit_host(gates, dst):
        (det.enqueue_cameras_surface_refit if cam else det.enqueue_surface_refit)(src.ptr, n, gates, dst.ptr, stride_bytes=stride)
        det.fetch_surface_refit()
        return records(dst)

    def refit_device(prev, dst):
        fn = det.enqueue_cameras_surface_refit_device if cam else det.enqueue_surface_refit_device
        fn(src.ptr, n, prev.ptr, dst.ptr, min_points=MIN_POINTS, k_sigma=K_SIGMA, gate_min=0.0, stride_bytes=stride)

    def fetch_raw(fn, kind):
        """ssd_fetch_risers / ssd_fetch_riser_moments into n + 1 poisoned host records: the last one stays poison"""
        arr = (kind * (n + 1))()
        C.memset(arr, POISON, C.sizeof(arr))
        assert fn(det._h, arr, n, None) == 0, ssd.lib().ssd_last_error()
        assert bytes(arr[n]) == bytes([POISON]) * C.sizeof(kind), "a record past nframes was written"
        return [kind.from_buffer_copy(arr[i]) for i in range(n)]

    try:
        src = ssd.DeviceBuffer(stride * n, device)
        bufs.append(src)
        for i, r in enumerate(refs):
            src.upload(np.ascontiguousarray(r.xyz), offset=i * stride)
        assert stride % 16 != 0
        det.set_risers(True, tolerance=fw.TOL, min_support=fw.SUPPORT)
        det.set_riser_moments(True)
        det.set_debug(True, images=False)
        # labels (with them: risers and riser moments of the same enqueue)
        lab = poisoned(lstride * (n + 1))
        if cam:
            det.enqueue_cameras(src.ptr, n, order, d_labels=lab.ptr, label_stride=lstride, stride_bytes=stride)
        else:
            det.enqueue_labels(src.ptr, n, lab.ptr, label_stride=lstride, stride_bytes=stride)
        res_labels = [bytes(r) for r in det.fetch_list(n)]
        raw = lab.download(lstride * (n + 1))
        for i in range(n):
            assert np.all(raw[i * lstride + wh:(i + 1) * lstride] == POISON), "label padding was written"
        assert np.all(raw[n * lstride:] == POISON), "labels past nframes were written"
        out.labels = np.stack([raw[i * lstride:i * lstride + wh] for i in range(n)])
        out.risers = fetch_raw(ssd.lib().ssd_fetch_risers, ssd.FrameRisers)
        out.rmom = fetch_raw(ssd.lib().ssd_fetch_riser_moments, ssd.FrameMoments)
        # first-pass moments, debug records
        first = poisoned(rec * (n + 1))
        enqueue_moments(first)
        out.res = det.fetch_list(n)
        out.first = records(first)
        out.dbg = [det.debug(i) for i in range(n)]
        out.stats = det.single_pass_stats(n)
        assert [bytes(r) for r in out.res] == res_labels, "the results do not depend on what else the enqueue gathers"
        assert [bytes(r) for r in fetch_raw(ssd.lib().ssd_fetch_risers, ssd.FrameRisers)] == [bytes(r) for r in out.risers]
        assert [bytes(r) for r in fetch_raw(ssd.lib().ssd_fetch_riser_moments, ssd.FrameMoments)] == [bytes(r) for r in out.rmom]
        # the device's gates of its own records
        gates = poisoned(gsz * (n + 1))
        det.enqueue_surface_gates(first.ptr, n, gates.ptr, min_points=MIN_POINTS, k_sigma=K_SIGMA, gate_min=0.0)
        assert ssd.lib().ssd_device_sync(device) == 0
        raw = gates.download(gsz * (n + 1))
        assert np.all(raw[gsz * n:] == POISON), "gates past nframes were written"
        out.gates = list((ssd.FrameGates * n).from_buffer_copy(raw[:gsz * n].tobytes()))
        # two refit passes gated on the host
        dst = poisoned(rec * (n + 1))
        out.refit1 = refit_host([ssd.surface_gates_from_moments(m, MIN_POINTS, K_SIGMA, 0.0) for m in out.first], dst)
        dst.upload(np.full(rec * (n + 1), POISON, dtype=np.uint8))
        out.refit2 = refit_host([ssd.surface_gates_from_moments(m, MIN_POINTS, K_SIGMA, 0.0) for m in out.refit1], dst)
        # one pass, then two, chained on the device: no fetch between the enqueues
        for passes in (1, 2):
            for b in (first, dst):
                b.upload(np.full(rec * (n + 1), POISON, dtype=np.uint8))
            enqueue_moments(first)
            refit_device(first, dst)
            if passes == 2:
                refit_device(dst, dst)
            assert [bytes(r) for r in det.fetch_list(n)] == res_labels
            det.fetch_surface_refit()
            setattr(out, "chain%d" % passes, records(dst))
            assert [bytes(m) for m in records(first)] == [bytes(m) for m in out.first], "the chain leaves the first pass's records alone"
        # risers with the moments off
        det.set_riser_moments(False)
        if cam:
            det.enqueue_cameras(src.ptr, n, order, stride_bytes=stride)
        else:
            det.enqueue(src.ptr, n, stride_bytes=stride)
        assert [bytes(r) for r in det.fetch_list(n)] == res_labels
        out.risers_plain = fetch_raw(ssd.lib().ssd_fetch_risers, ssd.FrameRisers)
        det.set_riser_moments(True)
    finally:
        for b in bufs:
            b.free()
    return out


_RUNS = {}


def batch_run(ssd, oracle, device, mode, frames=BATCH, w=fw.W, h=fw.H, z=0.5):
    """the batch behind a fresh one-calibration handle in the given K1 mode: run once, shared by the tests that read it"""
    key = (mode, tuple(frames), w, h, z)
    if key not in _RUNS:
        refs = _refs(ssd, oracle, frames, w, h, z)
        det = open_detector(ssd, device, w, h, len(refs), refs[0].trans, mode)
        try:
            _RUNS[key] = run_on(ssd, det, refs, device)
        except BaseException as e:                      # a batch that failed, or faulted, is not started again by the next test
            _RUNS[key] = e
        finally:
            det.close()
    if isinstance(_RUNS[key], BaseException):
        raise _RUNS[key]
    return _RUNS[key]


_WANT = {}


def host_moments(ssd, ref):
    """ssd_surface_moments_host over the CHECKER's labels, then the two host-gated refit passes over them -> (first, refit1, refit2)"""
    if ref.key not in _WANT:
        n = ref.res.n_steps
        first = ssd.surface_moments_host(ref.cfg, ref.xyz, ref.labels, n, ref.ground)
        chain = [first]
        for _ in range(2):
            gates = ssd.surface_gates_from_moments(chain[-1], MIN_POINTS, K_SIGMA, 0.0)
            chain.append(ssd.surface_refit_moments_host(ref.cfg, ref.xyz, ref.labels, gates, n, ref.ground))
        _WANT[ref.key] = chain
    return _WANT[ref.key]


def check_labels(ssd, refs, run):
    for i, r in enumerate(refs):
        assert run.res[i].n_steps == r.res.n_steps and run.res[i].status == 0, i
        assert np.array_equal(run.labels[i], r.labels), "frame %d (%s): %d labels differ" % (i, r.layout, int((run.labels[i] != r.labels).sum()))
        if r.n_steps == FULL:
            assert np.bincount(run.labels[i], minlength=18)[1:].min() > 0, "all 17 labels are present"


def check_moments(ssd, refs, run):
    zero = bytes(C.sizeof(ssd.SurfaceMoments))
    for i, r in enumerate(refs):
        n = r.res.n_steps
        got, want = run.first[i], host_moments(ssd, r)[0]
        assert (got.n_surfaces, got.ground) == (n, r.ground), i
        for k in range(ssd.MAX_STEPS):
            assert bytes(got.s[k]) == bytes(want.s[k]), "frame %d (%s), surface %d: not the host's sums over the checker's labels" % (i, r.layout, k)
            assert k < n or bytes(got.s[k]) == zero, "frame %d: row %d past n_surfaces is not zero" % (i, k)
        assert bytes(got) == bytes(want), i
        d = run.dbg[i]
        valid = [k for k in range(max(d.first_valid_ind, 0), d.n_plateaus) if d.plateaus[k].valid]
        for k in range(n):
            want_n = d.ground_n_in_quad if k == 0 else d.plateaus[valid[k - 1]].n_in_quad
            assert _kept(got, k) == want_n > 0, (i, k)
        if n == 0:
            assert bytes(got) == bytes(C.sizeof(ssd.FrameMoments)), "the bare ground's record is all zero"


def check_refit(ssd, refs, run):
    for i, r in enumerate(refs):
        n = r.res.n_steps
        first, want1, want2 = host_moments(ssd, r)
        assert bytes(run.gates[i]) == bytes(ssd.surface_gates_from_moments(run.first[i], MIN_POINTS, K_SIGMA, 0.0)), "frame %d: the device's gates" % i
        assert run.gates[i].n_surfaces == n and all(run.gates[i].g[k].gate > 0.0 for k in range(n)), i
        for name, got, want in (("host-gated pass 1", run.refit1, want1), ("host-gated pass 2", run.refit2, want2),
                                ("device chain, pass 1", run.chain1, want1), ("device chain, pass 2", run.chain2, want2)):
            for k in range(ssd.MAX_STEPS):
                assert bytes(got[i].s[k]) == bytes(want.s[k]), "frame %d (%s), %s, surface %d" % (i, r.layout, name, k)
            assert bytes(got[i]) == bytes(want), (i, name)
        for k in range(n):
            assert 0 < _kept(run.refit2[i], k) <= _kept(run.refit1[i], k) < _kept(run.first[i], k), "frame %d, surface %d: trimmed, not emptied" % (i, k)
        if n:
            assert bytes(run.refit1[i]) != bytes(run.refit2[i]), "the second pass moves something"


def check_risers(ssd, refs, run):
    for i, r in enumerate(refs):
        n_r = max(r.res.n_steps - 1, 0)
        parity.compare_risers(run.risers[i], r.risers)
        assert run.risers[i].n_risers == n_r == len(r.risers) and all(run.risers[i].risers[k].detected == 1 for k in range(n_r)), i
        labels = rm.riser_labels(r.cfg, r.cal, run.dbg[i], r.xyz, fw.TOL)
        want = ssd.surface_moments_host(r.cfg, r.xyz, labels, n_r, 0)
        got = run.rmom[i]
        assert (got.n_surfaces, got.ground) == (n_r, 0), i
        for k in range(ssd.MAX_STEPS):
            assert bytes(got.s[k]) == bytes(want.s[k]), "frame %d (%s), riser %d: not the host's sums over the model's labels" % (i, r.layout, k)
        assert bytes(got) == bytes(want), i
        for k in range(n_r):
            assert _kept(got, k) == run.risers[i].risers[k].n_points, (i, k)
        # the same bytes with the moments on and off
        assert bytes(run.risers_plain[i]) == bytes(run.risers[i]), "frame %d: risers with the moments off" % i


def test_labels_at_seventeen_surfaces(ssd, oracle, gpu_device):
    """(a) k_labels: every pixel of every frame of the batch is the checker's label; all 17 labels occur on the 17-surface frames"""
    refs = _refs(ssd, oracle)
    run = batch_run(ssd, oracle, gpu_device, TWO_PASSES)
    assert not run.stats["ran"], "small batches on two passes"
    check_labels(ssd, refs, run)
    assert [r.res.n_steps for r in refs] == [17, 17, 17, 17, 17, 9, 0, 17]
    assert bytes(run.res[1]) == bytes(run.res[7]) and np.array_equal(run.labels[1], run.labels[7]), "the same frame twice in a batch"


def test_surface_moments_at_seventeen_surfaces(ssd, oracle, gpu_device):
    """(b) k_surface_moments: all 17 rows of every record are ssd_surface_moments_host's over the checker's labels, m.n + n_far is the
    debug record's n_in_quad, and the rows at and past n_surfaces are zero - also where a 9-surface frame and the bare ground follow
    17-surface frames in the batch"""
    refs = _refs(ssd, oracle)
    run = batch_run(ssd, oracle, gpu_device, TWO_PASSES)
    check_moments(ssd, refs, run)
    assert bytes(run.first[1]) == bytes(run.first[7])
    for a, b in ((0, 1), (1, 2), (2, 3)):
        assert bytes(run.first[a]) == bytes(run.first[b]), "the layouts of one frame give one record"
    assert bytes(run.first[4]) != bytes(run.first[1])


def test_gates_and_refit_at_seventeen_surfaces(ssd, oracle, gpu_device):
    """(c) k_surface_gates on the device's own 17-surface records against ssd_surface_gates_from_moments; two refit passes, gated on the
    host and chained on the device, against ssd_surface_refit_moments_host over the checker's labels; every surface trimmed, none
    emptied"""
    refs = _refs(ssd, oracle)
    run = batch_run(ssd, oracle, gpu_device, TWO_PASSES)
    check_refit(ssd, refs, run)
    for a, b in ((0, 1), (1, 2), (2, 3), (1, 7)):
        assert bytes(run.chain2[a]) == bytes(run.chain2[b])


def test_risers_at_sixteen(ssd, oracle, gpu_device):
    """(d) k_risers / k_riser_results against the oracle's risers (16 of them, every one detected), k_riser_moments against the host
    sums over riser_model.riser_labels of the handle's own debug record, m.n + n_far = n_points, and n_points and mean_offset the same
    bytes with the moments on and off"""
    refs = _refs(ssd, oracle)
    run = batch_run(ssd, oracle, gpu_device, TWO_PASSES)
    check_risers(ssd, refs, run)
    assert run.risers[1].n_risers == ssd.MAX_RISERS == 16 and run.rmom[1].s[15].m.n > 0


def test_the_riser_rules_edges(ssd, oracle, gpu_device):
    """(e) the tolerance set to exactly |s| of an evidence point of riser 7: the point counts; to the next double below: exactly the
    points with that |s| fall out.  min_support = riser 15's n_points: detected; one more: not, and nothing else changes."""
    r = fw.reference(ssd, oracle, "scatter", FULL)
    run = batch_run(ssd, oracle, gpu_device, TWO_PASSES)
    dbg = run.dbg[1]
    labels, s = rm.evidence(r.cfg, r.cal, dbg, r.xyz, fw.TOL)
    mine = np.abs(s[labels == 8])
    assert len(mine) == run.risers[1].risers[7].n_points
    edge = float(np.sort(mine)[len(mine) // 2])                      # a point in the middle: half the evidence lies beyond it
    below = float(np.nextafter(edge, 0.0))
    on_edge = int((mine == edge).sum())
    assert 0.0 < below < edge < fw.TOL and on_edge >= 1
    det = open_detector(ssd, gpu_device, r.width, r.height, 1, r.trans, TWO_PASSES)
    buf = ssd.DeviceBuffer(r.xyz.nbytes, gpu_device)
    try:
        buf.upload(np.ascontiguousarray(r.xyz))

        def risers(tol, support):
            det.set_risers(True, tolerance=tol, min_support=support)
            det.enqueue(buf.ptr, 1)
            det.fetch_list(1)
            return det.fetch_risers(1)[0]

        counts = []
        for tol in (edge, below):
            got = risers(tol, fw.SUPPORT)
            want = np.bincount(rm.riser_labels(r.cfg, r.cal, dbg, r.xyz, tol), minlength=17)[1:]
            assert [got.risers[k].n_points for k in range(16)] == want.tolist(), tol
            counts.append(got.risers[7].n_points)
        assert counts[0] == int((mine <= edge).sum()) and counts[0] - counts[1] == on_edge
        n15 = run.risers[1].risers[15].n_points
        at, past = risers(fw.TOL, n15), risers(fw.TOL, n15 + 1)
        assert at.risers[15].detected == 1 and past.risers[15].detected == 0 and past.risers[15].n_points == n15
        for k in range(16):
            assert at.risers[k].detected == (1 if at.risers[k].n_points >= n15 else 0), k
            assert past.risers[k].detected == (1 if past.risers[k].n_points >= n15 + 1 else 0), k
            a, p = ssd.Riser.from_buffer_copy(at.risers[k]), ssd.Riser.from_buffer_copy(past.risers[k])
            a.detected = p.detected = 0
            assert bytes(a) == bytes(p), "riser %d: only `detected` depends on min_support" % k
    finally:
        buf.free()
        det.close()


@pytest.mark.parametrize("mode", [SINGLE_PASS, NO_PLANES], ids=["single_pass", "no_planes"])
def test_behind_the_single_pass_and_its_fallback(ssd, oracle, gpu_device, mode):
    """(f) the same batch behind K1's single pass (k_hist_planes rasters the planes) and behind a predictor that hands out no planes
    (every frame falls back to k_raster): labels, moments, gates, both refits, risers and riser moments against the references, and
    every byte the two-pass run's"""
    refs = _refs(ssd, oracle)
    run = batch_run(ssd, oracle, gpu_device, mode)
    st = run.stats
    assert st["ran"] and st["with_steps"] == 7, st
    if mode == NO_PLANES:
        assert st["covered"] == 0 and st["planes"] == 0, st
    else:
        assert st["covered"] > 0 and st["planes"] > 0, st
    check_labels(ssd, refs, run)
    check_moments(ssd, refs, run)
    check_refit(ssd, refs, run)
    check_risers(ssd, refs, run)
    base = batch_run(ssd, oracle, gpu_device, TWO_PASSES)
    for i in range(len(refs)):
        assert run.frame_bytes(i) == base.frame_bytes(i), "frame %d: not the two-pass run's bytes" % i


CAMERA_Z = (0.5, 0.7)
CAMERA_BATCH = [("ordered", FULL, 0), ("scatter", FULL, 1), ("lanes", FULL, 0), ("slots", FULL, 1), ("sparse", FULL, 0), ("scatter", NINE, 1),
                ("ordered", BARE, 0), ("lanes", FULL, 1)]
SECOND_CAMERA = [("scatter", FULL), ("slots", FULL), ("scatter", NINE), ("lanes", FULL)]


def test_camera_batches_equal_the_one_camera_handles(ssd, oracle, gpu_device):
    """(g) two cameras 0.5 m and 0.7 m below the origin behind an identity-calibrated handle, the frames alternating and each built
    for its camera: labels, risers, riser moments, surface moments, host-gated and device-chained refits of every frame are the bytes
    of the one-camera handle of its camera"""
    refs = [fw.reference(ssd, oracle, layout, n_steps, fw.W, fw.H, CAMERA_Z[c]) for layout, n_steps, c in CAMERA_BATCH]
    order = [c for _, _, c in CAMERA_BATCH]
    one = {0.5: (batch_run(ssd, oracle, gpu_device, TWO_PASSES), BATCH),
           0.7: (batch_run(ssd, oracle, gpu_device, TWO_PASSES, SECOND_CAMERA, z=0.7), SECOND_CAMERA)}
    second, second_refs = one[0.7][0], _refs(ssd, oracle, SECOND_CAMERA, z=0.7)
    check_labels(ssd, second_refs, second)
    check_moments(ssd, second_refs, second)
    check_refit(ssd, second_refs, second)
    check_risers(ssd, second_refs, second)
    assert second.frame_bytes(0) != one[0.5][0].frame_bytes(1), "another camera, other camera coordinates, other sums"
    det = open_detector(ssd, gpu_device, fw.W, fw.H, len(refs), ssd.GeometricTransformation(), TWO_PASSES,
                        cameras=[r.trans for r in (refs[0], refs[1])] + [ssd.GeometricTransformation()])
    try:
        run = run_on(ssd, det, refs, gpu_device, order=order)
    finally:
        det.close()
    for i, (layout, n_steps, c) in enumerate(CAMERA_BATCH):
        alone, frames = one[CAMERA_Z[c]]
        j = frames.index((layout, n_steps))
        got, want = run.frame_bytes(i), alone.frame_bytes(j)
        for part in want:
            assert got[part] == want[part], "frame %d (%s, camera %d): %s is not the one-camera handle's" % (i, layout, c, part)


def test_a_narrow_batch_behind_a_full_width_one(ssd, oracle, gpu_device):
    """(h) on one handle a batch of 17-surface frames, then at the same indices the 9-surface frame, the bare ground and a hand-built
    3-surface frame: everything the second batch returns is a fresh handle's, and rows 9 .. 16 (3 .. 16, all) of its records are zero"""
    wide = [("scatter", FULL), ("lanes", FULL), ("slots", FULL)]
    narrow = [("scatter", NINE), ("ordered", BARE), ("scatter", THREE)]
    refs_w, refs_n = _refs(ssd, oracle, wide), _refs(ssd, oracle, narrow)
    fresh = batch_run(ssd, oracle, gpu_device, TWO_PASSES, narrow)
    check_labels(ssd, refs_n, fresh)
    check_moments(ssd, refs_n, fresh)
    check_refit(ssd, refs_n, fresh)
    check_risers(ssd, refs_n, fresh)
    det = open_detector(ssd, gpu_device, fw.W, fw.H, 3, refs_w[0].trans, TWO_PASSES)
    try:
        first = run_on(ssd, det, refs_w, gpu_device)
        assert all(m.n_surfaces == 17 and m.s[16].m.n > 0 for m in first.first + first.chain2) and all(m.s[15].m.n > 0 for m in first.rmom)
        used = run_on(ssd, det, refs_n, gpu_device)
    finally:
        det.close()
    main = batch_run(ssd, oracle, gpu_device, TWO_PASSES)
    for i in range(3):
        assert first.frame_bytes(i) == main.frame_bytes(BATCH.index(wide[i])), "the wide batch is the main batch's frames"
        assert used.frame_bytes(i) == fresh.frame_bytes(i), "frame %d: not a fresh handle's" % i
    zero = bytes(C.sizeof(ssd.SurfaceMoments))
    for i, n in enumerate((9, 0, 3)):
        for part in ("first", "refit1", "refit2", "chain1", "chain2"):
            m = getattr(used, part)[i]
            assert m.n_surfaces == n and all(bytes(m.s[k]) == zero for k in range(n, 17)), (i, part)
        assert used.gates[i].n_surfaces == n and bytes(used.gates[i])[8 + n * C.sizeof(ssd.PlaneGate):] == bytes((17 - n) * C.sizeof(ssd.PlaneGate))
        assert used.rmom[i].n_surfaces == max(n - 1, 0) and all(bytes(used.rmom[i].s[k]) == zero for k in range(max(n - 1, 0), 17))
        assert used.risers[i].n_risers == max(n - 1, 0)
        assert bytes(used.risers[i])[8 + max(n - 1, 0) * C.sizeof(ssd.Riser):] == bytes((16 - max(n - 1, 0)) * C.sizeof(ssd.Riser)), "risers past n_risers"


def test_one_step_past_the_width(ssd, oracle, gpu_device):
    """(i) ground plus 17 step plateaus at 800 x 600 (18 plateaus on the oracle's record): the handle flags SSD_ST_OVERFLOW and stays
    inside its tables - n_steps <= 17, labels <= n_steps, n_risers <= 16 -, its moments are the host sums over ITS labels and its riser
    moments those over riser_labels of its debug record (the oracle knows no limit and is no reference here), and the poison behind
    every record, the labels and the riser buffers is intact (run_on)"""
    w, h = 800, 600
    over = fw.reference(ssd, oracle, "scatter", 17, w, h, fill=1.25)
    full = fw.reference(ssd, oracle, "lanes", FULL, w, h)
    assert (over.res.n_plateaus, over.res.n_steps) == (18, 18) and full.res.n_steps == 17
    refs = [over, full, over]
    det = open_detector(ssd, gpu_device, w, h, 3, over.trans, TWO_PASSES)
    try:
        run = run_on(ssd, det, refs, gpu_device)
    finally:
        det.close()
    check_labels(ssd, [full], _one(run, 1))
    check_moments(ssd, [full], _one(run, 1))
    check_risers(ssd, [full], _one(run, 1))
    assert run.frame_bytes(0) == run.frame_bytes(2)
    for i in (0, 2):
        res, lab = run.res[i], run.labels[i]
        assert res.status & ssd.ST_OVERFLOW and not (res.status & ssd.ST_THROW), res.status
        assert res.n_steps == 17 and int(lab.max()) == 17 and run.risers[i].n_risers == 16
        assert np.bincount(lab, minlength=18)[1:].min() > 0
        for part in ("first", "refit1", "refit2", "chain1", "chain2"):
            assert getattr(run, part)[i].n_surfaces == 17, part
        want = ssd.surface_moments_host(over.cfg, over.xyz, lab, 17, 1)
        assert bytes(run.first[i]) == bytes(want), "the overflowing frame's moments are the host sums over the handle's labels"
        cur = want
        for name in ("refit1", "refit2"):
            gates = ssd.surface_gates_from_moments(cur, MIN_POINTS, K_SIGMA, 0.0)
            cur = ssd.surface_refit_moments_host(over.cfg, over.xyz, lab, gates, 17, 1)
            assert bytes(getattr(run, name)[i]) == bytes(cur), name
        assert bytes(run.chain1[i]) == bytes(run.refit1[i]) and bytes(run.chain2[i]) == bytes(run.refit2[i])
        assert bytes(run.gates[i]) == bytes(ssd.surface_gates_from_moments(run.first[i], MIN_POINTS, K_SIGMA, 0.0))
        rl = rm.riser_labels(over.cfg, over.cal, run.dbg[i], over.xyz, fw.TOL, limit=ssd.MAX_STEPS)
        assert int(rl.max()) == 16
        assert bytes(run.rmom[i]) == bytes(ssd.surface_moments_host(over.cfg, over.xyz, rl, 16, 0)), "riser moments over the debug record's risers"
        assert [run.risers[i].risers[k].n_points for k in range(16)] == np.bincount(rl, minlength=17)[1:].tolist()
        assert bytes(run.risers_plain[i]) == bytes(run.risers[i])
        # the 17 surfaces the handle keeps are the oracle's lowest 17, point for point
        assert [_kept(run.first[i], k) for k in range(17)] == [over.res.ground_n_in_quad] + [over.res.plateaus[k].n_in_quad for k in range(1, 17)]


def _one(run, i):
    """frame i of a run as a run of its own"""
    out = Run()
    for name in Run.PARTS + ("dbg",):
        setattr(out, name, [getattr(run, name)[i]])
    out.labels = run.labels[i:i + 1]
    return out


def test_the_ragged_frame(ssd, oracle, gpu_device):
    """(j) 642 x 479 = 307,518 points, no multiple of 4 or of 64 (the 12-byte load path, a partial last cell), 17 surfaces in every
    layout: labels, surface moments, refits and risers"""
    frames = [(l, FULL) for l in fw.LAYOUTS]
    refs = _refs(ssd, oracle, frames, 642, 479)
    assert (642 * 479) % 4 != 0 and all(r.res.n_steps == 17 for r in refs)
    assert refs[1].xyz.reshape(-1, 3)[642 * 479 // 64 * 64:, 2].any(), "the partial last cell holds a point"
    run = batch_run(ssd, oracle, gpu_device, TWO_PASSES, frames, 642, 479)
    check_labels(ssd, refs, run)
    check_moments(ssd, refs, run)
    check_refit(ssd, refs, run)
    check_risers(ssd, refs, run)
