"""The order of the passes a handle keeps in call order (ssd_ordered_pass): the clearance pass, the tread grid, the
trimmed refit with host gates and the ground fit.  Each is called twice with no host wait between the calls - on stream B, then on stream
A with another rule into the SAME buffer - behind a whole enqueue on stream A of a handle with one workspace.  The library has to order the
second call behind the first (the record's event wait on a switch of streams), so that what the pass's fetch finds in the buffer is the
LAST call's records: byte for byte the host function's for that call's rule.

This guards the order; it cannot prove it.  A lost wait shows only when the race is lost - when the first call's kernel is still writing
as the second call's zeroing or kernel runs - and two small passes on an idle device may well finish in call order by themselves.

Frames: the two-frame scene batch of test_gpu_clearance.py's refusal test; streams made by ctypes on libamdhip64.so as
test_gpu_configs.py::test_calls_on_different_streams_are_ordered_by_the_library makes them."""
import ctypes as C

import numpy as np
import pytest

import clearance_model as cm
import tread_grid_model as tg
from test_gpu_clearance import POISON, Resident, _scene_batch

pytestmark = pytest.mark.gpu

TOLERANCES = (0.08, 0.012)                 # the ground fit's two calls (refine_calibration's first and last)
# The clearance pass's calls.  On these frames (sigma 1 mm) cm.RULE and cm.WIDE_RULE gather the same occupants - nothing lies between 1 cm
# and 3 cm above a tread -, so a third call, back on stream B, takes the rule without a margin, under which the riser faces leak in
CLEARANCE_RULES = (cm.RULE, cm.WIDE_RULE, (0.0, 0.02, 0.4))


@pytest.fixture(scope="module")
def batch(ssd, oracle):
    cfg, trans, intr, frames, pulled = _scene_batch(ssd, oracle, False)
    cfg.max_frames_per_batch = 2
    cfg.batches_in_flight = 1              # one workspace: every call on the caller's stream
    return cfg, trans, frames[:2]


@pytest.fixture
def two_streams():
    hip = C.CDLL("libamdhip64.so")          # the runtime libssd_hip.so already runs on
    streams = []
    for _ in range(2):
        st = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0          # hipStreamNonBlocking
        streams.append(st)
    yield streams[0].value, streams[1].value
    for st in streams:
        assert hip.hipStreamDestroy(st) == 0


def _download(ssd, buf, kind, n):
    return list((kind * n).from_buffer_copy(buf.download(C.sizeof(kind) * n).tobytes()))


def _live(ssd, r):
    return 1 if r.n_steps > 0 and not (r.status & ssd.ST_THROW) else 0


def test_clearance_on_another_stream_goes_behind_the_pass_before(ssd, oracle, gpu_device, batch, two_streams):
    cfg, trans, frames = batch
    a, b = two_streams
    r = Resident(ssd, gpu_device, cfg, trans, frames)
    try:
        det = r.det
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride, stream=a)
        r.out.upload(np.full(r.rec * 3, POISON, dtype=np.uint8))
        for rule, stream in zip(CLEARANCE_RULES, (b, a, b)):               # no host wait between them
            det.enqueue_clearance(r.src.ptr, 2, r.out.ptr, cm.rule_of(ssd, rule), stride_bytes=r.stride, stream=stream)
        det.fetch_clearance()
        got = _download(ssd, r.out, ssd.FrameMoments, 2)
        res = det.fetch_list(2)
        want = [[ssd.clearance_host(cfg, r.cal, frames[i], res[i], _live(ssd, res[i]), cm.rule_of(ssd, rule), mask=False)[0] for i in range(2)]
                for rule in CLEARANCE_RULES]
        assert all([bytes(x) for x in w] != [bytes(x) for x in want[2]] for w in want[:2]), "the last rule gives different records"
        assert [bytes(x) for x in got] == [bytes(x) for x in want[2]], "the records are the last call's"
    finally:
        r.close()


def test_tread_grid_on_another_stream_goes_behind_the_pass_before(ssd, oracle, gpu_device, batch, two_streams):
    cfg, trans, frames = batch
    a, b = two_streams
    r = Resident(ssd, gpu_device, cfg, trans, frames)
    try:
        det = r.det
        grec = C.sizeof(ssd.FrameTreadGrid)
        out = ssd.DeviceBuffer(grec * 2, gpu_device)
        r.bufs.append(out)
        det.enqueue(r.src.ptr, 2, stride_bytes=r.stride, stream=a)
        out.upload(np.full(grec * 2, POISON, dtype=np.uint8))
        for rule, stream in ((tg.RULE, b), (tg.WIDE_RULE, a)):             # no host wait between the two
            det.enqueue_tread_grid(r.src.ptr, 2, out.ptr, tg.rule_of(ssd, rule), stride_bytes=r.stride, stream=stream)
        det.fetch_tread_grid()
        got = _download(ssd, out, ssd.FrameTreadGrid, 2)
        res = det.fetch_list(2)
        want = [[ssd.tread_grid_host(cfg, r.cal, frames[i], res[i], _live(ssd, res[i]), tg.rule_of(ssd, rule)) for i in range(2)]
                for rule in (tg.RULE, tg.WIDE_RULE)]
        assert [bytes(x) for x in want[0]] != [bytes(x) for x in want[1]], "the two rules give different records"
        assert [bytes(x) for x in got] == [bytes(x) for x in want[1]], "the records are the second call's"
    finally:
        r.close()


def test_refit_with_host_gates_on_another_stream_goes_behind_the_pass_before(ssd, oracle, gpu_device, batch, two_streams):
    """a huge gate (the first pass's records), then a zero gate (nothing but the header)"""
    cfg, trans, frames = batch
    a, b = two_streams
    r = Resident(ssd, gpu_device, cfg, trans, frames)
    try:
        det, wh = r.det, r.wh
        lab = ssd.DeviceBuffer(wh * 2, gpu_device)
        first = ssd.DeviceBuffer(r.rec * 2, gpu_device)
        r.bufs += [lab, first]
        det.enqueue_labels(r.src.ptr, 2, lab.ptr, stride_bytes=r.stride, stream=a)
        det.fetch_list(2)
        labels = lab.download(wh * 2).reshape(2, wh).copy()
        det.enqueue_surface_moments(r.src.ptr, 2, first.ptr, stride_bytes=r.stride, stream=a)      # the whole enqueue the refits follow
        det.fetch_list(2)
        moments = _download(ssd, first, ssd.FrameMoments, 2)
        assert all(m.n_surfaces >= 3 for m in moments)
        gates = []
        for gate in (1e9, 0.0):
            gs = [ssd.surface_gates_from_moments(m, 200, 2.5, 0.0) for m in moments]
            for g in gs:
                for k in range(ssd.MAX_STEPS):
                    g.g[k].gate = gate
            gates.append(gs)
        r.out.upload(np.full(r.rec * 3, POISON, dtype=np.uint8))
        for gs, stream in zip(gates, (b, a)):                              # no host wait between the two
            det.enqueue_surface_refit(r.src.ptr, 2, gs, r.out.ptr, stride_bytes=r.stride, stream=stream)
        det.fetch_surface_refit()
        got = _download(ssd, r.out, ssd.FrameMoments, 2)
        want = [[ssd.surface_refit_moments_host(cfg, frames[i], labels[i], gs[i], moments[i].n_surfaces, moments[i].ground) for i in range(2)]
                for gs in gates]
        assert [bytes(x) for x in want[0]] == [bytes(m) for m in moments], "a gate of 1e9 keeps every labelled point"
        assert all(bytes(x)[8:] == bytes(r.rec - 8) for x in want[1]), "a zero gate keeps none"
        assert [bytes(x) for x in got] == [bytes(x) for x in want[1]], "the records are the second call's"
    finally:
        r.close()


def test_ground_fit_on_another_stream_goes_behind_the_call_before(ssd, oracle, gpu_device, batch, two_streams):
    """the ground fit's records are the handle's own: one fetch returns the second call's fits"""
    cfg, trans, frames = batch
    a, b = two_streams
    r = Resident(ssd, gpu_device, cfg, trans, frames)
    try:
        det = r.det
        for tol, stream in zip(TOLERANCES, (b, a)):                        # no host wait between the two
            det.enqueue_ground_fit(r.src.ptr, 2, tol, stride_bytes=r.stride, stream=stream)
        got = det.fetch_ground_fit(2)
        want = [[ssd.ground_fit_solve(ssd.ground_moments_host(cfg, r.cal, frames[i], tol), r.cal, 2000) for i in range(2)] for tol in TOLERANCES]
        assert [bytes(x.m) for x in want[0]] != [bytes(x.m) for x in want[1]], "the two tolerances give different moments"
        assert [bytes(x) for x in got] == [bytes(x) for x in want[1]], "the fits are the second call's"
    finally:
        r.close()
