"""The slice feed of the host entry points (ssd_capi.hip, SliceFeed): every ssd_process_*host* call cuts its batch
into slices and stages them through the handle's two ingest buffers.  What the other suites do not reach: the refit paths over more
than two slices (the third slice reuses the first one's buffer), one handle taking every kind of host call in turn (the feeds share the
buffers, the copy streams, the events and the label staging), and the ground fit's padded copy of vertex frames.  Every record on these
paths is integer sums or a deterministic solve of them, so every comparison is byte for byte."""
import numpy as np
import pytest

import surface_model as sm
import test_gpu_camera_surfaces as cs
from test_gpu_ground_fit import TOL, _set, _upload

W, H, N = 256, 192, 5


def _staircases(ssd, w=W, h=H, poses=None):
    """five frames, every fifth scene without stairs (the first); poses: one per camera, cycling"""
    return [ssd.make_scene(w, h, n_steps=3 if i % 5 else 0, seed=100 + i, sigma=0.001 + 0.0002 * (i % 4),
                           **(poses[i % len(poses)] if poses else dict(roll_deg=25.0))) for i in range(N)]


def _b(records):
    return [bytes(r) for r in records]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])
@pytest.mark.parametrize("cameras", [False, True], ids=["one-calibration", "four-cameras"])
def test_refit_over_three_slices_through_two_buffers(ssd, gpu_device, cameras, depth):
    """five frames on a handle of two frames per batch: slices of 2, 2 and 1, the third in the first one's buffer - results, first-pass
    records, refit records and fits equal those of a handle that takes the five frames as one slice; host gates and device gates"""
    scs = _staircases(ssd, poses=cs.POSES if cameras else None)
    which = [i % 4 for i in range(N)]
    frames = ssd.synth_depth_host(scs) if depth else ssd.synth_host(scs)
    trans = [ssd.transformation_for_scene(scs[j]) for j in range(4)]          # camera j: scene j's pose (one pose without cameras)
    assert all(bytes(ssd.transformation_for_scene(scs[i]).constants) == bytes(trans[which[i]].constants) for i in range(N))
    intr = ssd.intrinsics_for_scene(scs[0])

    def run(max_frames, device_gates):
        cfg = ssd.default_config(W, H, max_frames_per_batch=max_frames)
        det = cs._identity_detector(ssd, cfg, gpu_device) if cameras else ssd.Detector(cfg, trans[0], gpu_device)
        try:
            kw = dict(depth=depth, min_points=sm.MIN_POINTS, k_sigma=2.5, gate_min=0.0, passes=2, moments=True, device_gates=device_gates)
            if cameras:
                det.set_cameras([(t, intr) for t in trans] if depth else trans)
                return [_b(x) for x in det.process_host_cameras_surfaces_refit(frames, which, **kw)]
            if depth:
                det.set_intrinsics(intr)
            return [_b(x) for x in det.process_host_surfaces_refit(frames, **kw)]
        finally:
            det.close()

    for device_gates in (False, True):
        res, fits, first, refit = run(2, device_gates)
        assert [res, fits, first, refit] == run(8, device_gates), device_gates
        assert len(res) == N and len(set(first[1:])) == N - 1 and first != refit, "staircases, all different, and the gates trim them"
        assert first[0] == bytes(len(first[0])) and refit[0] == first[0], "the frame without stairs has no records"


def _every_call(ssd, det, frames, tol):
    """the calls of the test below, by name"""
    def riser_fits():
        det.set_risers(True)
        try:
            return det.process_host_riser_fits(frames, moments=True)
        finally:
            det.set_risers(False)

    def labels():
        res, lab = det.process_host_labels(frames)
        return res, [lab.tobytes()]

    return dict(process_host=lambda: (det.process_host(frames),),
                ground_fit=lambda: (det.process_host_ground_fit(frames, tol, min_points=300),),
                surfaces_refit=lambda: det.process_host_surfaces_refit(frames, min_points=sm.MIN_POINTS, passes=2, moments=True),
                labels=labels, riser_fits=riser_fits)


# 250 x 191: 47,750 points, no multiple of four - a vertex frame is 573,000 bytes where the ground fit stages it at 573,008, so its call
# re-makes the staging buffers between the others' and takes the padded copy; at 256 x 192 every call finds the buffers as they are
@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(W, H), (250, 191)], ids=["256x192", "250x191"])
def test_one_handle_takes_every_kind_of_host_call_in_turn(ssd, gpu_device, w, h):
    """two frames per batch, three workspaces, five frames: each call equals the same call on a fresh handle, the last process_host the
    first"""
    scs = _staircases(ssd, w, h)
    trans = ssd.transformation_for_scene(scs[0])
    frames = ssd.synth_host(scs)
    cfg = ssd.default_config(w, h, max_frames_per_batch=2, batches_in_flight=3)
    order = ["process_host", "ground_fit", "surfaces_refit", "labels", "riser_fits", "process_host"]

    def as_bytes(out):
        return [x if isinstance(x[0], bytes) else _b(x) for x in out]

    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        calls = _every_call(ssd, det, frames, TOL)
        got = [as_bytes(calls[name]()) for name in order]
    finally:
        det.close()
    assert got[-1] == got[0]
    for name, mine in zip(order[:-1], got):
        fresh = ssd.Detector(cfg, trans, gpu_device)
        try:
            assert as_bytes(_every_call(ssd, fresh, frames, TOL)[name]()) == mine, name
        finally:
            fresh.close()
    (results,), (ground_fits,), (_, (labels,)) = got[0], got[1], got[3]
    assert max(ssd.FrameResult.from_buffer_copy(r).n_steps for r in results) >= 3, "staircases are in sight"
    assert len(set(ground_fits)) == N and len(set(labels)) > 2, "ground fits that differ, labels of several surfaces"


@pytest.mark.gpu
def test_ground_fit_pads_vertex_frames_of_a_point_count_that_is_no_multiple_of_four(ssd, gpu_device):
    """31 x 29 = 899 points: 10,788 bytes a frame, staged at 10,800 by the pitched copy.  Seventy frames, seventy priors, three slices,
    against the enqueue path over the packed frames, as test_host_path_over_three_slices_equals_the_enqueue_path"""
    w, h, n = 31, 29, 70
    assert (12 * w * h) % 16 != 0
    d = _set(ssd, w, h)
    which = [(3 * k + k // 7) % 5 for k in range(n)]
    frames = np.ascontiguousarray(np.stack([d["xyz"][j] for j in which]))
    priors = []
    for k in range(n):
        cam = ssd.Camera()
        cam.cal = d["priors"][which[k]]
        cam.cal.b[2] += 1e-4 * k
        priors.append(cam)
    cfg = ssd.default_config(w, h, max_frames_per_batch=n)
    det = ssd.Detector(cfg, d["priors"][0], gpu_device)
    buf = _upload(ssd, frames, gpu_device)
    try:
        det.enqueue_ground_fit(buf.ptr, n, TOL, priors=priors)
        want = [bytes(f) for f in det.fetch_ground_fit(n, min_points=30)]
        for k in (0, 31, 32, 69):
            m = ssd.ground_moments_host(cfg, priors[k], frames[k], TOL)
            assert bytes(ssd.ground_fit_solve(m, priors[k], 30)) == want[k], k
        assert len(set(want)) > 60
        assert [bytes(f) for f in det.process_host_ground_fit(frames, TOL, priors=priors, min_points=30)] == want
    finally:
        buf.free()
        det.close()
