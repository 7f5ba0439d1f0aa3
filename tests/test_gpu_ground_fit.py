"""The ground fit on the GPU (ssd_enqueue_ground_fit / ssd_fetch_ground_fit / ssd_process_host_ground_fit; include/ssd_hip.h, DESIGN.md
section 7c).  The contract under test: the device's moments are, bit for bit, ssd_ground_moments_host's and the numpy restatement's
(tests/ground_model.py) - sums of integers, whatever the order - for shapes whose point count divides no unit of the kernel, strides
with padding that would count, both inputs, every form of priors; the calls leave detection batches alone; and a calibration refined
from five frames' own floors makes the detector report what the true calibrations make it report.  Small shapes: 64 x 50, 250 x 190,
256 x 192 (the kernel's paths depend on alignment and tails, not on size), 640 x 480 where steps must be detected."""
import numpy as np
import pytest

import ground_model as gm
import scenes
from test_ground_fit import boundary_cloud

F = 8
TOL = 0.08
_cache = {}


def _set(ssd, w, h):
    """five frames of five poses at w x h, as vertices and as 16-bit depth, with five different priors; host and numpy moments cached"""
    key = (w, h)
    if key not in _cache:
        kinds = ["steps", "floor", "outliers", "invalid", "steps"]
        poses = [dict(), dict(pitch_deg=47.0), dict(roll_deg=1.5, cam_height=1.03), dict(pitch_deg=52.0, roll_deg=-1.0), dict(cam_height=0.97, seed=11)]
        scs = [gm.scene(ssd, k, width=w, height=h, **p) for k, p in zip(kinds, poses)]
        signs = [+1, -1, +1, -1, 0]
        priors = [ssd.transformation_for_scene(gm.scene(ssd, k, width=w, height=h, sign=s, **p)).constants for k, p, s in zip(kinds, poses, signs)]
        _cache[key] = dict(w=w, h=h, scenes=scs, priors=priors, intr=[ssd.intrinsics_for_scene(sc) for sc in scs],
                           xyz=ssd.synth_host(scs), depth=ssd.synth_depth_host(scs), cfg=ssd.default_config(w, h, max_frames_per_batch=F), want={})
    return _cache[key]


def _want(ssd, d, frame, prior, depth, tol=TOL):
    """frame `frame` under prior `prior` of the set: the host function's moments, checked once against the numpy restatement"""
    key = (frame, prior, depth, tol)
    if key not in d["want"]:
        cal = d["priors"][prior]
        if depth:
            m = ssd.ground_moments_host(d["cfg"], (cal, d["intr"][prior]), d["depth"][frame], tol, depth=True)
            pts = ssd.deproject_host(d["intr"][prior], d["depth"][frame])
        else:
            m = ssd.ground_moments_host(d["cfg"], cal, d["xyz"][frame], tol)
            pts = d["xyz"][frame]
        t = gm.moments_tuple(m)
        assert t == gm.moments_np(d["cfg"], cal, pts, tol)
        d["want"][key] = t
    return d["want"][key]


def _prior_arg(d, idx, depth):
    return [(d["priors"][i], d["intr"][i]) if depth else d["priors"][i] for i in idx]


def _upload(ssd, a, device):
    a = np.ascontiguousarray(a)
    buf = ssd.DeviceBuffer(a.nbytes, device)
    buf.upload(a)
    return buf


def _moments(fits):
    return [gm.moments_tuple(f.m) for f in fits]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])
@pytest.mark.parametrize("shape", [(250, 190), (64, 50), (256, 192)], ids=lambda s: "%dx%d" % s)
def test_moments_bit_equal_every_form_of_priors(ssd, gpu_device, shape, depth):
    d = _set(ssd, *shape)
    frames = d["depth"] if depth else d["xyz"]
    det = ssd.Detector(d["cfg"], d["priors"][0], gpu_device)
    buf = _upload(ssd, frames, gpu_device)
    try:
        if depth:
            det.set_intrinsics(d["intr"][0])
        seen = 0
        for n in (1, 5):
            # npriors = 0: the handle's calibration (prior 0); 1: prior 3 for every frame; nframes: frame i under prior i, all different
            for priors, which in ((None, [0] * n), (_prior_arg(d, [3], depth), [3] * n), (_prior_arg(d, range(n), depth), list(range(n)))):
                det.enqueue_ground_fit(buf.ptr, n, TOL, priors=priors, depth=depth)
                got = _moments(det.fetch_ground_fit(n, min_points=1))
                want = [_want(ssd, d, i, which[i], depth) for i in range(n)]
                assert got == want, (n, which)
                seen += sum(1 for t in got if t[0] > 200)
        assert seen >= 10, "the frames show floor under these priors"
        assert len({repr(_want(ssd, d, i, i, depth)) for i in range(5)}) == 5
    finally:
        buf.free()
        det.close()


def _pad_count(frame_elems, per16, pad_elems):
    """elements of padding (a multiple of 3, so whole points for vertices; at least 96) behind a frame of frame_elems elements, per16 of
    which make 16 bytes: pad_elems = 16 brings the stride to a multiple of 16 bytes, pad_elems = 1 leaves it none"""
    n = 96
    while (frame_elems + n) % per16 != 0:
        n += 3
    return n if pad_elems == 16 else n + 3


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])
@pytest.mark.parametrize("pad_elems", [16, 1], ids=["stride-16B-multiple", "stride-odd"])
def test_stride_with_padding_that_would_count(ssd, gpu_device, depth, pad_elems):
    """a stride larger than the frame, the padding full of floor points: none of it is read (both the wide and the one-point loop:
    the odd stride takes frames 1.. off the 16-byte boundary)"""
    w, h = 250, 190
    d = _set(ssd, w, h)
    n = 3
    if depth:
        pad = np.repeat(d["depth"][1][h // 2, w // 2], _pad_count(w * h, 8, pad_elems))   # a floor pixel's depth, over and over
        rows = [np.concatenate([d["depth"][i].ravel(), pad]) for i in range(n)]
        elem = 2
    else:
        p = d["xyz"][1][h // 2, w // 2]
        one = np.zeros_like(d["xyz"][1])
        one[0, 0] = p
        assert ssd.ground_moments_host(d["cfg"], d["priors"][1], one, TOL).n == 1, "the padding's point is a floor point"
        pad = np.tile(p, _pad_count(3 * w * h, 4, pad_elems) // 3)
        rows = [np.concatenate([d["xyz"][i].ravel(), pad]) for i in range(n)]
        elem = 4
    packed = np.stack(rows)
    stride = packed.shape[1] * elem
    assert (stride % 16 == 0) == (pad_elems == 16)
    det = ssd.Detector(d["cfg"], d["priors"][0], gpu_device)
    buf = _upload(ssd, packed, gpu_device)
    try:
        det.enqueue_ground_fit(buf.ptr, n, TOL, priors=_prior_arg(d, [1], depth), depth=depth, stride_bytes=stride)
        assert _moments(det.fetch_ground_fit(n, min_points=1)) == [_want(ssd, d, i, 1, depth) for i in range(n)]
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
def test_largest_sums_and_empty_frames(ssd, gpu_device):
    """every point a floor point with q = 2^20 - 1 in all three coordinates - the largest sums 256 x 192 allows (n 2^40 = 5.4e16 per
    product sum) -, an all-zero frame, and a saturated depth frame"""
    w, h = 256, 192
    cfg = ssd.default_config(w, h, max_frames_per_batch=F)
    cfg.x_min, cfg.x_max, cfg.y_min, cfg.y_max = -20.0, 20.0, -20.0, 20.0
    cal = ssd.GeometricTransformation().constants
    cal.b[2] = -15.5
    v = np.float32(15.99999)
    q = int(np.rint(np.float64(v) * 65536))
    assert q == 2 ** 20 - 1
    full = np.full((h, w, 3), v, dtype=np.float32)
    frames = np.stack([full, np.zeros_like(full), -full])
    n = w * h
    det = ssd.Detector(cfg, cal, gpu_device)
    buf = _upload(ssd, frames, gpu_device)
    sc = gm.scene(ssd, "floor")
    intr = ssd.intrinsics_for_scene(sc)
    # 62000 x 0.25 mm = 15.5 m: every pixel a floor point here; 65535 is 16.4 m: none (q >= 2^20); and the all-zero frame
    depth = np.stack([np.full((h, w), 62000, dtype=np.uint16), np.full((h, w), 65535, dtype=np.uint16), np.zeros((h, w), dtype=np.uint16)])
    dbuf = _upload(ssd, depth, gpu_device)
    try:
        det.enqueue_ground_fit(buf.ptr, 3, 1.0)
        fits = det.fetch_ground_fit(3, min_points=1)
        assert _moments(fits) == [(n, [n * q] * 3, [n * q * q] * 6), (0, [0] * 3, [0] * 6), (0, [0] * 3, [0] * 6)]
        assert _moments(fits)[0] == gm.moments_tuple(ssd.ground_moments_host(cfg, cal, full, 1.0))
        assert [f.status for f in fits] == [ssd.GF_DEGENERATE, ssd.GF_FEW, ssd.GF_FEW]     # one point 49152 times is no plane
        det.set_intrinsics(intr)
        det.enqueue_ground_fit(dbuf.ptr, 3, 1.0, depth=True)
        got = _moments(det.fetch_ground_fit(3, min_points=1))
        assert got == [gm.moments_tuple(ssd.ground_moments_host(cfg, (cal, intr), f, 1.0, depth=True)) for f in depth]
        assert [t[0] for t in got] == [n, 0, 0]
    finally:
        buf.free()
        dbuf.free()
        det.close()


@pytest.mark.gpu
def test_boundary_cloud_on_the_device(ssd, gpu_device):
    cfg, cal, pts, tol, inside = boundary_cloud(ssd)
    cfg.max_frames_per_batch = 2
    det = ssd.Detector(cfg, cal, gpu_device)
    flat = pts.reshape(-1, 3)
    buf = ssd.DeviceBuffer(pts.nbytes, gpu_device)
    try:
        buf.upload(pts)
        det.enqueue_ground_fit(buf.ptr, 1, tol)
        got = _moments(det.fetch_ground_fit(1, min_points=1))[0]
        assert got == gm.moments_tuple(ssd.ground_moments_host(cfg, cal, pts, tol)) and got[0] == sum(inside)
        # point by point, each at a slot of its own: points 0 .. 31 of the frame, so every lane position of the wide loop's unit
        for i, want in enumerate(inside):
            one = np.zeros_like(flat)
            one[i] = flat[i]
            buf.upload(one)
            det.enqueue_ground_fit(buf.ptr, 1, tol)
            assert det.fetch_ground_fit(1, min_points=1)[0].m.n == (1 if want else 0), (i, flat[i])
    finally:
        buf.free()
        det.close()


@pytest.mark.gpu
def test_fetch_is_the_host_solve_and_contracts(ssd, gpu_device):
    d = _set(ssd, 256, 192)
    det = ssd.Detector(d["cfg"], d["priors"][0], gpu_device)
    buf = _upload(ssd, d["xyz"], gpu_device)
    dbuf = _upload(ssd, d["depth"], gpu_device)
    try:
        base = det.workspace_bytes
        det.enqueue(buf.ptr, 2)
        det.fetch(2)
        with pytest.raises(ssd.SsdError, match="last ssd_enqueue_ground_fit"):
            det.fetch_ground_fit(1)
        # refusals, before anything is made or launched
        for kw, what in ((dict(priors=_prior_arg(d, [0, 1], False)), "npriors"), (dict(depth=True), "ssd_set_intrinsics"),
                         (dict(priors=[d["priors"][0]], depth=True), "intrinsics")):
            with pytest.raises(ssd.SsdError, match=what):
                det.enqueue_ground_fit(dbuf.ptr if kw.get("depth") else buf.ptr, 5, TOL, **kw)
        with pytest.raises(ssd.SsdError, match="max_frames_per_batch"):
            det.enqueue_ground_fit(buf.ptr, F + 1, TOL)
        for tol in (0.0, -0.1, 1.0001, float("nan")):
            with pytest.raises(ssd.SsdError, match="tol"):
                det.enqueue_ground_fit(buf.ptr, 5, tol)
        assert det.workspace_bytes == base, "nothing allocated until the first ground-fit call"
        priors = _prior_arg(d, range(5), False)
        det.enqueue_ground_fit(buf.ptr, 5, TOL, priors=priors)
        assert det.workspace_bytes == base + F * (80 + 128)
        for min_points in (2000, 10 ** 6):
            fits = det.fetch_ground_fit(5, min_points=min_points)
            for i, f in enumerate(fits):
                assert bytes(f) == bytes(ssd.ground_fit_solve(f.m, d["priors"][i], min_points)), "the same host code"
            assert all(f.status == (ssd.GF_OK if min_points == 2000 else ssd.GF_FEW) for f in fits)
        assert _moments(det.fetch_ground_fit(5)) == [_want(ssd, d, i, i, False) for i in range(5)]
        assert det.workspace_bytes == base + F * (80 + 128)
    finally:
        buf.free()
        dbuf.free()
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [False, True], ids=["vertices", "depth16"])
def test_host_path_over_three_slices_equals_the_enqueue_path(ssd, gpu_device, depth):
    w, h, n = (250, 190, 70) if depth else (64, 50, 70)                              # 250 x 190 x 2 bytes: no multiple of 16, the padded staging copy
    d = _set(ssd, w, h)
    which = [(3 * k + k // 7) % 5 for k in range(n)]
    frames = np.ascontiguousarray(np.stack([(d["depth"] if depth else d["xyz"])[j] for j in which]))
    priors = []
    for k in range(n):                                                               # seventy priors, all different
        cam = ssd.Camera()
        cam.cal = d["priors"][which[k]]
        cam.cal.b[2] += 1e-4 * k
        if depth:
            cam.intr, cam.has_intrinsics = d["intr"][which[k]], 1
        priors.append(cam)
    cfg = ssd.default_config(w, h, max_frames_per_batch=n)
    det = ssd.Detector(cfg, d["priors"][0], gpu_device)
    buf = _upload(ssd, frames, gpu_device)
    pinned = ssd.PinnedArray(frames.shape, frames.dtype)
    try:
        det.enqueue_ground_fit(buf.ptr, n, TOL, priors=priors, depth=depth)
        want = [bytes(f) for f in det.fetch_ground_fit(n, min_points=300)]
        for k in (0, 31, 32, 69):
            m = ssd.ground_moments_host(cfg, priors[k], frames[k], TOL, depth=depth)
            assert bytes(ssd.ground_fit_solve(m, priors[k], 300)) == want[k], k
        assert len(set(want)) > 60
        pinned.array[...] = frames
        for src in (frames, pinned):
            assert [bytes(f) for f in det.process_host_ground_fit(src, TOL, priors=priors, depth=depth, min_points=300)] == want
        one = [bytes(f) for f in det.process_host_ground_fit(frames, TOL, priors=priors[5], depth=depth, min_points=300)]
        assert one[5] == want[5] and len(one) == n
    finally:
        pinned.free()
        buf.free()
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_detection_batches_in_flight_are_left_alone(ssd, gpu_device, lanes):
    sc = scenes.make(ssd, "vga_3steps_noise2mm")
    others = [ssd.make_scene(sc.width, sc.height, n_steps=3, sigma=0.002, seed=s, pitch_deg=p) for s, p in ((3, 48.0), (4, 52.0), (5, 50.0))]
    scs = [sc] + others
    trans = ssd.transformation_for_scene(sc)
    frames = ssd.synth_host(scs)
    cfg = ssd.default_config(sc.width, sc.height, max_frames_per_batch=4, batches_in_flight=lanes)
    det = ssd.Detector(cfg, trans, gpu_device)
    buf = _upload(ssd, frames, gpu_device)
    try:
        det.enqueue(buf.ptr, 4)
        plain = [bytes(r) for r in det.fetch_list(4)]
        assert det.fetch(4)[0].n_steps == 4
        det.enqueue_ground_fit(buf.ptr, 4, TOL)
        alone = [bytes(f) for f in det.fetch_ground_fit(4)]
        for _ in range(2):
            det.enqueue(buf.ptr, 4)
            det.enqueue_ground_fit(buf.ptr, 4, TOL)
            det.enqueue_ground_fit(buf.ptr, 2, 0.03)
            if lanes > 1:
                det.enqueue(buf.ptr, 3)
            fits2 = [bytes(f) for f in det.fetch_ground_fit(2)]
            det.enqueue_ground_fit(buf.ptr, 4, TOL)
            if lanes > 1:
                assert [bytes(r) for r in det.fetch(3, back=0)] == plain[:3]
                assert [bytes(r) for r in det.fetch(4, back=1)] == plain
            else:
                assert [bytes(r) for r in det.fetch_list(4)] == plain
            assert [bytes(f) for f in det.fetch_ground_fit(4)] == alone and fits2 != alone[:2]
    finally:
        buf.free()
        det.close()


def e2e_scenes(ssd, w, h):
    """five true poses around one rough prior (pitch 50 deg, no roll, 1 m): each off by up to (3 deg, 2 deg, 4 cm)"""
    poses = [dict(pitch_deg=53.0, roll_deg=2.0, cam_height=1.04), dict(pitch_deg=47.0, roll_deg=-2.0, cam_height=0.96),
             dict(pitch_deg=52.0, roll_deg=-1.5, cam_height=0.97), dict(pitch_deg=48.5, roll_deg=1.0, cam_height=1.03),
             dict(pitch_deg=51.0, roll_deg=0.5, cam_height=1.02)]
    scs = [ssd.make_scene(w, h, n_steps=3, sigma=0.002, seed=20 + i, **p) for i, p in enumerate(poses)]
    prior = ssd.transformation_for_scene(ssd.make_scene(w, h, n_steps=3, pitch_deg=50.0, roll_deg=0.0, cam_height=1.0)).constants
    return scs, prior


@pytest.mark.gpu
def test_refined_calibrations_detect_what_the_true_ones_detect(ssd, gpu_device):
    """five frames, five true poses, one rough prior -> refine_calibration -> a camera table -> process_host_cameras: every frame's
    step count and heights as with its true calibration, within BASELINE's 1e-4 m plus the height error the ground fit is recorded
    with (profiles/ground_fit_accuracy.txt); with the rough prior alone at least one frame is farther off than that (on the CPU oracle:
    every frame, by 1 - 6 cm).  At 256 x 192, the shape the accuracy was recorded at: the frames show ground and three steps, and the
    oracle puts the refined heights within 1.4e-4 m of the true ones.  The bar does not cover a surface far up the stairs: a tilt left
    over of 1e-4 rad moves a step 1.5 m away by 1.5e-4 m on its own (at 640 x 480, where a fourth surface is in sight, the oracle has
    it 2.2e-4 m off in one of these frames while the nearer three stay within the bar)."""
    w, h = 256, 192
    scs, prior = e2e_scenes(ssd, w, h)
    frames = ssd.synth_host(scs)
    truth = [ssd.transformation_for_scene(sc).constants for sc in scs]
    bar = 1e-4 + gm.recorded_accuracy()["worst_height_m"]
    cfg = ssd.default_config(w, h, max_frames_per_batch=F)
    det = ssd.Detector(cfg, prior, gpu_device)
    try:
        fits = det.refine_calibration(frames)                                       # prior = None: the handle's calibration
        assert [f.status for f in fits] == [ssd.GF_OK] * 5
        assert [bytes(f) for f in det.refine_calibration(frames, prior=prior)] == [bytes(f) for f in fits]
        for f, sc, t in zip(fits, frames, truth):                                    # the device path is the host path
            assert bytes(f) == bytes(gm.refine_host(ssd, cfg, sc, prior))
            print("angle %.3e rad, height %.3e m" % gm.errors(f, t))
        idx = list(range(5))

        def run(cals):
            det.set_cameras(list(cals))
            return det.process_host_cameras(frames, idx)

        def far(a, b):
            return a.n_steps != b.n_steps or any(abs(a.steps[k].height - b.steps[k].height) > bar for k in range(a.n_steps))

        want, got, rough = run(truth), run([f.cal for f in fits]), run([prior] * 5)
        assert all(r.n_steps == 3 for r in want)
        for i in range(5):
            assert not far(got[i], want[i]), (i, [(got[i].steps[k].height, want[i].steps[k].height) for k in range(want[i].n_steps)])
        assert any(far(rough[i], want[i]) for i in range(5)), "the rough prior alone would have done"
    finally:
        det.close()
