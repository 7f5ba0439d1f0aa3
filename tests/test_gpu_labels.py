"""Per-pixel surface labels on the GPU (k_labels; include/ssd_hip.h): every pixel against the host restatement of test_labels.py, the
invariant (count and fixed-point mean per surface = the debug record) at full batch sizes, and the entry points' contract."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_binding as ob
import scenes
from test_labels import expected_labels, per_surface, same_double
import test_gpu_prefilter_regimes as regimes
from test_gpu_quirks import _bin_edge_cloud, _snap_onto_quad_edges

NAMED = ["xga_config1", "vga_3steps_noise2mm", "xga_8steps_outliers", "fhd_config5", "xga_yaw_m10", "xga_no_stairs", "vga_empty",
         "vga_yaw40_wide_throws", "vga_yaw50_throws", "xga_bin_boundary", "ragged_600x450", "ragged_427x321_yaw",
         "ragged_1100x700_outliers", "xga_2steps_deep", "xga_low_camera"]
POISON = 0xA5


def _expected(ssd, oracle, cfg, cal, xyz):
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), xyz)[0]
    return expected_labels(oracle, cfg, cal, res, xyz), res


def _run_device(ssd, det, cfg, frames, depth=False, unaligned=False, label_pad=0, extra_frames=0, device=0):
    """frames through enqueue_labels / enqueue_depth_labels from device memory -> (results, labels [n, W H], raw label buffer)"""
    n, wh = len(frames), cfg.width * cfg.height
    fb = wh * 2 if depth else wh * 12
    stride = fb + (4 if unaligned else 0)
    off = 4 if unaligned else 0
    buf = ssd.DeviceBuffer(stride * n + off, device)
    lstride = wh + label_pad
    lbuf = ssd.DeviceBuffer(lstride * (n + extra_frames), device)
    try:
        lbuf.upload(np.full(lstride * (n + extra_frames), POISON, dtype=np.uint8))
        for i, f in enumerate(frames):
            buf.upload(np.ascontiguousarray(f, dtype=np.uint16 if depth else np.float32), offset=off + i * stride)
        if depth:
            det.enqueue_depth_labels(buf.ptr, n, lbuf.ptr, label_stride=lstride, stride_bytes=stride)
        else:
            det.enqueue_labels(buf.ptr + off, n, lbuf.ptr, label_stride=lstride, stride_bytes=stride)
        res = det.fetch_list(n)
        raw = lbuf.download(lstride * (n + extra_frames))
    finally:
        buf.free()
        lbuf.free()
    lab = np.stack([raw[i * lstride:i * lstride + wh] for i in range(n)])
    return res, lab, raw


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMED)
def test_labels_of_the_named_scenes_equal_the_checker(ssd, oracle, gpu_device, name):
    """every pixel, vertex input aligned (host entry point) and at a stride of 12 W H + 4 bytes, and 16-bit depth input"""
    sc = scenes.make(ssd, name)
    trans = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(sc.width, sc.height, max_frames_per_batch=2)
    xyz = ssd.synth_host([sc])[0]
    want, ref = _expected(ssd, oracle, cfg, trans.constants, xyz)
    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        res, lab = det.process_host_labels(xyz)
        assert res[0].n_steps == ref.n_steps
        assert np.array_equal(lab[0].reshape(-1), want)
        res2, lab2, _ = _run_device(ssd, det, cfg, [xyz], unaligned=True, device=gpu_device)
        assert np.array_equal(lab2[0], want)
        if sc.width % 4 == 0:
            intr = ssd.intrinsics_for_scene(sc)
            depth = ssd.synth_depth_host([sc])[0]
            det.set_intrinsics(intr)
            dxyz = oracle.deproject(intr, depth)
            dwant, _ = _expected(ssd, oracle, cfg, trans.constants, dxyz)
            _, dlab = det.process_depth_host_labels(depth)
            assert np.array_equal(dlab[0].reshape(-1), dwant)
    finally:
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("inflight", [0, 3])
@pytest.mark.parametrize("nframes", [16, 64])
def test_labels_of_a_batch_equal_the_checker(ssd, oracle, gpu_device, inflight, nframes):
    """XGA batch_scenes: 16 frames (two passes) and 64 (the single pass, vertex input), one workspace and three"""
    W, H = 1024, 768
    scs = scenes.batch_scenes(ssd, W, H, nframes, base_seed=6000, rng_seed=3)
    cfg = ssd.default_config(W, H, max_frames_per_batch=nframes, batches_in_flight=inflight)
    trans = ssd.transformation_for_scene(scs[0])
    xyz = ssd.synth_host(scs)
    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        res, lab, _ = _run_device(ssd, det, cfg, list(xyz), device=gpu_device)
        step = 1 if nframes == 16 else 8
        for i in range(0, nframes, step):
            want, ref = _expected(ssd, oracle, cfg, trans.constants, xyz[i])
            assert res[i].n_steps == ref.n_steps
            assert np.array_equal(lab[i], want), i
    finally:
        det.close()


def _check_bands(ssd, oracle, det, cfg, cal, frame, depth_intr=None):
    if depth_intr is not None:
        det.set_intrinsics(depth_intr)
        _, lab = det.process_depth_host_labels(frame)
        xyz = oracle.deproject(depth_intr, frame)
    else:
        _, lab = det.process_host_labels(frame)
        xyz = frame
    want, _ = _expected(ssd, oracle, cfg, cal, xyz)
    got = lab[0].reshape(-1)
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("yaw_deg", [-9.0, 14.0])
def test_labels_of_points_on_the_quadrilaterals_edges(ssd, oracle, gpu_device, yaw_deg):
    """test_gpu_quirks' band cloud: points of treads and ground moved onto their quadrilaterals' edges (within a micrometre)"""
    W, H = 1024, 768
    sc = ssd.make_scene(W, H, n_steps=3, seed=79, pitch_deg=44.0, roll_deg=1.5, yaw_deg=yaw_deg, sigma=0.001)
    trans = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(W, H, max_frames_per_batch=1)
    a = np.array(list(trans.constants.a), dtype=np.float64).reshape(3, 3)
    b = np.array(list(trans.constants.b), dtype=np.float64)
    xyz = ssd.synth_host([sc])[0].reshape(H, W, 3).copy()
    ref0 = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants), xyz)[0]
    surf = [(list(ref0.plateaus[k].quad_world), ref0.plateaus[k].bin_lo, ref0.plateaus[k].bin_hi)
            for k in range(ref0.n_plateaus) if ref0.plateaus[k].is_step and ref0.plateaus[k].valid]
    g = ref0.plateaus[ref0.ground_ind]
    surf.append((list(ref0.ground_quad_world), g.bin_lo, g.bin_hi))
    made, dist = _snap_onto_quad_edges(cfg, a, b, xyz, surf, np.random.default_rng(11))
    assert (dist < 1e-6).sum() > 400
    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        for mode in (0, 1):
            det.single_pass(mode)
            _check_bands(ssd, oracle, det, cfg, trans.constants, made)
    finally:
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("far_camera", [False, True])
def test_labels_of_points_on_bin_edges(ssd, oracle, gpu_device, far_camera):
    """test_gpu_quirks' bin-edge cloud (world z on every bin edge, plus or minus nothing .. 1e-3 of a bin; an eighth of it on an x / y
    limit too) in a staircase frame, the common regime (no per-point checks): which bin such a point takes decides whether it is
    labelled with the plateau's surface.  Camera near, and 25 m off (single precision ten times as coarse)"""
    W, H = 1024, 768
    sc = ssd.make_scene(W, H, n_steps=2, seed=78, pitch_deg=46.0, roll_deg=-2.5, yaw_deg=-9.0, sigma=0.001)
    trans = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(W, H, max_frames_per_batch=1)
    a = np.array(list(trans.constants.a), dtype=np.float64).reshape(3, 3)
    b = np.array(list(trans.constants.b), dtype=np.float64)
    rng = np.random.default_rng(6)
    xyz = ssd.synth_host([sc])[0].reshape(-1, 3).copy()
    use = trans
    if far_camera:
        shift = np.array([2.0, -1.5, -25.0])              # the same rotation seen from 25 m: world = a (p - shift) + (b + a shift)
        use = ssd.GeometricTransformation()
        C.memmove(C.byref(use.constants), C.byref(trans.constants), C.sizeof(use.constants))
        b = b + a @ shift
        for i in range(3):
            use.constants.b[i] = b[i]
        valid = xyz[:, 2] > 0
        xyz[valid] = (xyz[valid].astype(np.float64) - shift).astype(np.float32)
        xyz[valid & ~(xyz[:, 2] > 0)] = 0.0
    edges = _bin_edge_cloud(cfg, a, b, rng, 400)
    idx = np.sort(rng.permutation(W * H)[:len(edges)])
    xyz[idx] = edges
    xyz = xyz.reshape(H, W, 3)
    det = ssd.Detector(cfg, use, gpu_device)
    try:
        want, ref = _expected(ssd, oracle, cfg, use.constants, xyz)
        assert ref.n_steps >= 2
        on_edge = np.zeros(W * H, dtype=bool)
        on_edge[idx] = True
        assert (want[on_edge] > 0).sum() > 200                # the cloud reaches the labelled surfaces
        for mode in (0, 1):
            det.single_pass(mode)
            _check_bands(ssd, oracle, det, cfg, use.constants, xyz)
    finally:
        det.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", regimes.CASES)
def test_labels_in_the_prefilters_regimes(ssd, oracle, gpu_device, name):
    """test_gpu_prefilter_regimes' cases (checkInput, zCheckTop, all doubles): clouds in the bin bands of each regime"""
    case = regimes.build_case(ssd, oracle, name)
    cfg, trans, frame = case["cfg"], case["trans"], case["frame"]
    det = ssd.Detector(cfg, trans, gpu_device)
    try:
        if case["src"] == "f3":
            _, lab, _ = _run_device(ssd, det, cfg, [frame], unaligned=True, device=gpu_device)
            want, _ = _expected(ssd, oracle, cfg, trans.constants, frame)
            assert np.array_equal(lab[0], want), int((lab[0] != want).sum())
        else:
            _check_bands(ssd, oracle, det, cfg, trans.constants, frame, depth_intr=case["intr"])
    finally:
        det.close()


def _invariant(ssd, records, cfg, cal, xyz, res, lab, frames):
    for i in frames:
        r = res[i]
        d = records[i]
        li = lab[i].reshape(-1)
        if (r.status & ssd.ST_THROW) or r.n_steps == 0:
            assert not li.any(), i
            continue
        assert int(li.max()) <= r.n_steps
        got = per_surface(cal, xyz[i], li, r.n_steps)
        for s, (cnt, mean) in enumerate(got):
            if s == 0 and d.ground_ind >= 0:
                want_n, want_mean = d.ground_n_in_quad, d.ground_mean_z
            else:
                k = [k for k in range(d.first_valid_ind, d.n_plateaus) if d.plateaus[k].valid][s - (1 if d.ground_ind >= 0 else 0)]
                want_n, want_mean = d.plateaus[k].n_in_quad, d.plateaus[k].mean_z
            assert cnt == want_n, (i, s, cnt, want_n)
            assert cnt == 0 or same_double(mean, want_mean), (i, s)
            q6 = s == 0 and d.ground_ind >= 0 and not d.ground_front_valid         # the all-zero ground: its height is world_z
            assert cnt == 0 or same_double(cal.world_z + (0.0 if q6 else mean), r.steps[s].height), (i, s)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["xga1024", "fhd64", "depth1024"])
def test_label_counts_and_means_equal_the_records_at_full_size(ssd, gpu_device, what):
    """BASELINE configs[2] (1024 XGA frames), configs[4] (64 FHD stress frames) and 1024 depth-16 frames, resident in device memory,
    debug records on: no label above n_steps and THROW frames all zero in every frame; per surface the count and the fixed-point mean
    of the labelled points equal the record and the result, in every frame"""
    if what == "fhd64":
        W, H, n = 1920, 1080, 64
        scs = scenes.fhd_stress_scenes(ssd, n)
    else:
        W, H, n = 1024, 768, 1024
        scs = scenes.batch_scenes(ssd, W, H, n)
    wh = W * H
    depth = what == "depth1024"
    cfg = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    trans = ssd.transformation_for_scene(scs[0])
    det = ssd.Detector(cfg, trans, gpu_device)
    fb = wh * (2 if depth else 12)
    buf = ssd.DeviceBuffer(fb * n, gpu_device)
    lbuf = ssd.DeviceBuffer(wh * n, gpu_device)
    try:
        det.set_debug(True, images=False)
        if depth:
            intr = ssd.intrinsics_for_scene(scs[0])
            det.set_intrinsics(intr)
            ssd.synth_depth_device(scs, buf.ptr, device=gpu_device)
            det.enqueue_depth_labels(buf.ptr, n, lbuf.ptr)
        else:
            ssd.synth_device(scs, buf.ptr, device=gpu_device)
            det.enqueue_labels(buf.ptr, n, lbuf.ptr)
        res = det.fetch_list(n)
        lab = lbuf.download(wh * n).reshape(n, wh)
        for i in range(n):
            if (res[i].status & ssd.ST_THROW) or res[i].n_steps == 0:
                assert not lab[i].any(), i
            assert int(lab[i].max()) <= res[i].n_steps, i
        assert sum(r.n_steps for r in res) > n
        records = [det.debug(i) for i in range(n)]

        def check(i):
            xyz = ssd.deproject_host(intr, ssd.synth_depth_host([scs[i]])[0]) if depth else ssd.synth_host([scs[i]])[0]
            _invariant(ssd, records, cfg, trans.constants, {i: xyz}, res, lab, [i])
        with ThreadPoolExecutor(min(len(os.sched_getaffinity(0)), 16)) as pool:
            list(pool.map(check, range(n)))                  # every frame; an assertion in a worker is raised here
    finally:
        buf.free()
        lbuf.free()
        det.close()


@pytest.mark.gpu
def test_the_label_contract(ssd, oracle, gpu_device):
    """padding and frames past nframes untouched; results and debug records as a plain enqueue; three batches in flight each with
    its own labels; host entry points (several slices, pinned and pageable) = the device one; workspace bytes unchanged"""
    W, H, n = 640, 480, 40
    scs = scenes.batch_scenes(ssd, W, H, n, base_seed=7000, rng_seed=5)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    xyz = ssd.synth_host(scs)
    det = ssd.Detector(cfg, trans, gpu_device)
    plain = ssd.Detector(cfg, trans, gpu_device)
    wh = W * H
    try:
        assert det.workspace_bytes == plain.workspace_bytes
        res, lab, raw = _run_device(ssd, det, cfg, list(xyz), label_pad=37, extra_frames=2, device=gpu_device)
        lstride = wh + 37
        for i in range(n):
            assert np.all(raw[i * lstride + wh:(i + 1) * lstride] == POISON)
        assert np.all(raw[n * lstride:] == POISON)
        assert det.workspace_bytes == plain.workspace_bytes
        # results and records as a plain enqueue
        buf = ssd.DeviceBuffer(wh * 12 * n, gpu_device)
        lbuf = ssd.DeviceBuffer(wh * n, gpu_device)
        try:
            buf.upload(np.ascontiguousarray(xyz))
            for d in (det, plain):
                d.set_debug(True, images=False)
            det.enqueue_labels(buf.ptr, n, lbuf.ptr)
            r1 = [bytes(r) for r in det.fetch_list(n)]
            d1 = [bytes(det.debug(i)) for i in range(n)]
            plain.enqueue(buf.ptr, n)
            r0 = [bytes(r) for r in plain.fetch_list(n)]
            d0 = [bytes(plain.debug(i)) for i in range(n)]
            assert r1 == r0 and d1 == d0
            assert np.array_equal(lbuf.download(wh * n).reshape(n, wh), lab)
            for d in (det, plain):
                d.set_debug(False)
            # three batches in flight into three buffers
            bufs = [ssd.DeviceBuffer(wh * 8, gpu_device) for _ in range(3)]
            try:
                parts = [(0, 8), (8, 8), (16, 8)]
                for (at, m), lb in zip(parts, bufs):
                    det.enqueue_labels(buf.ptr + at * wh * 12, m, lb.ptr)
                for back, ((at, m), lb) in zip((2, 1, 0), zip(parts, bufs)):
                    det.fetch(m, back=back)
                    assert np.array_equal(lb.download(wh * m).reshape(m, wh), lab[at:at + m])
            finally:
                for lb in bufs:
                    lb.free()
        finally:
            buf.free()
            lbuf.free()
        # host entry points: several slices, pageable and pinned
        res_h, lab_h = det.process_host_labels(xyz)
        assert np.array_equal(lab_h.reshape(n, wh), lab)
        assert [bytes(r) for r in res_h] == [bytes(r) for r in res]
        ptr = C.c_void_p()
        assert ssd.lib().ssd_host_alloc(xyz.nbytes, C.byref(ptr)) == 0
        try:
            arr = np.ctypeslib.as_array((C.c_float * xyz.size).from_address(ptr.value)).reshape(xyz.shape)
            arr[...] = xyz
            _, lab_p = det.process_host_labels(arr)
            assert np.array_equal(lab_p.reshape(n, wh), lab)
        finally:
            ssd.lib().ssd_host_free(ptr)
        # depth: host = device
        intr = ssd.intrinsics_for_scene(scs[0])
        det.set_intrinsics(intr)
        depth = ssd.synth_depth_host(scs)
        _, dlab_h = det.process_depth_host_labels(depth)
        _, dlab_d, _ = _run_device(ssd, det, cfg, list(depth), depth=True, device=gpu_device)
        assert np.array_equal(dlab_h.reshape(n, wh), dlab_d)
        # timing: the label kernel's time of a labelled enqueue, 0 for a plain one
        det.set_timing(True)
        _run_device(ssd, det, cfg, list(xyz[:4]), device=gpu_device)
        assert det.labels_time_ms(0) > 0.0
        plain_buf = ssd.DeviceBuffer(wh * 12 * 4, gpu_device)
        try:
            plain_buf.upload(np.ascontiguousarray(xyz[:4]))
            det.enqueue(plain_buf.ptr, 4)
            det.fetch(4)
            assert det.labels_time_ms(0) == 0.0
        finally:
            plain_buf.free()
    finally:
        det.close()
        plain.close()
