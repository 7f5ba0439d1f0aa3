"""Per-pixel surface labels (include/ssd_hip.h, ssd_enqueue_labels & co.): the host restatement of what a label is, and the CPU tier.

expected_labels() owes nothing to the GPU: from the oracle's record of a frame (plateaus, their bin pairs, ground_ind /
first_valid_ind, quadrilaterals) it derives the bins that feed each plateau (pointcloud.cpp:280-343), transforms the vertices in
numpy doubles in the reference's order, applies the strict range test and the bin, and asks the oracle's QuadrilateralTest about
the candidates.  Label k + 1 = the point counts toward surface k of the result (ground first when emitted, then the valid steps
ascending), 0 = none.  The CPU tests below check it against the oracle's own counts and fixed-point means; the GPU tests
(test_gpu_labels.py) compare the kernel's labels with it pixel for pixel.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import scenes

ZFIX = float(1 << 40)


def world(cal, p32):
    """CameraToWorld in the reference's doubles and order: (a0 x + a1 y) + a2 z, then + b"""
    a = np.array(list(cal.a), dtype=np.float64).reshape(3, 3)
    b = np.array(list(cal.b), dtype=np.float64)
    x, y, z = (p32[:, k].astype(np.float64) for k in range(3))
    wx = ((a[0, 0] * x + a[0, 1] * y) + a[0, 2] * z) + b[0]
    wy = ((a[1, 0] * x + a[1, 1] * y) + a[1, 2] * z) + b[1]
    wz = ((a[2, 0] * x + a[2, 1] * y) + a[2, 2] * z) + b[2]
    return wx, wy, wz


def effective_bins(res):
    """[(lo, hi)] per plateau: the bins that feed it.  extractPlateauPoints keeps, of the points not yet taken (those above every
    earlier plateau's upper bin: the ones below an earlier pair's lower bin went to the remainder), the ones in [bin_lo, bin_hi]."""
    out, taken = [], -(1 << 30)
    for k in range(res.n_plateaus):
        pl = res.plateaus[k]
        lo, hi = max(pl.bin_lo, taken + 1, 0), min(pl.bin_hi, res.n_bins - 1)
        out.append((lo, hi))
        taken = max(taken, pl.bin_hi)
    return out


def surfaces(res):
    """the emitted surfaces in result order: [(plateau index, quadrilateral in camera-dependent world x / y, is_ground)]"""
    if (res.status & ob.ST_THROW) or res.n_steps == 0 or res.first_valid_ind < 0:
        return []
    out = []
    if res.ground_ind >= 0:
        out.append((res.ground_ind, list(res.ground_quad_world), True))
    for k in range(res.first_valid_ind, res.n_plateaus):
        pl = res.plateaus[k]
        if pl.valid:
            out.append((k, list(pl.quad_world), False))
    return out[:ob.MAX_STEPS]


def expected_labels(oracle, cfg, cal, res, xyz):
    """uint8 [W H]: label of every point of the frame (xyz: float32 camera vertices) given the oracle's record `res` of it"""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    labels = np.zeros(len(p), dtype=np.uint8)
    surf = surfaces(res)
    if not surf:
        return labels
    wx, wy, wz = world(cal, p)
    ok = (p[:, 2] > 0) & (wx > cfg.x_min) & (wx < cfg.x_max) & (wy > cfg.y_min) & (wy < cfg.y_max) & (wz > cfg.z_min) & (wz < cfg.z_max)
    with np.errstate(invalid="ignore"):
        hbin = np.where(ok, (wz - cfg.z_min) * (1.0 / cfg.height_interval), -1.0).astype(np.int64)
    eff = effective_bins(res)
    for place, (k, quad, _) in enumerate(surf):
        lo, hi = eff[k]
        cand = np.flatnonzero(ok & (hbin >= lo) & (hbin <= hi))
        if len(cand) == 0:
            continue
        rc, inside = oracle.quad_test(quad, np.stack([wx[cand], wy[cand]], 1))
        assert rc == 0
        labels[cand[inside.astype(bool)]] = place + 1
    return labels


def fixed_mean(wz):
    """mean_of_fixed (ssd_kernels.hip): sum of round(z 2^40) in int64, over 2^40, over n; the empty case is x86's -nan"""
    if len(wz) == 0:
        return float("nan")
    s = int(np.rint(wz * ZFIX).astype(np.int64).sum(dtype=np.int64))
    return (float(s) / ZFIX) / len(wz)


def plain_mean(wz):
    """calcAverageZ (pointcloud.cpp:574-581) as the reference runs it: a running double sum in point order, over n"""
    return float(np.add.accumulate(wz)[-1]) / len(wz) if len(wz) else float("nan")


def per_surface(cal, xyz, labels, n, mean=fixed_mean):
    """[(count, mean of world z)] of labels 1 .. n (the GPU's fixed-point mean, or the reference's plain one)"""
    p = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    lab = np.asarray(labels).reshape(-1)
    sel = np.flatnonzero(lab)
    wz = world(cal, p[sel])[2] if len(sel) else np.zeros(0)
    ls = lab[sel]
    return [(int((ls == i + 1).sum()), mean(wz[ls == i + 1])) for i in range(n)]


def same_double(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes() or (a != a and b != b)


def check_against_record(oracle, cfg, cal, res, xyz, labels):
    """labels against the oracle's record: per surface the count is n_in_quad and the mean of its points' world z, summed in point
    order as the reference does, its mean_z, bit for bit"""
    surf = surfaces(res)
    lab = np.asarray(labels).reshape(-1)
    assert int(lab.max(initial=0)) <= len(surf)
    for (k, _, ground), (cnt, mean) in zip(surf, per_surface(cal, xyz, lab, len(surf), plain_mean)):
        want_n = res.ground_n_in_quad if ground else res.plateaus[k].n_in_quad
        want_mean = res.ground_mean_z if ground else res.plateaus[k].mean_z
        assert cnt == want_n, (k, ground, cnt, want_n)
        assert cnt == 0 or same_double(mean, want_mean), (k, ground, mean, want_mean)


NAMED = ["xga_config1", "vga_3steps_noise2mm", "xga_8steps_outliers", "xga_yaw_m10", "xga_no_stairs", "vga_empty",
         "vga_yaw50_throws", "xga_bin_boundary", "ragged_427x321_yaw", "xga_2steps_deep"]


@pytest.mark.parametrize("name", NAMED)
def test_the_checker_reproduces_the_oracles_counts_and_means(ssd, oracle, name):
    """The checker's labels, per surface: the count is the oracle's n_in_quad / ground_n_in_quad and the mean of the labelled points'
    z its mean_z / ground_mean_z, bit for bit (what validates the checker itself before the GPU tests compare with it)."""
    sc = scenes.make(ssd, name)
    trans = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(sc.width, sc.height, max_frames_per_batch=1)
    xyz = ssd.synth_host([sc])[0]
    ocfg, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants)
    res = oracle.process(ocfg, ocal, xyz)[0]
    labels = expected_labels(oracle, cfg, trans.constants, res, xyz)
    check_against_record(oracle, cfg, trans.constants, res, xyz, labels)
    if (res.status & ob.ST_THROW) or res.n_steps == 0:
        assert not labels.any()
    else:
        assert int(labels.max()) == len(surfaces(res)) == res.n_steps


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_checker_on_random_staircases_at_xga(ssd, oracle, seed):
    sc = scenes.batch_scenes(ssd, 1024, 768, 1, base_seed=4000 + seed, rng_seed=seed)[0]
    trans = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(1024, 768, max_frames_per_batch=1)
    xyz = ssd.synth_host([sc])[0]
    ocfg, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants)
    res = oracle.process(ocfg, ocal, xyz)[0]
    labels = expected_labels(oracle, cfg, trans.constants, res, xyz)
    check_against_record(oracle, cfg, trans.constants, res, xyz, labels)
    assert res.n_steps >= 2 and int(labels.max()) == res.n_steps


LABEL_NAMES = ["ssd_enqueue_labels", "ssd_enqueue_depth_labels", "ssd_process_host_labels", "ssd_process_depth_host_labels",
               "ssd_get_labels_time_back"]


def test_the_label_entry_points_are_exported_and_wrapped(ssd):
    for n in LABEL_NAMES:
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("enqueue_labels", "enqueue_depth_labels", "process_host_labels", "process_depth_host_labels", "labels_time_ms"):
        assert callable(getattr(ssd.Detector, m))


def test_the_label_entry_points_reject_bad_arguments(ssd):
    """null handle, null destination, a stride below W H: SSD_E_ARG with a message (no GPU needed: the checks come first)"""
    L = ssd.lib()
    vp = C.c_void_p
    dummy = vp(16)
    assert L.ssd_enqueue_labels(None, dummy, 12 * 640 * 480, 1, None, dummy, 640 * 480) == -1
    assert b"null" in L.ssd_last_error()
    assert L.ssd_enqueue_depth_labels(None, dummy, 2 * 640 * 480, 1, None, dummy, 640 * 480) == -1
    res = (ssd.FrameResult * 1)()
    assert L.ssd_process_host_labels(None, dummy, 1, res, dummy) == -1
    assert L.ssd_process_depth_host_labels(None, dummy, 1, res, dummy) == -1
    ms = C.c_float(0.0)
    assert L.ssd_get_labels_time_back(None, 0, C.byref(ms)) == -1


@pytest.mark.gpu
def test_the_label_entry_points_reject_a_null_destination_and_a_short_stride(ssd, gpu_device):
    sc = scenes.make(ssd, "vga_3steps_noise2mm")
    cfg = ssd.default_config(sc.width, sc.height, max_frames_per_batch=2)
    det = ssd.Detector(cfg, ssd.transformation_for_scene(sc), gpu_device)
    L = ssd.lib()
    dummy = C.c_void_p(4096)
    wh = cfg.width * cfg.height
    try:
        assert L.ssd_enqueue_labels(det._h, dummy, 12 * wh, 1, None, None, wh) == -1
        assert b"null" in L.ssd_last_error()
        assert L.ssd_enqueue_labels(det._h, dummy, 12 * wh, 1, None, dummy, wh - 1) == -1
        assert b"stride" in L.ssd_last_error()
        assert L.ssd_enqueue_depth_labels(det._h, dummy, 2 * wh, 1, None, dummy, wh - 1) == -1
        res = (ssd.FrameResult * 1)()
        assert L.ssd_process_host_labels(det._h, dummy, 1, res, None) == -1
    finally:
        det.close()
