"""GPU parity at the limits ssd_create accepts: the largest frame, the widest, the tallest, frames smaller than one load /
cell / tile, the largest batch, the histogram's first and last bins, the fixed-point mean near 2^63 and one step image.

Hand-built world-space clouds (tests/clouds.py: identity rotation, camera 0.5 m below the world origin).  Each case first
checks on the oracle's record that its scene reaches the branch it was built for, then that the HIP path matches the oracle."""
import math

import numpy as np
import pytest

import clouds
import oracle_binding as ob
import parity

pytestmark = pytest.mark.gpu

E = 1e-4                                              # inside the strict range limits (x +-0.6, y 0.1 / 1.3)
IMAGES_UP_TO = 1300000


def _ocfg_cal(ssd, cfg, z_shift=clouds.Z_SHIFT):
    trans = clouds.calibration(ssd, z_shift)
    return trans, ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants)


def shape_scene(W, H, seed=0):
    """Frames with room for a ground and a step above filterPeaks' 2000 points: a ground in the near third, a step that spans
    the image's full height in its middle, a step that touches all four borders.  Smaller frames: a ground and a step."""
    n = W * H
    if n < 6000:
        return clouds.cloud([(0.005, n // 2, (-0.5, 0.5), (0.15, 0.5)), (0.1755, n - n // 2, (-0.4, 0.4), (0.6, 1.2))], W, H, seed=seed)
    cols = lambda x0, x1: max(1, int((x1 - x0) / 1.2 * W))           # one grid column per pixel column
    return clouds.cloud([(0.005, int(n * 0.35), (-0.6 + E, 0.6 - E), (0.1 + E, 0.5), cols(-0.6, 0.6)),
                         (0.1755, int(n * 0.30), (-0.5, 0.5), (0.1 + E, 1.3 - E), cols(-0.5, 0.5)),
                         (0.3455, int(n * 0.35) - 1, (-0.6 + E, 0.6 - E), (0.1 + E, 1.3 - E), cols(-0.6, 0.6))], W, H, seed=seed)


def full_height_probes(H):
    """probe rows of a vertical edge whose outer bounds lie on the first and the last image row (detectEdge: yStart = front
    y - 10, yEnd = back y + 10, one probe every 10 rows)"""
    return ((H - 1 - 10) - 10) // 10 + 1


def _scan_columns(W):
    """scan columns right (x = W/2, W/2 + 25, ..) and left (W/2 - 25, ..) of the centre"""
    return len(range(W // 2, W, 25)), len(range(W // 2 - 25, -1, -25))


def _expect_largest(ssd, res, W, H):
    assert res.n_steps == 3 and res.ground_ind >= 0 and res.status == 0
    full, borders = res.plateaus[1], res.plateaus[2]
    for p in (full, borders):
        assert p.is_step and p.outline_found and list(p.corner_found) == [1, 1, 1, 1]
        assert list(p.n_vpts) == [full_height_probes(H)] * 2
    # the plateau on all four borders: every scan column finds it, from the first row to the last
    assert (borders.n_scans_right, borders.n_scans_left) == _scan_columns(W)
    rows = [r[1:] for r in borders.scans_right[:borders.n_scans_right]] + [r[1:] for r in borders.scans_left[:borders.n_scans_left]]
    assert min(min(r) for r in rows) == 0 and max(max(r) for r in rows) == H - 1


def _expect_tall(ssd, res, W, H):
    """the step over the full height: every probe row of both vertical edges finds a point (nearly SSD_MAX_EDGE_PTS of them)"""
    assert H == 10 * ssd.MAX_EDGE_PTS and res.status == 0
    assert any(list(res.plateaus[k].n_vpts) == [full_height_probes(H)] * 2 for k in range(res.n_plateaus))
    assert full_height_probes(H) > ssd.MAX_EDGE_PTS - 3


def _expect_no_vertical_edges(ssd, res, W, H):
    """two image rows: the step's outline is found, but the vertical-edge windows are empty (yStart < yEnd), so every
    corner is a horizontal edge's outer bound"""
    steps = [res.plateaus[k] for k in range(res.n_plateaus) if res.plateaus[k].is_step]
    assert steps and res.ground_ind >= 0
    for p in steps:
        assert p.outline_found and list(p.n_vpts) == [0, 0] and list(p.corner_found) == [0, 0, 0, 0]


def _expect_no_outline(ssd, res, W, H):
    """three columns: one scan column, no outline; the left scans would start left of the image, where the reference asserts
    (segmentation.cpp:61)"""
    steps = [res.plateaus[k] for k in range(res.n_plateaus) if res.plateaus[k].is_step]
    assert steps and all(p.outline_found == 0 and (p.n_scans_right, p.n_scans_left) == (1, 0) for p in steps)
    assert res.n_steps == 0 and res.ground_ind >= 0 and res.status == ob.ST_ASSERT


def _expect_no_peaks(ssd, res, W, H):
    """every point in range, none of the histogram's bins reaches filterPeaks' 2000 points"""
    assert res.n_inrange == W * H and res.n_peaks == 0 and res.n_steps == 0


def _expect_smallest_stairs(ssd, res, W, H):
    assert res.n_steps == 2 and res.ground_ind >= 0
    assert all(list(res.plateaus[k].corner_found) == [1, 1, 1, 1] for k in range(res.n_plateaus) if res.plateaus[k].is_step)


SHAPES = [
    ("largest", 3175, 2400, _expect_largest),         # 7.62 M points: 1.1 * W * H just below 2^23, W at SSD_MAX_SCANS
    ("widest_flat", 3175, 2, _expect_no_vertical_edges),
    ("tallest_thin", 3, 2560, _expect_no_outline),    # H at SSD_MAX_EDGE_PTS
    ("tallest", 64, 2560, _expect_tall),              # wide enough for three scan columns: the probe rows at their maximum
    ("1x1", 1, 1, _expect_no_peaks),
    ("3x1", 3, 1, _expect_no_peaks),
    ("5x3", 5, 3, _expect_no_peaks),
    ("63x15", 63, 15, _expect_no_peaks),
    ("64x16", 64, 16, _expect_no_peaks),
    ("65x100", 65, 100, _expect_smallest_stairs),
]


def _single_pass_geometry(W, H):
    return 64 <= W <= 8192 and 16 <= H <= 4096


@pytest.mark.parametrize("name,W,H,expect", SHAPES, ids=[s[0] for s in SHAPES])
def test_extreme_shapes(ssd, oracle, gpu_device, name, W, H, expect):
    """every intermediate (images up to 1.3 M points) or the results; a batch [frame, all-invalid, frame] gives the frame's
    result twice, byte for byte; the single pass forced on and off agree; 16-bit depth input where the handle takes it"""
    cfg = ssd.default_config(W, H, max_frames_per_batch=3)
    trans, ocfg, ocal = _ocfg_cal(ssd, cfg)
    xyz = shape_scene(W, H)
    res = oracle.process(ocfg, ocal, xyz)[0]
    expect(ssd, res, W, H)
    det = ssd.Detector(cfg, trans, gpu_device)
    parity.check_frame(ssd, oracle, det, cfg, trans.constants, xyz, images=W * H <= IMAGES_UP_TO)
    three = np.stack([xyz, np.zeros_like(xyz), xyz])
    got = det.process_host(three)
    assert bytes(got[0]) == bytes(got[2]) and got[1].n_steps == 0 and got[1].status == 0
    parity.check_results_only(ssd, oracle, cfg, trans.constants, xyz, got[0])
    if _single_pass_geometry(W, H):
        det.single_pass(0)
        two_pass = [bytes(r) for r in det.process_host(three)]
        det.single_pass(1)
        assert [bytes(r) for r in det.process_host(three)] == two_pass
        assert det.single_pass_stats(3)["ran"]
        det.single_pass(-1)
    if W % 4 == 0 and W >= 64:
        sc = ssd.make_scene(W, H, n_steps=2, seed=4700 + H, sigma=0.001)
        intr = ssd.intrinsics_for_scene(sc)
        dtrans = ssd.transformation_for_scene(sc)
        ddet = ssd.Detector(cfg, dtrans, gpu_device)
        ddet.set_intrinsics(intr)
        depth = ssd.synth_depth_host([sc])[0]
        dgot = ddet.process_depth_host(np.stack([depth, np.zeros_like(depth), depth]))
        assert bytes(dgot[0]) == bytes(dgot[2])
        parity.check_results_only(ssd, oracle, cfg, dtrans.constants, oracle.deproject(intr, depth), dgot[0])
        ddet.close()
    det.close()


SUB_TILE = [(3, 1), (7, 5), (31, 29)]                 # 3 (< one 4-point load), 35 (< one cell), 899 (< one tile) points


def _sub_tile_frames(W, H, n_frames, rng):
    """all-invalid, full, partly valid (some points out of range), in turn; heights spread over the whole histogram"""
    n = W * H
    frames = np.zeros((n_frames, n, 3), dtype=np.float32)
    for i in range(n_frames):
        kind = i % 3
        if kind == 0:
            continue
        p = np.stack([rng.uniform(-0.59, 0.59, n), rng.uniform(0.11, 1.29, n), rng.uniform(-0.099, 1.099, n) + clouds.Z_SHIFT], 1)
        if kind == 2:
            p[rng.random(n) < 0.4] = 0.0
            p[rng.random(n) < 0.2, 2] = 2.0 + clouds.Z_SHIFT             # above z_max
        frames[i] = p
    return frames.reshape(n_frames, H, W, 3)


@pytest.mark.parametrize("W,H", SUB_TILE, ids=["%dx%d" % s for s in SUB_TILE])
def test_sub_tile_frames_in_one_batch(ssd, oracle, gpu_device, W, H):
    """frames packed at 12 bytes per point, n not a multiple of 4: frame boundaries fall inside a 16-byte load and inside a
    tile; a ragged last tile must not count the next frame's points"""
    n_frames = 24
    cfg = ssd.default_config(W, H, max_frames_per_batch=n_frames)
    trans, ocfg, ocal = _ocfg_cal(ssd, cfg)
    frames = _sub_tile_frames(W, H, n_frames, np.random.default_rng(W * 1000 + H))
    det = ssd.Detector(cfg, trans, gpu_device)
    det.set_debug(True, images=False)
    got = det.process_host(frames)
    for i in range(n_frames):
        res = oracle.process(ocfg, ocal, frames[i])[0]
        assert res.n_nonzero == int(np.count_nonzero(np.any(frames[i] != 0, axis=2)))
        dbg = det.debug(i)
        assert (dbg.n_nonzero, dbg.n_inrange) == (res.n_nonzero, res.n_inrange), i
        assert list(dbg.hist[:res.n_bins]) == list(res.hist[:res.n_bins]), i
        parity.check_results_only(ssd, oracle, cfg, trans.constants, frames[i], got[i])
    det.set_debug(False)
    det.close()


def test_largest_batch(ssd, oracle, gpu_device):
    """max_frames_per_batch = 65535 frames of the smallest frame that still holds stairs (65 x 100), each with its own
    heights: every frame's result is the oracle's for that frame"""
    W, H, n = 65, 100, 65535
    cfg = ssd.default_config(W, H, max_frames_per_batch=n, max_step_plateaus=2)
    trans, ocfg, ocal = _ocfg_cal(ssd, cfg)
    npts = W * H
    templates = []
    for k in range(29):                               # the two steps' heights move with the template; one frame in 29 is empty
        if k == 28:
            templates.append(np.zeros((npts, 3), dtype=np.float32))
            continue
        z1, z2 = 0.1255 + 0.01 * k, 0.4355 + 0.02 * k
        templates.append(clouds.cloud([(0.005, int(npts * 0.35), (-0.6 + E, 0.6 - E), (0.1 + E, 0.5)),
                                       (z1, int(npts * 0.30), (-0.15, 0.15), (0.1 + E, 1.3 - E)),
                                       (z2, int(npts * 0.35) - 1, (-0.6 + E, 0.6 - E), (0.1 + E, 1.3 - E))], W, H, seed=k).reshape(npts, 3))
    templates = np.stack(templates)
    lean = [oracle.process_lean(ocfg, ocal, t) for t in templates]
    assert sum(1 for l in lean if l[0] == 2) == 28
    which = (np.arange(n) * 7) % len(templates)
    buf = ssd.DeviceBuffer(npts * 12 * n, gpu_device)
    chunk = 4096
    for at in range(0, n, chunk):
        buf.upload(templates[which[at:at + chunk]], offset=npts * 12 * at)
    det = ssd.Detector(cfg, trans, gpu_device)
    det.enqueue(buf.ptr, n)
    got = det.fetch(n)
    for i in range(n):
        try:
            parity.compare_results_only(ssd, oracle, got[i], lean[which[i]])
        except parity.Mismatch as e:
            raise parity.Mismatch("frame %d: %s" % (i, e))
    det.close()
    buf.free()


def _bins_config(ssd, W, H, bins, z_min, z_max):
    """height_interval for `bins` bins over [z_min, z_max], the quotient half-way between two integers"""
    cfg = ssd.default_config(W, H, max_frames_per_batch=1)
    cfg.z_min, cfg.z_max = z_min, z_max
    cfg.height_interval = (z_max - z_min) / (bins - 0.5)
    assert int((z_max - z_min) * (1 / cfg.height_interval)) + 1 == bins
    return cfg


def test_histogram_128_bins_first_and_last(ssd, oracle, gpu_device):
    """exactly SSD_MAX_BINS bins; plateaus in bin 0 (the ground) and bin 127, points just below z_max (in bin 127) and
    exactly at z_max (outside)"""
    W, H = 640, 480
    cfg = _bins_config(ssd, W, H, ssd.MAX_BINS, -0.1, 1.1)
    trans, ocfg, ocal = _ocfg_cal(ssd, cfg)
    hi = cfg.height_interval
    z0, z127 = cfg.z_min + 0.5 * hi, cfg.z_min + 127.25 * hi
    xyz = clouds.cloud([(z0, 60000, (-0.55, 0.55), (0.15, 0.45)), (0.5, 30000, (-0.4, 0.4), (0.5, 0.75)),
                        (z127, 30000, (-0.4, 0.4), (0.8, 1.05))], W, H,
                       extra=[[0.0, 0.7, cfg.z_max - 1e-6]] * 300 + [[0.0, 0.7, cfg.z_max]] * 300)
    res = oracle.process(ocfg, ocal, xyz)[0]
    # findPeaks looks at interior bins only: bins 0 and 127 count points but hold no peak; the points at z_max are outside
    assert res.n_bins == ssd.MAX_BINS and res.hist[0] == 60000 and res.hist[ssd.MAX_BINS - 1] == 30000 + 300
    assert res.n_inrange == 60000 + 30000 + 30000 + 300 and list(res.peaks[:res.n_peaks]) == [63] and res.n_steps == 1
    det = ssd.Detector(cfg, trans, gpu_device)
    parity.check_frame(ssd, oracle, det, cfg, trans.constants, xyz, images=True)
    det.close()


def test_histogram_3_bins(ssd, oracle, gpu_device):
    """the fewest bins make_params accepts: every plateau pair runs into the histogram's ends"""
    W, H = 640, 480
    cfg = _bins_config(ssd, W, H, 3, -0.1, 1.1)
    cfg.min_height_above_ground = 0.3
    trans, ocfg, ocal = _ocfg_cal(ssd, cfg)
    hi = cfg.height_interval
    xyz = clouds.cloud([(cfg.z_min + 0.5 * hi, 80000, (-0.55, 0.55), (0.15, 0.45)), (cfg.z_min + 1.5 * hi, 30000, (-0.4, 0.4), (0.5, 0.75)),
                        (cfg.z_min + 2.25 * hi, 40000, (-0.4, 0.4), (0.8, 1.05))], W, H)
    res = oracle.process(ocfg, ocal, xyz)[0]
    assert res.n_bins == 3 and list(res.hist[:3]) == [80000, 30000, 40000] and list(res.peaks[:res.n_peaks]) in ([], [1])
    det = ssd.Detector(cfg, trans, gpu_device)
    parity.check_frame(ssd, oracle, det, cfg, trans.constants, xyz, images=True)
    det.close()


def _fsum_mean(pts_f32, quad, z_shift, oracle):
    """mean world z of the points inside a world quadrilateral: the float32 inputs, transformed in float64, summed exactly"""
    p = pts_f32.astype(np.float64)
    rc, inside = oracle.quad_test(quad, p[:, :2])
    assert rc >= 0
    z = p[inside.astype(bool), 2] - z_shift
    return math.fsum(z.tolist()) / len(z), len(z)


@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
def test_fixed_point_mean_at_its_limit(ssd, oracle, gpu_device, sign):
    """max|z| * W * H just below 2^23 (XGA, |z| up to 10.66 m, 8.5 cm bins): one plateau holds most of the frame, so the sum of
    round(z * 2^40) over its in-quadrilateral points is near +-2^63.  Heights against the oracle and against an exact mean."""
    W, H = 1024, 768
    z_abs = math.floor(2 ** 23 / (W * H) * 1000) / 1000
    cfg = ssd.default_config(W, H, max_frames_per_batch=1)
    cfg.height_interval = 0.085
    cfg.min_height_above_ground = 0.5 if sign > 0 else -10.0      # minHeight: bin 7 of 127 either way
    if sign > 0:
        cfg.z_min, cfg.z_max = -0.1, z_abs
        shift = 0.5
        ground, big = 0.0, 10.52               # the big plateau: a step near z_max
    else:
        cfg.z_min, cfg.z_max = -z_abs, 0.1
        shift = 11.0
        ground, big = -10.52, -1.0             # the big plateau: the ground near z_min, the step above it
    trans, ocfg, ocal = _ocfg_cal(ssd, cfg, shift)
    n = W * H
    if sign > 0:
        planes = [(ground, int(n * 0.1), (-0.55, 0.55), (0.15, 0.3)), (big, n - int(n * 0.1) - 1, (-0.58, 0.58), (0.35, 1.28))]
    else:
        planes = [(ground, n - int(n * 0.1) - 1, (-0.58, 0.58), (0.12, 0.9)), (big, int(n * 0.1), (-0.4, 0.4), (0.95, 1.25))]
    xyz = clouds.cloud(planes, W, H, z_shift=shift)
    res = oracle.process(ocfg, ocal, xyz)[0]
    assert res.n_steps >= 1 and res.ground_ind >= 0 and res.first_valid_ind >= 0
    pts = xyz.reshape(-1, 3)
    pts = pts[np.any(pts != 0, axis=1)]
    if sign > 0:
        k = [i for i in range(res.n_plateaus) if res.plateaus[i].is_step][-1]
        pl = res.plateaus[k]
        mine = pts[np.abs(pts[:, 2] - np.float32(big + shift)) < 1e-3]
        exact, cnt = _fsum_mean(mine, list(pl.quad_world), shift, oracle)
        assert cnt == pl.n_in_quad and cnt * abs(big) * 2 ** 40 > 2 ** 62
        assert abs(pl.mean_z - exact) <= parity.TOL_HEIGHT
    else:
        mine = pts[np.abs(pts[:, 2] - np.float32(ground + shift)) < 1e-3]
        exact, cnt = _fsum_mean(mine, list(res.ground_quad_world), shift, oracle)
        assert cnt == res.ground_n_in_quad and cnt * abs(ground) * 2 ** 40 > 2 ** 62
        assert abs(res.ground_mean_z - exact) <= parity.TOL_HEIGHT
    det = ssd.Detector(cfg, trans, gpu_device)
    parity.check_frame(ssd, oracle, det, cfg, trans.constants, xyz, images=True)
    det.set_debug(True, images=False)
    det.process_host(xyz)
    dbg = det.debug(0)
    if sign > 0:
        assert abs(dbg.plateaus[k].mean_z - exact) <= parity.TOL_HEIGHT
    else:
        assert abs(dbg.ground_mean_z - exact) <= parity.TOL_HEIGHT
    det.close()


def test_one_step_image(ssd, oracle, gpu_device):
    """max_step_plateaus = 1 on a one-step scene"""
    W, H = 640, 480
    cfg = ssd.default_config(W, H, max_frames_per_batch=1, max_step_plateaus=1)
    trans, ocfg, ocal = _ocfg_cal(ssd, cfg)
    xyz = clouds.cloud([(0.005, 60000, (-0.55, 0.55), (0.15, 0.45)), (0.1755, 30000, (-0.4, 0.4), (0.5, 0.75))], W, H)
    res = oracle.process(ocfg, ocal, xyz)[0]
    assert res.n_steps == 2 and res.status == 0
    det = ssd.Detector(cfg, trans, gpu_device)
    rep = parity.check_frame(ssd, oracle, det, cfg, trans.constants, xyz, images=True)
    assert rep["n_steps"] == 2
    det.close()
