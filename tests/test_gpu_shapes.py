"""k_outline, k_final and what consumes their quadrilaterals (k_quads, k_inquad, k_labels) on plateaus that are not rectangles:
the catalogue of tests/shapes.py through the HIP path against the oracle.  Every comparison goes through parity.check_frame,
compare_debug and compare_result: integers exact, corners and lines identical doubles, heights to 1e-9 m.  Each case first
shows on the oracle's record that it reaches the branch it was built for (test_shapes.check_signature)."""
import numpy as np
import pytest

import clouds
import oracle_binding as ob
import parity
import shapes
from test_labels import expected_labels
from test_shapes import check_signature, record

pytestmark = pytest.mark.gpu

W, H = 640, 480


@pytest.fixture(scope="module")
def handles():
    """one handle per image size for the single-frame tests, closed when the module is done"""
    dets = {}
    yield dets
    for det in dets.values():
        det.close()


def _handle(ssd, dets, device, w, h):
    if (w, h) not in dets:
        dets[(w, h)] = ssd.Detector(ssd.default_config(w, h, max_frames_per_batch=1), clouds.calibration(ssd), device)
    return dets[(w, h)]


def _check_all(ssd, oracle, dets, device, xyz, w, h):
    """every intermediate and the raw and closed images with debug capture; then the production path without it (there the closing
    runs only inside the bits' bounding box)"""
    det = _handle(ssd, dets, device, w, h)
    cfg, cal = det.cfg, clouds.calibration(ssd).constants
    rep = parity.check_frame(ssd, oracle, det, cfg, cal, xyz, images=True)
    parity.check_results_only(ssd, oracle, cfg, cal, xyz, det.process_host(xyz)[0])
    return rep


@pytest.mark.parametrize("name", shapes.NAMES)
def test_every_case_at_vga(ssd, oracle, gpu_device, handles, name):
    xyz, res, _, _ = record(ssd, oracle, name)
    check_signature(res, shapes.SIGNATURES[name], name)
    rep = _check_all(ssd, oracle, handles, gpu_device, xyz, W, H)
    assert rep["n_steps"] == shapes.SIGNATURES[name]["n_steps"] and rep["images_checked"] == 2


def _corner_pixels(w, h):
    """lone pixels at plateau height in the image's corners and beside them (a lone pixel in a corner survives the closing: the
    erosion ignores neighbours outside the image), and half-way down the two border columns (those the closing removes)"""
    at = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (1, 1), (w - 2, h - 2), (w - 1, h // 2), (0, h // 2)]
    return [shapes.pixel_point(w, h, c, r, shapes.Z_STEP) for c, r in at]


@pytest.mark.parametrize("name", ["full", "left_edge_touch", "right_edge_touch"])
@pytest.mark.parametrize("w", [650, 651])
def test_scan_columns_on_the_images_borders(ssd, oracle, gpu_device, handles, w, name):
    """650 and 651 pixels: a scan column on pixel column 0 (325 - 13 * 25); 651 also one on column W - 1 (325 + 13 * 25), where the
    column-wise closing's 5 x 5 neighbourhood is cut on the right"""
    cfg = ssd.default_config(w, H, max_frames_per_batch=1)
    cal = clouds.calibration(ssd).constants
    xyz = shapes.frame(name, w, H, extra=_corner_pixels(w, H))
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), xyz)[0]
    p = [res.plateaus[k] for k in range(res.n_plateaus) if res.plateaus[k].is_step][0]
    assert res.status == 0 and res.n_steps == 2 and p.outline_found
    last_left, last_right = p.scans_left[p.n_scans_left - 1], p.scans_right[p.n_scans_right - 1]
    # the shapes that touch a border are scanned on it, from the first row to the last where a corner pixel extends the column
    assert (last_left[0] == 0) == (name != "right_edge_touch")
    assert (last_right[0] == w - 1) == (w == 651 and name != "left_edge_touch")
    if last_left[0] == 0:
        assert (last_left[1], last_left[2]) == (0, H - 1)
    if last_right[0] == w - 1:
        assert (last_right[1], last_right[2]) == (0, H - 1)
    _check_all(ssd, oracle, handles, gpu_device, xyz, w, H)


@pytest.mark.parametrize("name", shapes.WIDE)
def test_wide_images(ssd, oracle, gpu_device, handles, name):
    """wider than 1024 pixels: the column scan fetches a row's five pixels with one 8-byte load"""
    xyz, res, _, _ = record(ssd, oracle, name, 1280, 720)
    check_signature(res, shapes.WIDE_SIGNATURES[name], name)
    _check_all(ssd, oracle, handles, gpu_device, xyz, 1280, 720)


def test_both_thread_counts_and_both_passes(ssd, oracle, gpu_device):
    """One handle, max_frames_per_batch = 66: the catalogue cycled to 66 frames with an all-invalid frame first and last.  66 frames
    run k_outline / k_final with 256 threads, 64 frames of the same buffer with 512 (two waves share an edge's BestLine pairs, the
    first of equal residuals wins across the parts); each on two passes and on the single pass.  Every frame of the 66 against the
    oracle, the 64 byte for byte against the 66."""
    n = 66
    names = [None] + [shapes.NAMES[i % len(shapes.NAMES)] for i in range(n - 2)] + [None]
    cfg = ssd.default_config(W, H, max_frames_per_batch=n)
    trans = clouds.calibration(ssd)
    empty = np.zeros((H, W, 3), dtype=np.float32)
    ores = {None: oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants), empty)[0]}
    frames = []
    for name in names:
        if name is None:
            frames.append(empty)
            continue
        xyz, res, _, _ = record(ssd, oracle, name)
        check_signature(res, shapes.SIGNATURES[name], name)
        ores[name] = res
        frames.append(xyz)
    assert ores[None].n_steps == 0 and ores[None].status == 0
    det = ssd.Detector(cfg, trans, gpu_device)
    buf = ssd.DeviceBuffer(W * H * 12 * n, gpu_device)
    try:
        buf.upload(np.ascontiguousarray(np.stack(frames), dtype=np.float32))
        det.set_debug(True, images=False)
        runs = []
        for mode in (0, 1):
            det.single_pass(mode)
            det.enqueue(buf.ptr, n)
            got = det.fetch_list(n)
            assert det.single_pass_stats(n)["ran"] == bool(mode)
            for i, name in enumerate(names):
                try:
                    parity.compare_debug(det.debug(i), ores[name], {})
                    parity.compare_result(ssd, got[i], ores[name], {})
                except parity.Mismatch as e:
                    raise parity.Mismatch("mode %d, frame %d (%s), 256 threads: %s" % (mode, i, name, e))
            runs.append([bytes(r) for r in got])
            det.enqueue(buf.ptr, 64)
            few = [bytes(r) for r in det.fetch_list(64)]
            for i in range(64):
                assert few[i] == runs[-1][i], "mode %d, frame %d (%s): 512 threads give other bytes than 256" % (mode, i, names[i])
        assert runs[0] == runs[1]
    finally:
        buf.free()
        det.close()


# ---- a plateau the single pass reads from two planes
STRIP = shapes.rect(-0.55, 0.55, 1.17, 1.29)              # outside every shape of the catalogue
TWO_PLANE = ["triangle_near", "triangle_far", "lens", "diamond", "trapezoid_near", "parallelogram", "sawtooth_back", "rect45"]
PEAK = 27


def _three_bin_frame(name, seed=0):
    """The shape spread over three height bins so that the predictor cannot tell which neighbour the plateau takes: its left
    three quarters (by points) in the peak bin 27, the right quarter in bin 28, and 300 points fewer than that in bin 26 on a
    strip OUTSIDE the shape (60 / 20 / 20 % of the three bins' points).  The plateau is bins (27, 28): the whole shape, which
    neither plane shows alone.  -> (frame, mask of the peak bin's part)"""
    m = shapes.SHAPES[name]
    pts = shapes.grid_points(W, H, m, shapes.Z_STEP)
    split = float(np.sort(pts[:, 0])[(3 * len(pts)) // 4])
    peak = lambda x, y: m(x, y) & (x < split)
    upper = lambda x, y: m(x, y) & ~(x < split)
    n_upper = int((~(pts[:, 0] < split)).sum())
    strip = shapes.grid_points(W, H, STRIP, shapes.Z_STEP - 0.01)[:n_upper - 300]
    assert len(strip) == n_upper - 300
    xyz = shapes.shape_cloud(W, H, [(shapes.GROUNDS["ground"], shapes.Z_GROUND), (peak, shapes.Z_STEP), (upper, shapes.Z_STEP + 0.01)],
                             seed=seed, extra=strip)
    return xyz, peak


def _two_plane_record(ssd, oracle, name):
    cfg = ssd.default_config(W, H, max_frames_per_batch=8)
    cal = clouds.calibration(ssd).constants
    xyz, peak = _three_bin_frame(name)
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), xyz)[0]
    steps = [res.plateaus[k] for k in range(res.n_plateaus) if res.plateaus[k].is_step]
    assert len(steps) == 1 and res.status == 0
    p = steps[0]
    assert (p.peak_bin, p.bin_lo, p.bin_hi) == (PEAK, PEAK, PEAK + 1), "the plateau's pair"
    h = [int(v) for v in res.hist[PEAK - 1:PEAK + 2]]
    assert 0 < h[2] - h[0] <= 300 and 2 * h[0] > h[2] and 2.9 * h[2] < h[1] < 3.1 * h[2], h
    # the pair's image is not the peak bin's: a scan of the record lies on a column where the peak bin's part has no pixel
    x = shapes.X_MIN + (np.arange(W) + 0.5) * (1.2 / W)
    y = shapes.Y_MAX - (np.arange(H) + 0.5) * (1.2 / H)
    peak_cols = peak(*np.meshgrid(x, y)).any(axis=0)
    scanned = [s[0] for s in p.scans_right[:p.n_scans_right]] + [s[0] for s in p.scans_left[:p.n_scans_left]]
    assert p.outline_found and any(not peak_cols[c] for c in scanned)
    return xyz, res


def test_a_plateau_read_from_two_planes(ssd, oracle, gpu_device):
    """the single pass gives such a plateau three planes; k_outline reads its image as two planes OR-ed on the fly (BitImg::w2)"""
    cfg = ssd.default_config(W, H, max_frames_per_batch=8)
    trans = clouds.calibration(ssd)
    made = [_two_plane_record(ssd, oracle, name) for name in TWO_PLANE]
    det = ssd.Detector(cfg, trans, gpu_device)
    buf = ssd.DeviceBuffer(W * H * 12 * len(made), gpu_device)
    try:
        det.single_pass(1)
        xyz = made[0][0]
        det.process_host(xyz)
        table, planes, covered, step_plateaus = det.single_pass_frame(0)
        assert det.single_pass_stats(1)["ran"] and planes == 3 and covered and step_plateaus == 1
        assert len({int(table[b]) for b in (PEAK - 1, PEAK, PEAK + 1)}) == 3 and 255 not in table[PEAK - 1:PEAK + 2]
        parity.check_frame(ssd, oracle, det, cfg, trans.constants, xyz, images=True)       # still forced: every intermediate, the images
        assert det.single_pass_stats(1)["ran"]
        buf.upload(np.ascontiguousarray(np.stack([m[0] for m in made]), dtype=np.float32))
        det.set_debug(True, images=False)
        det.enqueue(buf.ptr, len(made))
        got = det.fetch_list(len(made))
        st = det.single_pass_stats(len(made))
        assert st["ran"] and st["covered"] == len(made) and st["planes"] == 3 * len(made) and st["dirty_words"] == 0
        for i, (_, res) in enumerate(made):
            try:
                parity.compare_debug(det.debug(i), res, {})
                parity.compare_result(ssd, got[i], res, {})
            except parity.Mismatch as e:
                raise parity.Mismatch("frame %d (%s): %s" % (i, TWO_PLANE[i], e))
        det.single_pass(0)
        det.enqueue(buf.ptr, len(made))
        assert [bytes(r) for r in det.fetch_list(len(made))] == [bytes(r) for r in got]
    finally:
        buf.free()
        det.close()


LABELLED = ["triangle_near", "diamond", "lens", "trapezoid_far", "g_one_column", "g_far_half"]


@pytest.mark.parametrize("name", LABELLED)
def test_labels_of_shaped_surfaces(ssd, oracle, gpu_device, handles, name):
    """corners taken from bounds (triangle, diamond, trapezoid), the lens, and the two grounds without a front edge"""
    xyz, res, _, _ = record(ssd, oracle, name)
    check_signature(res, shapes.SIGNATURES[name], name)
    det = _handle(ssd, handles, gpu_device, W, H)
    cal = clouds.calibration(ssd).constants
    want = expected_labels(oracle, det.cfg, cal, res, xyz)
    assert set(np.unique(want)) == {0, 1, 2}
    got, lab = det.process_host_labels(xyz)
    assert got[0].n_steps == res.n_steps
    assert np.array_equal(lab[0].reshape(-1), want), int((lab[0].reshape(-1) != want).sum())


def test_shapes_from_two_cameras_in_one_batch(ssd, oracle, gpu_device):
    """k_outline_cams / k_final_cams on non-rectangles: two cameras 0.5 m and 0.7 m below the world origin, eight shape frames built
    for their camera in mixed order; each frame's record and result are the oracle's under its own camera"""
    shifts = [0.5, 0.7]
    order = [0, 1, 1, 0, 1, 0, 0, 1]
    names = ["lens", "triangle_far", "rect_left", "diamond", "cols3", "notch_back", "g_far_half", "rect_right"]
    cfg = ssd.default_config(W, H, max_frames_per_batch=len(order))
    cams = [clouds.calibration(ssd, s) for s in shifts]
    frames, ores = [], []
    for name, c in zip(names, order):
        xyz = shapes.frame(name, W, H, z_shift=shifts[c])
        res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cams[c].constants), xyz)[0]
        check_signature(res, shapes.SIGNATURES[name], name)
        frames.append(xyz)
        ores.append(res)
    det = ssd.Detector(cfg, ssd.GeometricTransformation(), gpu_device)          # the handle's own calibration is neither camera's
    buf = ssd.DeviceBuffer(W * H * 12 * len(order), gpu_device)
    try:
        buf.upload(np.ascontiguousarray(np.stack(frames), dtype=np.float32))
        det.set_cameras(cams)
        det.set_debug(True, images=False)
        for mode in (0, 1):
            det.single_pass(mode)
            det.enqueue_cameras(buf.ptr, len(order), order)
            got = det.fetch_list(len(order))
            for i, name in enumerate(names):
                try:
                    parity.compare_debug(det.debug(i), ores[i], {})
                    parity.compare_result(ssd, got[i], ores[i], {})
                except parity.Mismatch as e:
                    raise parity.Mismatch("mode %d, frame %d (%s, camera %d): %s" % (mode, i, name, order[i], e))
    finally:
        buf.free()
        det.close()
