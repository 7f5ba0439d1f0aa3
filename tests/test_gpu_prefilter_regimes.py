"""K1 (k_hist, k_hist_planes) and k_inquad in the pre-filter's rarer regimes (csrc/ssd_prexy.h), against the oracle on clouds made for
each regime's own band.

make_pre_xy / make_pre_z / make_pre_pixel put a handle in one of three regimes.  The common one (check_input == 0, z_check_top == 0)
is what tests/test_gpu_quirks.py's band tests run in.  Here:
  A  z_check_top == 1: the z range is not a whole number of bins, and points within the bound of its top go to the doubles
     (the CHECKS instantiations; SSD_SABOTAGE_PRE & 8 drops that band);
  B  check_input == 1 with in-range inputs beyond PreXY::max_input (64): a calibration in millimetres, a camera 3 km off
     (the per-point magnitude test mFar; SSD_SABOTAGE_PRE & 16 drops it);
  C  all doubles: a calibration single precision cannot serve in x / y (lo < 0, hi = inf, max_input < 0), and one that cannot
     serve z either (z_h0 < 0).

Each case is built on the host - pytest's CPU tier checks, without a GPU, that it is in its regime and that its cloud reaches its
band: prefilter_model (the kernel's decisions restated in numpy) must reproduce the oracle's histogram with every band in place, and
get at least a few dozen points and the oracle's histogram wrong with the case's band removed.  The GPU tests then compare the HIP
path with the oracle bit for bit (parity.check_frame, with images), two passes and the single pass forced, on the three sources of
load_cell (16-byte aligned vertices, vertices at a stride of 12 W H + 4 bytes, 16-bit depth) and both walks of k_hist_planes
(W = 1024: the tile loop; W = 640: the strips).  profiles/prefilter_regimes_sabotage.txt: each GPU case fails on a build that
drops its band."""
import numpy as np
import pytest

import oracle_binding as ob
import parity
import prefilter_model as pm

# offsets from an edge in bins (pixels, ranges): nothing, a few double ulps, 1e-12 .. 1e-3
DELTAS = np.concatenate([[0.0], *[[d, -d] for d in (1e-14, 1e-12, 1e-10, 1e-8, 1e-7, 3e-7, 1e-6, 3e-6, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3)]])

CASES = ["A-near-aligned-640", "A-near-f3-1024", "A-near-depth-640", "A-far25-aligned-1024", "A-far25-f3-640",
         "B-mm-aligned-1024", "B-mm-f3-640", "B-mm-depth-640", "B-km-aligned-640", "B-km-f3-1024",
         "C-xy-aligned-640", "C-all-aligned-1024"]


def _lim(cfg):
    return (cfg.x_min, cfg.x_max, cfg.y_min, cfg.y_max, cfg.z_min, cfg.z_max)


def _transformation(ssd, base, a, b):
    """base's constants with the rows a and the offset b (ssd_create takes any)"""
    t = ssd.GeometricTransformation()
    for i in range(9):
        t.constants.a[i] = float(a.reshape(9)[i])
    for i in range(3):
        t.constants.b[i] = float(b[i])
    for name in ("r2", "t2"):
        for i in range(len(getattr(base.constants, name))):
            getattr(t.constants, name)[i] = getattr(base.constants, name)[i]
    t.constants.world_z = base.constants.world_z
    return t


def _camera(w, a, b):
    return ((w - b) @ np.linalg.inv(a).T).astype(np.float32)


def _in_range_xy(cfg, rng, n, margin=0.01):
    return rng.uniform(cfg.x_min + margin, cfg.x_max - margin, n), rng.uniform(cfg.y_min + margin, cfg.y_max - margin, n)


def _top_points(cfg, a, b, rng, n):
    """world z on the top of the z range (mostly just below it: the band's mistakes then all read "outside") and x / y in range"""
    x, y = _in_range_xy(cfg, rng, n)
    d = np.abs(rng.choice(DELTAS, n)) * np.where(rng.uniform(size=n) < 0.8, -1.0, 1.0)
    return _camera(np.stack([x, y, cfg.z_max + d * cfg.height_interval], 1), a, b)


def _bin_edge_points(cfg, a, b, rng, n_per):
    n_bins = int((cfg.z_max - cfg.z_min) / cfg.height_interval) + 1
    pts = []
    for edge in range(n_bins):
        x, y = _in_range_xy(cfg, rng, n_per)
        pts.append(_camera(np.stack([x, y, cfg.z_min + (edge + rng.choice(DELTAS, n_per)) * cfg.height_interval], 1), a, b))
    return np.concatenate(pts)


def _limit_points(cfg, a, b, rng, n_per):
    """world x or y on a limit of the measuring range, DELTAS of the range's extent off it"""
    pts = []
    for lim, axis in ((cfg.x_min, 0), (cfg.x_max, 0), (cfg.y_min, 1), (cfg.y_max, 1)):
        x, y = _in_range_xy(cfg, rng, n_per, 0.05)
        w = np.stack([x, y, rng.choice([0.0034, 0.1712, 0.3391], n_per) + rng.normal(0.0, 0.0007, n_per)], 1)
        ext = (cfg.x_max - cfg.x_min) if axis == 0 else (cfg.y_max - cfg.y_min)
        w[:, axis] = lim + rng.choice(DELTAS, n_per) * ext
        pts.append(_camera(w, a, b))
    return np.concatenate(pts)


def _pixel_edge_points(cfg, a, b, rng, heights, n_per, width, height):
    """at the treads' heights beside the staircase (|x| > 0.45 m), x or y on a pixel edge (the image's borders among them)"""
    x_to_img, y_to_img = width / (cfg.x_max - cfg.x_min), height / (cfg.y_max - cfg.y_min)
    pts = []
    for z in heights:
        for axis in (0, 1):
            w = np.stack([rng.choice([-1.0, 1.0], n_per) * rng.uniform(0.46, 0.59, n_per), rng.uniform(cfg.y_min + 0.02, cfg.y_max - 0.02, n_per),
                          z + rng.normal(0.0, 0.0004, n_per)], 1)
            d = rng.choice(DELTAS, n_per) * 5.0
            if axis == 0:
                col = np.floor((w[:, 0] - cfg.x_min) * x_to_img)
                col[: n_per // 10] = rng.choice([0.0, float(width)], n_per // 10)
                w[:, 0] = cfg.x_min + (col + d) / x_to_img
            else:
                row = np.floor((cfg.y_max - w[:, 1]) * y_to_img)
                row[: n_per // 10] = rng.choice([0.0, float(height)], n_per // 10)
                w[:, 1] = cfg.y_max - (row + d) / y_to_img
            pts.append(_camera(w, a, b))
    return np.concatenate(pts)


def _place(xyz, extra, rng):
    flat = xyz.reshape(-1, 3).copy()
    assert len(extra) < len(flat) // 3
    flat[np.sort(rng.permutation(len(flat))[:len(extra)])] = extra
    return flat.reshape(xyz.shape)


def _depth_on_level(depth, intr, a, b, z_target, rng, frac):
    """16-bit depth cannot put a point on an edge: for a share `frac` of the pixels, the raw value whose world z lies nearest
    z_target (world z is linear in raw along the pixel's ray)"""
    H, W = depth.shape
    v, u = np.mgrid[0:H, 0:W]
    rx = (u.astype(np.float32) - np.float32(intr.ppx)) / np.float32(intr.fx)
    ry = (v.astype(np.float32) - np.float32(intr.ppy)) / np.float32(intr.fy)
    slope = intr.depth_units * (a[2, 0] * rx + a[2, 1] * ry + a[2, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        raw = np.rint((z_target - b[2]) / slope)
    pick = (rng.uniform(size=depth.shape) < frac) & (raw >= 1) & (raw <= 65535)
    out = depth.copy()
    out[pick] = raw[pick].astype(np.uint16)
    return out, int(pick.sum())


def build_case(ssd, oracle, name):
    """-> dict(cfg, trans, frame (float vertices or uint16 depth), intr (depth only), src, res (the oracle's record), count (points the
    kernel would get wrong without the case's band), W, H); asserts the regime and that the cloud reaches the band"""
    kind, where, src, W = name.split("-")
    W = int(W)
    H = W * 3 // 4
    seed = sum(ord(ch) for ch in name)
    rng = np.random.default_rng(seed)
    roll = -25.0 if where == "km" else -2.5                             # km: the camera's x axis takes a share of the large inputs
    sc = ssd.make_scene(W, H, n_steps=2, seed=seed, pitch_deg=46.0, roll_deg=roll, yaw_deg=-9.0, sigma=0.001)
    base = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(W, H, max_frames_per_batch=1)
    a0 = np.array(list(base.constants.a), dtype=np.float64).reshape(3, 3)
    b0 = np.array(list(base.constants.b), dtype=np.float64)
    xyz = ssd.synth_host([sc])[0]
    intr, depth = None, None
    if src == "depth":
        units = 0.0001                                               # a finer depth unit than the default puts more pixels into a band
        intr = ssd.intrinsics_for_scene(sc, depth_units=units)
        depth = ssd.synth_depth_host([sc], depth_units=units)[0]
    a, b = a0, b0
    if kind == "A":
        cfg.z_max = cfg.z_min + 100.5 * cfg.height_interval              # the top in the middle of bin 100
        drop = ("top",)
        if where == "far25":
            shift = np.array([2.0, -1.5, -25.0])                       # the same rotation seen from 25 m: the staircase moves along
            b = b0 + a0 @ shift
            valid = xyz[..., 2] > 0
            xyz = xyz.copy()
            xyz[valid] = (xyz[valid].astype(np.float64) - shift).astype(np.float32)
        if src == "depth":
            depth, n_set = _depth_on_level(depth, intr, a, b, cfg.z_max, rng, 0.6)
            assert n_set > W * H // 5
        else:
            extra = np.concatenate([_top_points(cfg, a, b, rng, 12000), _bin_edge_points(cfg, a, b, rng, 40)])
            xyz = _place(xyz, extra, rng)
    elif kind == "B":
        if where == "mm":
            # the magnitude test holds every point of the frame; the float x / y decision is right even so (single precision scales),
            # so the range ends mid-bin as in A and the cloud is made for that band too: both per-point tests of CHECKS at once
            drop = ("top",)
            cfg.z_max = cfg.z_min + 100.5 * cfg.height_interval
            a = a0 * 0.001                                              # camera coordinates in millimetres
            xyz = (xyz.astype(np.float64) * 1000.0).astype(np.float32)
            if src == "depth":
                intr.depth_units *= 1000.0                              # the same raw image: every point 1000 times as far
                depth, n_set = _depth_on_level(depth, intr, a, b, cfg.z_max, rng, 0.6)
                assert n_set > W * H // 5
            else:
                xyz = _place(xyz, np.concatenate([_top_points(cfg, a, b, rng, 12000), _bin_edge_points(cfg, a, b, rng, 40)]), rng)
        else:
            # the camera 3 km above the range, x / y offsets as before: the x / y rows' own offsets stay small, the inputs are 3 km -
            # single precision's error exceeds the bound derived for 64 m (make_pre_xy), only the magnitude test saves the decision
            drop = ("far",)
            shift = np.linalg.solve(a0, np.array([0.0, 0.0, 3000.0]))
            b = b0 + a0 @ shift
            valid = xyz[..., 2] > 0
            xyz = xyz.copy()
            xyz[valid] = (xyz[valid].astype(np.float64) - shift).astype(np.float32)
            ref0 = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(_transformation(ssd, base, a, b).constants), xyz)[0]
            treads = [cfg.z_min + (p.peak_bin + 0.5) * cfg.height_interval for p in (ref0.plateaus[i] for i in range(ref0.n_plateaus)) if p.is_step][:2]
            assert treads
            extra = np.concatenate([_limit_points(cfg, a, b, rng, 2500), _pixel_edge_points(cfg, a, b, rng, treads, 1500, W, H)])
            xyz = _place(xyz, extra, rng)
    else:
        drop = ("xy", "z")
        a = a0 * 1e6                                                    # camera coordinates in micrometres ...
        xyz = (xyz.astype(np.float64) * 1e-6).astype(np.float32)
        if where == "all":
            b = b0 + np.array([0.0, 0.0, 10000.0])                      # ... and the world's z origin 10 km below: z cannot be served
            valid = xyz[..., 2] > 0
            xyz = xyz.copy()
            xyz[valid] = (xyz[valid].astype(np.float64) - np.linalg.inv(a) @ np.array([0.0, 0.0, 10000.0])).astype(np.float32)
        ref0 = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(_transformation(ssd, base, a, b).constants), xyz)[0]
        treads = [cfg.z_min + (p.peak_bin + 0.5) * cfg.height_interval for p in (ref0.plateaus[i] for i in range(ref0.n_plateaus)) if p.is_step][:2]
        assert treads
        extra = np.concatenate([_limit_points(cfg, a, b, rng, 1500), _bin_edge_points(cfg, a, b, rng, 40),
                                _pixel_edge_points(cfg, a, b, rng, treads, 1500, W, H)])
        xyz = _place(xyz, extra, rng)
    trans = _transformation(ssd, base, a, b)
    lim = _lim(cfg)
    Q = ssd.prexy_host(*lim, a, b)
    Z = ssd.prez_host(*lim, a, b, height_interval=cfg.height_interval, width=W, height=H)
    # (1) the regime
    if kind == "A":
        assert Z["z_check_top"] and Z["z_h0"] > 0 and Q["lo"] > 0 and Z["px_h0"] > 0
    elif kind == "B":
        assert Q["check_input"] and Q["max_input"] == 64.0 and Q["lo"] > 0 and Z["z_h0"] > 0 and Z["z_check_top"] == (where == "mm")
    else:
        assert Q["lo"] < 0 and np.isinf(Q["hi"]) and Q["max_input"] < 0 and Q["check_input"]
        if where == "xy":
            assert Z["z_h0"] > 0 and Z["px_h0"] > 0                     # the z row and the pixel stay single precision first
        else:
            assert Z["z_h0"] < 0 and Z["z_neg_k"] < 0 and Z["px_h0"] > 0
    frame = depth if src == "depth" else xyz
    pts = (oracle.deproject(intr, depth) if src == "depth" else xyz).reshape(-1, 3)
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants), pts.reshape(H, W, 3))[0]
    # (2) the cloud reaches the band: the model with every band is the oracle; without this case's band it is not
    recip = 1.0 / cfg.height_interval
    ok, hb = pm.reference(lim, a, b, recip, pts)
    inr, hbin, _ = pm.kernel_decisions(Q, Z, lim, a, b, recip, pts)
    assert np.array_equal(inr, ok) and np.array_equal(hbin[ok], hb[ok])
    hist = list(res.hist[:res.n_bins])
    assert int(ok.sum()) == res.n_inrange and list(pm.histogram(ok, hb, res.n_bins)) == hist
    inr_x, hbin_x, _ = pm.kernel_decisions(Q, Z, lim, a, b, recip, pts, drop=drop)
    wrong = (inr_x != ok) | (ok & (hbin_x != hb))
    count = int(wrong.sum())
    if kind == "B":
        M3 = pm.absmax3(pts)
        if where == "mm":
            assert ok.sum() > W * H // 10 and not np.any(ok & (M3 <= 64.0))   # every point in range is beyond max_input
        else:
            assert (ok & (M3 > 64.0)).sum() > W * H // 10
    assert count >= 30, (name, count)
    assert list(pm.histogram(inr_x, hbin_x, res.n_bins)) != hist or int(inr_x.sum()) != res.n_inrange
    return dict(cfg=cfg, trans=trans, frame=frame, intr=intr, src=src, res=res, count=count, W=W, H=H)


@pytest.mark.parametrize("name", CASES)
def test_the_case_is_in_its_regime_and_its_cloud_reaches_the_band(ssd, oracle, name):
    """Host only: build_case's assertions - the regime from prexy_host / prez_host, and the numpy model of the kernel's decisions with
    and without the case's band (the oracle's histogram with it; a few dozen points and the histogram wrong without it)."""
    build_case(ssd, oracle, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_the_kernels_match_the_oracle_in_the_prefilters_regime(ssd, oracle, gpu_device, name):
    """Regime: A (z_check_top), B (check_input with in-range inputs beyond 64 m) or C (all doubles), per the case's name.
    Band: A the top of a z range that ends mid-bin (world z on it, 0 .. 1e-3 of a bin off, and on every bin edge; depth: the raw
    value nearest to it); B the magnitude test - every point of a millimetre calibration (its range ending mid-bin as in A), and a camera 3 km off with points on the
    x / y limits and on pixel edges; C the whole x / y test (limits, bin edges, pixel edges), and z as well for C-all.
    Proof the cloud reaches it: build_case asserts the regime's constants and that the kernel's decisions without the band
    (prefilter_model) get at least 30 points and the oracle's histogram or in-range count wrong.  Records, results and images:
    the oracle's, bit for bit, two passes and the single pass forced."""
    case = build_case(ssd, oracle, name)
    cfg, trans, frame = case["cfg"], case["trans"], case["frame"]
    det = ssd.Detector(cfg, trans, gpu_device)
    buf = ssd.DeviceBuffer(det.frame_bytes + 16, gpu_device) if case["src"] == "f3" else None
    try:
        reps = []
        for mode in (0, 1):
            det.single_pass(mode)
            reps.append(parity.check_frame(ssd, oracle, det, cfg, trans.constants, frame, images=True, depth_intr=case["intr"],
                                           unaligned_buf=buf))
        assert reps[0]["line"] == reps[1]["line"]
        if name.startswith("B-mm"):
            assert reps[0]["n_steps"] >= 2                             # the staircase, all of it through the magnitude test
    finally:
        if buf is not None:
            buf.free()
        det.close()
