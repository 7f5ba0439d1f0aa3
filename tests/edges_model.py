"""The depth edge filter's rule (include/ssd_hip.h) in numpy, written from the rule's text, and what the CPU and the
GPU tests share: a seeded model of mixed pixels, small frames stated by hand, one per edge of the rule, frames whose planted pixels sit on
the kernel's seams, and the figures of profiles/depth_edges_accuracy.txt.

For the pixel with sample d: t = min(65535, tol + ((d * slope) >> 12)); a neighbour q (one of the up to eight pixels around it inside the
frame) is near iff d_q != 0 and |d_q - d| <= t; c = the number of near neighbours; the pixel is bridged iff for one of the opposite pairs
W/E, N/S, NW/SE, NE/SW, both inside the frame and not 0, (d_a + t < d and d + t < d_b) or (d_b + t < d and d + t < d_a).  Classes in this
order: EMPTY (1) d == 0; LONE (2) c < min_support; BRIDGE (3) bridge != 0 and bridged; else KEPT (0), the only one whose output is d."""
import numpy as np

KEPT, EMPTY, LONE, BRIDGE = 0, 1, 2, 3
STATS = ("n_kept", "n_empty", "n_lone", "n_bridge", "sum_support")
SLOPES = (0, 16, 32, 64, 128, 256)          # the candidates for the default slope
DEFAULT = (2, 1, 40, 0)                     # min_support, bridge, tol, slope (profiles/depth_edges_accuracy.txt: the measured choice)
RULES = (None, (0, 1, 40, 32), (2, 0, 40, 32), (2, 1, 40, 0), (1, 1, 0, 64), (8, 1, 65535, 4096), (3, 1, 7, 4096))
PAIRS = (((0, -1), (0, 1)), ((-1, 0), (1, 0)), ((-1, -1), (1, 1)), ((-1, 1), (1, -1)))    # (dy, dx) of a and b


def edges_np(frame, rule=None):
    """frame: uint16 [H, W]; rule: (min_support, bridge, tol, slope) or None for the defaults -> (out uint16, classes uint8, stats dict)"""
    min_support, bridge, tol, slope = rule if rule is not None else DEFAULT
    d = np.asarray(frame).astype(np.int64)
    H, W = d.shape
    pad = np.zeros((H + 2, W + 2), np.int64)                       # a pixel outside the frame does not exist: as an invalid one, it is
    pad[1:-1, 1:-1] = d                                            # never near and never one end of a bridge
    t = np.minimum(65535, tol + ((d * slope) >> 12))

    def nb(dy, dx):
        return pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    c = np.zeros((H, W), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                q = nb(dy, dx)
                c += (q != 0) & (np.abs(q - d) <= t)
    bridged = np.zeros((H, W), bool)
    for (ay, ax), (by, bx) in PAIRS:
        a, b = nb(ay, ax), nb(by, bx)
        bridged |= (a != 0) & (b != 0) & (((a + t < d) & (d + t < b)) | ((b + t < d) & (d + t < a)))
    cls = np.where(d == 0, EMPTY, np.where(c < min_support, LONE, np.where((bridge != 0) & bridged, BRIDGE, KEPT)))
    out = np.where(cls == KEPT, d, 0)
    stats = dict(n_kept=int((cls == KEPT).sum()), n_empty=int((cls == EMPTY).sum()), n_lone=int((cls == LONE).sum()),
                 n_bridge=int((cls == BRIDGE).sum()), sum_support=int(c[cls == KEPT].sum()))
    return out.astype(np.uint16), cls.astype(np.uint8), stats


def stats_dict(s):
    assert list(s.reserved) == [0, 0, 0]
    return {k: int(getattr(s, k)) for k in STATS}


def rule_of(ssd, rule):
    return None if rule is None else ssd.EdgeRule(*rule)


def t_of(d, rule=None):
    _, _, tol, slope = rule if rule is not None else DEFAULT
    return min(65535, tol + ((int(d) * slope) >> 12))


# ---- frames -------------------------------------------------------------------------------------------------------------------------------
def clean_frame(ssd, width, height, **kw):
    """the 3-step scene without noise, outliers or holes"""
    return ssd.synth_depth_host([ssd.make_scene(width, height, n_steps=3, seed=1000, sigma=0.0, **kw)])[0]


def stress_frame(ssd, width, height, seed=1000):
    """the stress configuration: sigma 2 mm, 5 % random depths, 2 % invalid"""
    return ssd.synth_depth_host([ssd.make_scene(width, height, n_steps=3, seed=seed, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02)])[0]


def plant_mixed(clean, jump=200, seed=7, rule=None):
    """The mixed-pixel model.  Every valid pixel of `clean` one of whose valid 4-neighbours differs from it by more than `jump` raw units is
    replaced by near + u * (far - near): near and far are the smaller and the larger of the pixel and the 4-neighbour that differs most, u is
    uniform in (0, 1) per pixel from the seed.  -> (frame, planted bool [H, W], truth bool [H, W]).  Both sides of a discontinuity are
    planted.  truth: the planted pixels that lie more than t (of their new sample) from both sides - across the axis of their jump, in the
    frame as planted, one neighbour is valid and more than t below and the opposite one valid and more than t above."""
    d = np.asarray(clean).astype(np.int64)
    H, W = d.shape
    rng = np.random.default_rng(seed)
    u = rng.uniform(0.0, 1.0, size=(H, W))
    pad = np.zeros((H + 2, W + 2), np.int64)
    pad[1:-1, 1:-1] = d
    best, axis = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    other = d.copy()
    for k, (dy, dx) in enumerate(((0, -1), (0, 1), (-1, 0), (1, 0))):
        q = pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        diff = np.where((q != 0) & (d != 0), np.abs(q - d), 0)
        take = diff > best
        best, other, axis = np.where(take, diff, best), np.where(take, q, other), np.where(take, k // 2, axis)
    planted = best > jump
    near, far = np.minimum(d, other), np.maximum(d, other)
    mixed = np.clip(np.rint(near + u * (far - near)).astype(np.int64), 1, 65535)
    f = np.where(planted, mixed, d)
    fp = np.zeros((H + 2, W + 2), np.int64)
    fp[1:-1, 1:-1] = f
    _, _, tol, slope = rule if rule is not None else DEFAULT
    t = np.minimum(65535, tol + ((f * slope) >> 12))
    truth = np.zeros((H, W), bool)
    for k, ((ay, ax), (by, bx)) in enumerate(PAIRS[:2]):
        a, b = fp[1 + ay:1 + ay + H, 1 + ax:1 + ax + W], fp[1 + by:1 + by + H, 1 + bx:1 + bx + W]
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        truth |= planted & (axis == k) & (lo != 0) & (f - lo > t) & (hi - f > t)
    return f.astype(np.uint16), planted, truth


def hand_frames():
    """-> [(name, frame uint16 [H, W], rule, {(y, x): (output, class)})]: the rule's edges, one small frame per case, with what the rule's
    TEXT says must come out of the named pixels - stated here, taken from no implementation.  t = 40 under the defaults."""
    A = lambda rows: np.array(rows, np.uint16)                                                   # noqa: E731
    out = []
    # a corner pixel has 3 neighbours, an edge pixel 5: min_support at the count and one above it
    f = A([[1000] * 3] * 3)
    out.append(("corner and edge at min_support 3", f, (3, 0, 40, 0), {(0, 0): (1000, KEPT), (0, 1): (1000, KEPT), (1, 1): (1000, KEPT)}))
    out.append(("corner below min_support 4", f, (4, 0, 40, 0), {(0, 0): (0, LONE), (2, 2): (0, LONE), (0, 1): (1000, KEPT), (1, 1): (1000, KEPT)}))
    out.append(("edge at min_support 5", f, (5, 0, 40, 0), {(0, 0): (0, LONE), (0, 1): (1000, KEPT), (1, 0): (1000, KEPT), (1, 1): (1000, KEPT)}))
    out.append(("edge below min_support 6", f, (6, 0, 40, 0), {(0, 1): (0, LONE), (1, 2): (0, LONE), (1, 1): (1000, KEPT)}))
    out.append(("centre at 8 and nothing at more", f, (8, 0, 40, 0), {(1, 1): (1000, KEPT), (0, 1): (0, LONE)}))
    # a neighbour at exactly t and at t + 1 (the centre's view; the neighbour's own t is the same: slope 0)
    out.append(("a neighbour at exactly t", A([[1000, 1040]]), (1, 0, 40, 0), {(0, 0): (1000, KEPT), (0, 1): (1040, KEPT)}))
    out.append(("a neighbour at t + 1", A([[1000, 1041]]), (1, 0, 40, 0), {(0, 0): (0, LONE), (0, 1): (0, LONE)}))
    out.append(("a neighbour at exactly t below", A([[1000], [960]]), (1, 0, 40, 0), {(0, 0): (1000, KEPT), (1, 0): (960, KEPT)}))
    out.append(("t grows with the depth", A([[4096, 4096 + 72, 4096 + 73 + 73]]), (1, 0, 40, 32),
                {(0, 0): (4096, KEPT), (0, 1): (4168, KEPT), (0, 2): (0, LONE)}))   # t(4096) = 72, t(4168) = 72: 4242 is 74 from 4168
    # 3 beside 65500: a difference that wraps in 16 bits would come back as 39
    out.append(("3 beside 65500", A([[3, 65500]]), (1, 0, 40, 0), {(0, 0): (0, LONE), (0, 1): (0, LONE)}))
    out.append(("65500 between 3 and 3 is no bridge", A([[3, 65500, 3]]), (0, 1, 40, 0), {(0, 1): (65500, KEPT)}))
    # d = 65535 with slope 4096: t = min(65535, 40 + 65535) saturates; unsaturated it would be 65575, which wraps to 39 in 16 bits
    out.append(("t saturates at 65535", A([[65535, 1, 65535]]), (1, 1, 40, 4096), {(0, 0): (65535, KEPT), (0, 1): (0, LONE), (0, 2): (65535, KEPT)}))
    out.append(("t saturates: everything valid is near", A([[65535, 30000], [100, 65535]]), (3, 1, 40, 4096),
                {(0, 0): (65535, KEPT), (1, 1): (65535, KEPT), (0, 1): (0, LONE), (1, 0): (0, LONE)}))
    # a bridge at exactly t (not bridged) and at t + 1, on each of the four pairs; min_support 0: only BRIDGE decides
    for name, (ay, ax), (by, bx) in (("W/E", (1, 0), (1, 2)), ("N/S", (0, 1), (2, 1)), ("NW/SE", (0, 0), (2, 2)), ("NE/SW", (0, 2), (2, 0))):
        for flip in (False, True):
            for gap, want in ((40, (1000, KEPT)), (41, (0, BRIDGE))):
                f = np.zeros((3, 3), np.uint16)
                f[1, 1] = 1000
                f[(by, bx) if flip else (ay, ax)] = 1000 - gap
                f[(ay, ax) if flip else (by, bx)] = 1000 + 41
                out.append(("bridge %s below at %d%s" % (name, gap, " flipped" if flip else ""), f, (0, 1, 40, 0), {(1, 1): want}))
                f = f.copy()
                f[(by, bx) if flip else (ay, ax)] = 1000 - 41
                f[(ay, ax) if flip else (by, bx)] = 1000 + gap
                out.append(("bridge %s above at %d%s" % (name, gap, " flipped" if flip else ""), f, (0, 1, 40, 0), {(1, 1): want}))
    out.append(("bridge switched off", A([[900, 1000, 1100]]), (0, 0, 40, 0), {(0, 1): (1000, KEPT)}))
    out.append(("both sides below is no bridge", A([[900, 1000, 900]]), (0, 1, 40, 0), {(0, 1): (1000, KEPT)}))
    # a pair with one pixel missing or invalid
    out.append(("a pair with one pixel outside the frame", A([[1000, 1100]]), (0, 1, 40, 0), {(0, 0): (1000, KEPT), (0, 1): (1100, KEPT)}))
    out.append(("a pair with one pixel invalid", A([[0, 1000, 1100]]), (0, 1, 40, 0), {(0, 0): (0, EMPTY), (0, 1): (1000, KEPT)}))
    out.append(("a pair with the low pixel invalid", A([[900], [1000], [0]]), (0, 1, 40, 0), {(1, 0): (1000, KEPT)}))
    # LONE and bridged at once: the class order decides
    out.append(("lone and bridged: LONE", A([[900, 1000, 1100]]), (1, 1, 40, 0), {(0, 1): (0, LONE), (0, 0): (0, LONE), (0, 2): (0, LONE)}))
    out.append(("bridged with support: BRIDGE", A([[900, 1000, 1100], [0, 1010, 0]]), (1, 1, 40, 0), {(0, 1): (0, BRIDGE), (1, 1): (1010, KEPT)}))
    out.append(("empty first", A([[900, 0, 1100]]), (0, 1, 40, 0), {(0, 1): (0, EMPTY)}))
    # 1 x 1, 1 x N, N x 1
    out.append(("1 x 1 valid", A([[1234]]), (0, 1, 40, 32), {(0, 0): (1234, KEPT)}))
    out.append(("1 x 1 valid, lone", A([[1234]]), (1, 1, 40, 32), {(0, 0): (0, LONE)}))
    out.append(("1 x 1 empty", A([[0]]), None, {(0, 0): (0, EMPTY)}))
    out.append(("1 x N", A([[1000, 1010, 1020, 0, 5000, 5040, 5081]]), (1, 1, 40, 0),
                {(0, 0): (1000, KEPT), (0, 1): (1010, KEPT), (0, 2): (1020, KEPT), (0, 3): (0, EMPTY), (0, 4): (5000, KEPT), (0, 5): (5040, KEPT),
                 (0, 6): (0, LONE)}))
    out.append(("N x 1", A([[1000], [1010], [1200], [1400], [1410]]), (1, 1, 40, 0),
                {(0, 0): (1000, KEPT), (1, 0): (1010, KEPT), (2, 0): (0, LONE), (3, 0): (1400, KEPT), (4, 0): (1410, KEPT)}))
    out.append(("the defaults on a flat patch with a flying pixel", A([[1000] * 3, [1000, 1500, 1000], [2000] * 3]), None,
                {(1, 1): (0, LONE), (0, 0): (1000, KEPT), (1, 0): (1000, KEPT), (2, 1): (2000, KEPT)}))
    out.append(("the defaults: a mixed pixel with company", A([[1000, 1500, 2000], [1000, 1500, 2000], [1000, 1500, 2000]]), None,
                {(1, 1): (0, BRIDGE), (0, 1): (0, LONE), (1, 0): (1000, KEPT), (1, 2): (2000, KEPT)}))
    return out


def ramp(width, height, step, base=1000):
    """a surface that steps by `step` raw units from pixel to pixel along a row, the same in every row"""
    return (base + step * np.arange(width, dtype=np.int64))[None, :].repeat(height, 0).astype(np.uint16)


def seam_frame(width, height, seams_x, seams_y, seed=0):
    """a seeded frame of plateaus, jumps, zeros and 65535s whose planted pixels (lone ones, mixed ones between two plateaus, zeros, 65535s)
    sit on the given seams: on columns x - 1 and x of every seam column x and rows y - 1 and y of every seam row y, as far as they lie
    inside the frame"""
    rng = np.random.default_rng(seed + 31 * width + height)
    levels = np.array([900, 1000, 1040, 1041, 3000, 20000, 65400, 65535])
    f = levels[rng.integers(0, len(levels), size=((height + 3) // 4, (width + 4) // 5))].repeat(4, 0).repeat(5, 1)[:height, :width].astype(np.int64)
    f += rng.integers(-6, 7, size=f.shape)
    f = np.clip(f, 1, 65535)
    f[rng.random(f.shape) < 0.03] = 0
    special = np.array([0, 65535, 1, 950, 1020, 1500, 2000, 12000, 65495])
    cols = sorted({c for x in seams_x for c in (x - 1, x) if 0 <= c < width})
    rows = sorted({r for y in seams_y for r in (y - 1, y) if 0 <= r < height})
    for c in cols:
        f[:, c] = np.where(rng.random(height) < 0.6, special[rng.integers(0, len(special), size=height)], f[:, c])
    for r in rows:
        f[r, :] = np.where(rng.random(width) < 0.6, special[rng.integers(0, len(special), size=width)], f[r, :])
    return f.astype(np.uint16)


# ---- what the rule achieves (tools/depth_edges_accuracy.py records it, tests/test_depth_edges.py holds the host statement to it) -----------
ACC_W, ACC_H, ACC_JUMP, LOSS_CAP = 256, 192, 200, 0.001


def sweep_loss(ssd, oracle, slope):
    """the noise-free depth frames of the scenes in tests/sweep_scenes.py under (2, 1, 40, slope): of the pixels the oracle's labels assign
    to a reported surface, how many the filter removes -> (removed, labelled)"""
    import sweep_scenes as sw
    s = _clean_sweep(ssd, oracle)
    removed = labelled = 0
    for frame, lab in zip(s.frames, s.labels):
        out, _ = ssd.depth_edges_host(frame, ssd.EdgeRule(2, 1, 40, slope))
        on = lab.reshape(frame.shape) != 0
        labelled += int(on.sum())
        removed += int((on & (out == 0)).sum())
    del sw
    return removed, labelled


_CLEAN = {}


def _clean_sweep(ssd, oracle):
    import sweep_scenes as sw
    if "s" not in _CLEAN:
        entries = [(g, v, dict(kw, sigma=0.0, outlier_frac=0.0, invalid_frac=0.0)) for g, v, kw in sw.scene_list()]
        _CLEAN["s"] = sw.Sweep(ssd, oracle, depth=True, entries=entries)
    return _CLEAN["s"]


def chosen_slope(ssd, oracle):
    """-> (the smallest candidate whose loss is within LOSS_CAP or None, [(slope, removed, labelled)])"""
    rows = [(s,) + sweep_loss(ssd, oracle, s) for s in SLOPES]
    ok = [s for s, r, n in rows if r <= LOSS_CAP * n]
    return (ok[0] if ok else None), rows


def _staircase(ssd, oracle):
    """the clean 3-step frame, the oracle's detection of it and its labels, and the same frame with a box on every reported surface: a
    patch of 25 pixels by half the surface's rows around its middle, 10 % nearer to the camera along its rays"""
    import clearance_model as cm
    import oracle_binding as ob
    from test_labels import expected_labels
    if "stairs" not in _CLEAN:
        sc = ssd.make_scene(ACC_W, ACC_H, n_steps=3, seed=1000, sigma=0.0)
        cfg, intr, cal = ssd.default_config(ACC_W, ACC_H), ssd.intrinsics_for_scene(sc), ssd.transformation_for_scene(sc).constants
        clean = clean_frame(ssd, ACC_W, ACC_H)
        pts = ssd.deproject_host(intr, clean)
        rec = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), pts)[0]
        result = cm.result_of_oracle(ssd, rec)
        labels = expected_labels(oracle, cfg, cal, rec, pts).reshape(ACC_H, ACC_W)
        boxed = clean.copy()
        for k in range(1, int(result.n_steps) + 1):
            ys, xs = np.nonzero(labels == k)
            if len(ys):
                cy, cx, h = int(np.median(ys)), int(np.median(xs)), max(2, int(ys.max() - ys.min()) // 4)
                boxed[cy - h:cy + h + 1, cx - 12:cx + 13] = (boxed[cy - h:cy + h + 1, cx - 12:cx + 13] * 0.9).astype(np.uint16)
        _CLEAN["stairs"] = dict(cfg=cfg, intr=intr, cal=cal, clean=clean, result=result, labels=labels, boxed=boxed)
    return _CLEAN["stairs"]


def _occupants(ssd, oracle, depth):
    """occupants per reported surface from ssd_clearance_host over a depth frame, against the CLEAN frame's detection"""
    s = _staircase(ssd, oracle)
    _, mask = ssd.clearance_host(s["cfg"], s["cal"], depth, s["result"], 1, intr=s["intr"])
    return [int((mask == k + 1).sum()) for k in range(int(s["result"].n_steps))]


def accuracy(ssd, oracle):
    """the figures of profiles/depth_edges_accuracy.txt under the default rule at ACC_W x ACC_H, the 3-step scene"""
    s = _staircase(ssd, oracle)
    clean = s["clean"]
    f, planted, truth = plant_mixed(clean, ACC_JUMP)
    out, st = ssd.depth_edges_host(f)
    cout, cst = ssd.depth_edges_host(clean)
    on = s["labels"] != 0
    noisy = stress_frame(ssd, ACC_W, ACC_H)
    nclean = ssd.synth_depth_host([ssd.make_scene(ACC_W, ACC_H, n_steps=3, seed=1000, sigma=0.002, outlier_frac=0.0, invalid_frac=0.02)])[0]
    nout, _ = ssd.depth_edges_host(noisy)
    # the stress configuration's outliers: the pixels whose sample differs from the same seed's frame without outliers
    outlier = (noisy != nclean) & (noisy != 0)
    inlier = (noisy == nclean) & (noisy != 0)
    bf, bplanted, _ = plant_mixed(s["boxed"], ACC_JUMP)
    bout, _ = ssd.depth_edges_host(bf)
    return dict(planted=int(planted.sum()), truth=int(truth.sum()), truth_removed=int((truth & (out == 0)).sum()),
                planted_removed=int((planted & (out == 0)).sum()),
                clean_valid=int((clean != 0).sum()), clean_removed=int(((clean != 0) & (cout == 0)).sum()),
                surface=int(on.sum()), surface_removed=int((on & (cout == 0)).sum()),
                outliers=int(outlier.sum()), outliers_removed=int((outlier & (nout == 0)).sum()),
                inliers=int(inlier.sum()), inliers_removed=int((inlier & (nout == 0)).sum()),
                occupants_before=_occupants(ssd, oracle, f), occupants_after=_occupants(ssd, oracle, out),
                box_planted=int(bplanted.sum()), box_alone=_occupants(ssd, oracle, s["boxed"]), box_before=_occupants(ssd, oracle, bf),
                box_after=_occupants(ssd, oracle, bout), stats=stats_dict(st), clean_stats=stats_dict(cst))


def accuracy_lines(ssd, oracle):
    slope, rows = chosen_slope(ssd, oracle)
    a = accuracy(ssd, oracle)
    lines = ["# tools/depth_edges_accuracy.py: host statement and oracle only",
             "# (a) the default slope: the noise-free depth frames of tests/sweep_scenes.py (%d x %d), rule (2, 1, 40, slope); of the pixels the"
             % (ACC_W, ACC_H),
             "#     oracle's labels assign to a reported surface, those the filter removes; the cap is %.1f %%" % (100 * LOSS_CAP)]
    lines += ["slope %4d: removed %6d of %7d labelled pixels = %.4f %%" % (s, r, n, 100.0 * r / max(n, 1)) for s, r, n in rows]
    lines += ["chosen slope = %s" % slope,
              "# (b) %d x %d, the 3-step scene, the default rule (2, 1, 40, %d); mixed pixels planted at jumps above %d raw units" % (ACC_W, ACC_H, DEFAULT[3], ACC_JUMP),
              "truth subset removed = %d of %d" % (a["truth_removed"], a["truth"]),
              "planted pixels removed = %d of %d" % (a["planted_removed"], a["planted"]),
              "clean valid pixels removed = %d of %d" % (a["clean_removed"], a["clean_valid"]),
              "clean surface pixels (the oracle's labels) removed = %d of %d" % (a["surface_removed"], a["surface"]),
              "stress outliers removed = %d of %d" % (a["outliers_removed"], a["outliers"]),
              "stress inliers removed = %d of %d" % (a["inliers_removed"], a["inliers"]),
              "occupants per surface, planted scene: before -> after = %s" % "  ".join("%d -> %d" % p for p in zip(a["occupants_before"], a["occupants_after"])),
              "# a box on every surface (25 pixels wide, 10 %% nearer), %d pixels planted at its silhouette and the scene's jumps" % a["box_planted"],
              "occupants per surface, the boxes alone = %s" % " ".join(str(n) for n in a["box_alone"]),
              "occupants per surface, boxes with planted pixels: before -> after = %s" % "  ".join("%d -> %d" % p for p in zip(a["box_before"], a["box_after"]))]
    return lines
