"""The depth fusion's rule (include/ssd_hip.h) in numpy, written from the rule's text, and the frames the CPU and
the GPU tests share: the noisy frames of one still scene, and a frame built for the rule's edges, one pixel per case.

For one pixel with samples d_0 .. d_(n-1): a sample is valid iff it is not 0, m of them are; m == 0: output 0, EMPTY; 0 < m < min_valid:
output 0, FEW; med = the (m - 1) // 2-th smallest valid sample; a valid sample agrees iff |d_j - med| <= tol, c of them do, their sum is
s; c < min_agree: output 0, SPLIT; else FUSED and the output is (2 s + c) // (2 c).  The support byte is c for a fused pixel, else 0."""
import numpy as np

STATS = ("n_fused", "n_empty", "n_few", "n_split", "sum_valid", "sum_agree", "sum_abs_dev", "reserved")


def default_rule(n):
    return ((n + 1) // 2, (n + 1) // 2, 40)


def fuse_np(frames, rule=None):
    """frames: uint16 [n, ...]; rule: (min_valid, min_agree, tol) or None for the defaults -> (fused uint16, support uint8, stats dict)"""
    d = np.asarray(frames).astype(np.int64)
    n = d.shape[0]
    min_valid, min_agree, tol = rule if rule is not None else default_rule(n)
    valid = d != 0
    m = valid.sum(axis=0)
    ranked = np.sort(np.where(valid, d, 1 << 20), axis=0)                    # the valid samples first, ascending
    at = np.maximum(m - 1, 0) // 2
    med = np.take_along_axis(ranked, at[None], axis=0)[0]
    agree = valid & (np.abs(d - med[None]) <= tol)
    c = agree.sum(axis=0)
    s = np.where(agree, d, 0).sum(axis=0)
    empty = m == 0
    few = ~empty & (m < min_valid)
    split = ~empty & ~few & (c < min_agree)
    fused = ~empty & ~few & ~split
    out = np.where(fused, (2 * s + c) // np.maximum(2 * c, 1), 0)
    dev = np.where(agree, np.abs(d - out[None]), 0).sum(axis=0)
    assert out.max(initial=0) <= 65535 and (out[fused] > 0).all() and (np.abs(out - med)[fused] <= tol).all()
    stats = dict(n_fused=int(fused.sum()), n_empty=int(empty.sum()), n_few=int(few.sum()), n_split=int(split.sum()), sum_valid=int(m.sum()),
                 sum_agree=int(c[fused].sum()), sum_abs_dev=int(dev[fused].sum()), reserved=0)
    return out.astype(np.uint16), np.where(fused, c, 0).astype(np.uint8), stats


def stats_dict(s):
    return {k: int(getattr(s, k)) for k in STATS}


def rule_of(ssd, rule):
    return None if rule is None else ssd.FuseRule(rule[0], rule[1], rule[2], 0)


def scene_frames(ssd, width, height, n, sigma=0.002, outliers=0.05, invalid=0.02, seed=1000):
    """n depth frames of the 3-step scene that differ in their noise alone (seeds seed .. seed + n - 1), uint16 [n, H, W]"""
    return ssd.synth_depth_host([ssd.make_scene(width, height, n_steps=3, seed=seed + i, sigma=sigma, outlier_frac=outliers, invalid_frac=invalid)
                                 for i in range(n)])


def clean_frame(ssd, width, height):
    """the same scene without noise, outliers or holes (the geometry does not depend on the seed)"""
    return ssd.synth_depth_host([ssd.make_scene(width, height, n_steps=3, seed=1000, sigma=0.0)])[0]


def _column(n, samples):
    """n samples of one pixel: those given, in an order that is not sorted, the rest invalid"""
    assert len(samples) <= n
    col = list(samples) + [0] * (n - len(samples))
    return col[1::2] + col[0::2]


def edge_cases(n, rule):
    """-> list of (name, the pixel's n samples) for the rule's edges, as far as n has room for them"""
    min_valid, min_agree, tol = rule
    far = 20000 + 2 * tol + 500
    cases = [("all invalid", [])]
    cases.append(("m == min_valid - 1", [20000] * (min_valid - 1)))
    cases.append(("m == min_valid", [20000] * min_valid))
    if min_agree >= 2 and n >= min_valid and n >= 2 * (min_agree - 1):
        k = min_agree - 1                                    # two camps of k: the lower one holds the median, nobody joins it
        cases.append(("c == min_agree - 1", [20000] * k + [far] * max(k, min_valid - k)))
    if n >= min_agree + 1:
        cases.append(("c == min_agree", [20000] * min_agree + ([far] if min_agree > 1 else [])))
    if n >= 3:
        for name, other in (("a sample at med + tol", 30000 + tol), ("a sample at med + tol + 1", 30000 + tol + 1),
                            ("a sample at med - tol", 30000 - tol), ("a sample at med - tol - 1", 30000 - tol - 1)):
            cases.append((name, [30000, 30000, other]))
        # far below a small median and far above a large one: a difference that wraps in 16 bits would come back small
        cases.append(("unsigned wrap below", [3, 3, 65535 - tol + 3 if tol < 60000 else 65535]))
        cases.append(("unsigned wrap above", [65534, 65534, 1]))
    if n >= 2:
        cases.append(("even m: the lower median", [1000, 1000 + 2 * tol + 10]))
        cases.append(("a mean ending in one half, even c", [1000, 1001]))
    if n >= 4:
        cases.append(("even m = 4: the lower median of two camps", [1000, 1000, far, far]))
        cases.append(("duplicates of the median", [500, 700, 700, 700]))
    if n >= 3:
        cases.append(("a mean ending in one half, odd c", [1000, 1000, 1000 + (3 if tol >= 3 else 0)]))
        cases.append(("valid samples of 1", [1, 1, 1]))
        cases.append(("valid samples of 65535", [65535, 65535, 65535]))
        cases.append(("a median within tol of 65535 beside invalid samples", [65535 - min(tol, 7), 65535, 65535 - min(tol, 7)]))
    cases.append(("one valid 65535 among invalid samples", [65535]))
    cases.append(("one valid 1 among invalid samples", [1]))
    return [(name, _column(n, s)) for name, s in cases]


def edge_frame(n, rule, width, height, seed=0):
    """uint16 [n, H, W]: the edge cases in the first pixels, then random pixels that mix invalid samples, two camps and near values"""
    cases = edge_cases(n, rule)[:width * height]                 # (a frame of fewer pixels takes the first of them)
    rng = np.random.default_rng(seed + n)
    base = rng.choice(np.array([0, 1, 39, 40, 41, 1000, 30000, 65495, 65535]), size=(height * width,))
    f = base[None, :] + rng.integers(-45, 46, size=(n, height * width))
    f = np.where(rng.random((n, height * width)) < 0.25, 0, np.clip(f, 0, 65535))
    for p, (_, col) in enumerate(cases):
        f[:, p] = col
    return f.reshape(n, height, width).astype(np.uint16), [name for name, _ in cases]


# ---- what the rule achieves (tools/depth_fuse_accuracy.py records it, tests/test_depth_fuse.py holds the host statement to it) ---------
ACC_W, ACC_H, ACC_N, ACC_FAR = 256, 192, 8, 40


def pixel_figures(frame, clean, far=ACC_FAR):
    """a frame against the clean one -> (share of its valid pixels more than `far` raw units off, rms of the remaining valid pixels in
    raw units, share of invalid pixels)"""
    valid = frame != 0
    err = np.abs(frame.astype(np.int64) - clean.astype(np.int64))
    off = valid & (err > far)
    rest = valid & ~off
    return (float(off.sum()) / max(int(valid.sum()), 1), float(np.sqrt((err[rest].astype(np.float64) ** 2).mean())) if rest.any() else 0.0,
            1.0 - float(valid.mean()))


def accuracy_rows(ssd):
    """the issue's table: (label, sigma, outliers, invalid, n) -> single frame and fused figures, from ssd_depth_fuse_host"""
    rows = []
    clean = clean_frame(ssd, ACC_W, ACC_H)
    for sigma, outl, inv, n in ((0.002, 0.05, 0.02, 3), (0.002, 0.05, 0.02, 5), (0.002, 0.05, 0.02, 8), (0.002, 0.05, 0.02, 16),
                                (0.003, 0.05, 0.10, 8), (0.001, 0.0, 0.0, 8)):
        frames = scene_frames(ssd, ACC_W, ACC_H, n, sigma, outl, inv)
        fused, stats = ssd.depth_fuse_host(frames)
        rows.append(dict(sigma=sigma, outliers=outl, invalid=inv, n=n, single=pixel_figures(frames[0], clean), fused=pixel_figures(fused, clean),
                         stats=stats_dict(stats)))
    return rows


def detection_figures(ssd, oracle):
    """the eight frames of the table's third row through the CPU oracle, one by one and fused: step counts and the worst step height
    error against the clean frame's detection"""
    import oracle_binding as ob
    sc = ssd.make_scene(ACC_W, ACC_H, n_steps=3, seed=1000, sigma=0.0)
    intr = ssd.intrinsics_for_scene(sc)
    ocfg = ob.to_oracle_config(ssd.default_config(ACC_W, ACC_H))
    ocal = ob.to_oracle_calibration(ssd.transformation_for_scene(sc).constants)

    def detect(depth):
        n, steps, _ = oracle.process_lean(ocfg, ocal, ssd.deproject_host(intr, depth))
        return n, [float(s[0]) for s in steps]

    def worst(heights, ref):
        return max((abs(a - b) for a, b in zip(heights, ref)), default=0.0) if len(heights) == len(ref) else float("inf")
    frames = scene_frames(ssd, ACC_W, ACC_H, ACC_N)
    clean_n, clean_h = detect(clean_frame(ssd, ACC_W, ACC_H))
    singles = [detect(f) for f in frames]
    fused_n, fused_h = detect(ssd.depth_fuse_host(frames)[0])
    return dict(clean_steps=clean_n, clean_heights=clean_h, single_steps=[n for n, _ in singles], single_worst=[worst(h, clean_h) for _, h in singles],
                fused_steps=fused_n, fused_worst=worst(fused_h, clean_h))
