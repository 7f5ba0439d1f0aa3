"""The depth fill's rule (include/ssd_hip.h) in numpy, written from the rule's text, and the frames, rules and
recipes the CPU and the GPU tests share.

A pixel outside the frame is the sample 0.  For the pixel with sample d, the opposite pairs (a, b) in the order W/E, N/S, NW/SE, NE/SW:
  lo = min(a, b), hi = max(a, b), t = min(65535, tol + ((lo * slope) >> 12))
  agrees: a != 0 and b != 0 and hi - lo <= t;  m = (a + b + 1) >> 1;  covers: agrees and hi + t < d
EMPTY d == 0 with fewer than min_pairs agreeing pairs -> 0; FILLED d == 0 otherwise -> the m of the agreeing pair with the smallest
hi - lo, the first on a tie; COVERED d != 0, cover != 0, at least cover covering pairs -> the m of the covering pair with the smallest
hi - lo, the first on a tie; otherwise KEPT -> d.  The record: the four counts, sum_pairs (the agreeing pairs of FILLED pixels plus the
covering pairs of COVERED ones) and sum_spread (the hi - lo of the pair each FILLED or COVERED pixel took its m from)."""
import numpy as np

import warp_model as wm

KEPT, EMPTY, FILLED, COVERED = 0, 1, 2, 3
STATS = ("n_kept", "n_empty", "n_filled", "n_covered", "sum_pairs", "sum_spread")
PAIRS = (((0, -1), (0, 1)), ((-1, 0), (1, 0)), ((-1, -1), (1, 1)), ((-1, 1), (1, -1)))      # (dy, dx) of a and b
DEFAULT = dict(min_pairs=1, cover=1, tol=40, slope=0)
# the rule variants both tiers run: each min_pairs, each cover, a slope, tol 0, and the ends of the ranges
RULES = (dict(DEFAULT), dict(DEFAULT, min_pairs=2), dict(DEFAULT, min_pairs=3), dict(DEFAULT, min_pairs=4), dict(DEFAULT, cover=0),
         dict(DEFAULT, cover=2), dict(DEFAULT, slope=32), dict(DEFAULT, tol=0), dict(DEFAULT, tol=0, slope=32, cover=3),
         dict(min_pairs=2, cover=4, tol=65535, slope=4096), dict(DEFAULT, tol=3, slope=4096))


def shift(f, dy, dx):
    H, W = f.shape
    p = np.zeros((H + 2, W + 2), np.int64)
    p[1:-1, 1:-1] = f
    return p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]


def fill_np(frame, tol=40, slope=0, min_pairs=1, cover=1):
    """frame uint16 [H, W] -> (filled uint16 [H, W], classes uint8 [H, W], record dict)"""
    f = np.asarray(frame).astype(np.int64)
    big = np.full(f.shape, 1 << 30)
    bs, bm, na, cs, cm, nc = big.copy(), 0 * f, 0 * f, big.copy(), 0 * f, 0 * f
    for pa, pb in PAIRS:
        a, b = shift(f, *pa), shift(f, *pb)
        lo, hi = np.minimum(a, b), np.maximum(a, b)
        t = np.minimum(65535, tol + ((lo * slope) >> 12))
        ag = (a != 0) & (b != 0) & (hi - lo <= t)
        m = (a + b + 1) >> 1
        k = ag & (hi - lo < bs)
        bs, bm = np.where(k, hi - lo, bs), np.where(k, m, bm)
        na += ag
        cv = ag & (hi + t < f)
        k = cv & (hi - lo < cs)
        cs, cm = np.where(k, hi - lo, cs), np.where(k, m, cm)
        nc += cv
    filled = (f == 0) & (na >= min_pairs)
    covered = (f != 0) & (cover > 0) & (nc >= max(cover, 1))
    out = np.where(filled, bm, np.where(covered, cm, f)).astype(np.uint16)
    cls = np.where(filled, FILLED, np.where(covered, COVERED, np.where(f == 0, EMPTY, KEPT))).astype(np.uint8)
    stats = dict(n_kept=int((cls == KEPT).sum()), n_empty=int((cls == EMPTY).sum()), n_filled=int(filled.sum()), n_covered=int(covered.sum()),
                 sum_pairs=int(na[filled].sum() + nc[covered].sum()), sum_spread=int(bs[filled].sum() + cs[covered].sum()))
    return out, cls, stats


def make_rule(ssd, r=None):
    rule = ssd.FillRule()
    for k, v in dict(DEFAULT, **(r or {})).items():
        setattr(rule, k, v)
    return rule


def stats_dict(s):
    return {k: int(getattr(s, k)) for k in STATS}


def host(ssd, frame, r=None):
    """ssd_depth_fill_host held to the model and to the record's sums -> (filled, classes, record dict)"""
    out, st, cls = ssd.depth_fill_host(frame, make_rule(ssd, r), classes=True)
    want, want_cls, want_st = fill_np(frame, **dict(DEFAULT, **(r or {})))
    got = stats_dict(st)
    assert (out == want).all() and (cls == want_cls).all() and got == want_st, (r, got, want_st)
    assert sum(got[k] for k in STATS[:4]) == np.asarray(frame).size and list(st.reserved) == [0, 0]
    return out, cls, got


# ---- frames stated by hand: (name, rule, frame, the expected centre output / class or None, where) ------------------------------------
def _around(centre, **at):
    """a 3 x 3 frame: the centre and the named neighbours (w e n s nw se ne sw), everything else 0"""
    pos = dict(nw=(0, 0), n=(0, 1), ne=(0, 2), w=(1, 0), e=(1, 2), sw=(2, 0), s=(2, 1), se=(2, 2))
    f = np.zeros((3, 3), np.uint16)
    f[1, 1] = centre
    for k, v in at.items():
        f[pos[k]] = v
    return f


PAIR_ENDS = (("w", "e"), ("n", "s"), ("nw", "se"), ("ne", "sw"))


def hand_frames():
    """[(name, rule dict, frame uint16, expected output at (1, 1), expected class at (1, 1))]: what the rule's text says must come out,
    stated here and not taken from any implementation"""
    out = []
    for i, (a, b) in enumerate(PAIR_ENDS):
        # each pair alone: agreeing at a spread of exactly t, failing at t + 1
        out.append(("pair %d at t" % i, dict(tol=40), _around(0, **{a: 1000, b: 1040}), 1020, FILLED))
        out.append(("pair %d at t + 1" % i, dict(tol=40), _around(0, **{a: 1000, b: 1041}), 0, EMPTY))
        out.append(("pair %d swapped at t" % i, dict(tol=40), _around(0, **{a: 1040, b: 1000}), 1020, FILLED))
        # ... with a slope: t = 3 + ((4096 * 32) >> 12) = 35 at lo = 4096
        out.append(("pair %d at sloped t" % i, dict(tol=3, slope=32), _around(0, **{a: 4096, b: 4131}), 4114, FILLED))
        out.append(("pair %d at sloped t + 1" % i, dict(tol=3, slope=32), _around(0, **{a: 4096, b: 4132}), 0, EMPTY))
    # ties: two pairs of one spread, the first in the rule's order wins - in both orders of the values
    for i in range(4):
        for j in range(i + 1, 4):
            (a, b), (c, d) = PAIR_ENDS[i], PAIR_ENDS[j]
            out.append(("tie %d %d" % (i, j), {}, _around(0, **{a: 1000, b: 1010, c: 2000, d: 2010}), 1005, FILLED))
            out.append(("tie %d %d the other way" % (i, j), {}, _around(0, **{a: 2000, b: 2010, c: 1000, d: 1010}), 2005, FILLED))
    # the smaller spread wins over an earlier pair
    out.append(("later pair is tighter", {}, _around(0, w=1000, e=1020, ne=3000, sw=3019), 3010, FILLED))
    # m rounds up for a + b odd
    out.append(("m rounds up", {}, _around(0, n=1000, s=1001), 1001, FILLED))
    out.append(("m rounds up, swapped", {}, _around(0, n=1001, s=1000), 1001, FILLED))
    out.append(("m of 1 and 2", {}, _around(0, w=1, e=2), 2, FILLED))
    # 65535 beside 65535, and t saturating: tol + ((lo * slope) >> 12) = 65535 + lo > 65535
    out.append(("65535 beside 65535", dict(tol=0), _around(0, w=65535, e=65535), 65535, FILLED))
    out.append(("65535 beside 65534", {}, _around(0, nw=65535, se=65534), 65535, FILLED))
    out.append(("t saturates", dict(tol=65535, slope=4096), _around(0, w=1, e=65535), 32768, FILLED))
    out.append(("t saturates: no cover above 65535", dict(tol=65535, slope=4096), _around(65535, w=1, e=2), 65535, KEPT))
    out.append(("slope 4096 doubles", dict(tol=0, slope=4096), _around(0, n=100, s=200), 150, FILLED))
    out.append(("slope 4096 doubles, one more", dict(tol=0, slope=4096), _around(0, n=100, s=201), 0, EMPTY))
    # min_pairs reached and missed by one
    three = dict(w=1000, e=1001, n=1002, s=1003, nw=1004, se=1005)
    out.append(("min_pairs 3 reached", dict(min_pairs=3), _around(0, **three), 1001, FILLED))
    out.append(("min_pairs 4 missed", dict(min_pairs=4), _around(0, **three), 0, EMPTY))
    out.append(("min_pairs 4 reached", dict(min_pairs=4), _around(0, ne=1006, sw=1007, **three), 1001, FILLED))
    out.append(("min_pairs 2 missed", dict(min_pairs=2), _around(0, w=1000, e=1001, n=1002, s=2000), 0, EMPTY))
    # covers at hi + t == d (not covered) and hi + t + 1 == d
    out.append(("covers: hi + t == d", {}, _around(1050, w=1000, e=1010), 1050, KEPT))
    out.append(("covers: hi + t + 1 == d", {}, _around(1051, w=1000, e=1010), 1005, COVERED))
    out.append(("covers is against hi", {}, _around(1045, w=1000, e=1010), 1045, KEPT))
    # cover reached and missed by one; the covering pair with the smallest spread, not the agreeing one
    two = dict(w=1000, e=1010, n=1003, s=1004)
    out.append(("cover 2 reached", dict(cover=2), _around(2000, **two), 1004, COVERED))
    out.append(("cover 3 missed", dict(cover=3), _around(2000, **two), 2000, KEPT))
    out.append(("cover 2 missed: one pair agrees behind", dict(cover=2), _around(2000, w=1000, e=1010, n=3000, s=3001), 2000, KEPT))
    out.append(("covered by the covering pair", {}, _around(2000, w=1000, e=1010, n=3000, s=3001), 1005, COVERED))
    # a valid pixel farther than an agreeing pair, but cover 0
    out.append(("cover 0", dict(cover=0), _around(2000, **two), 2000, KEPT))
    # a valid pixel nearer than its pairs stays; a pair that does not agree covers nothing
    out.append(("nearer than the pair", {}, _around(500, **two), 500, KEPT))
    out.append(("a pair that does not agree", {}, _around(5000, w=1000, e=2000), 5000, KEPT))
    # a hole whose four pairs each straddle a step of more than t stays EMPTY (property iii)
    out.append(("a hole on a step", {}, _around(0, w=1000, e=1041, n=1000, s=1041, nw=1000, se=1041, ne=1041, sw=1000), 0, EMPTY))
    out.append(("one end invalid", {}, _around(0, w=1000, n=1000, nw=1000, ne=1000), 0, EMPTY))
    return out


def border_frames():
    """[(name, frame, expected whole output)]: a pair end outside the frame on each border and corner - nothing fills there; and the
    frames of one row or one column, where only the pair along them exists"""
    out = []
    full = np.full((3, 3), 1000, np.uint16)
    for y in range(3):
        for x in range(3):
            f = full.copy()
            f[y, x] = 0
            want = f.copy()
            if (y, x) == (1, 1):
                want[1, 1] = 1000
            elif y == 1 or x == 1:
                want[y, x] = 1000                                  # an edge's middle: the pair along the edge is inside
            out.append(("hole at %d %d of 3 x 3" % (y, x), f, want))
    one = np.array([[7]], np.uint16)
    out.append(("1 x 1", one, one.copy()))
    out.append(("1 x 1 empty", np.zeros((1, 1), np.uint16), np.zeros((1, 1), np.uint16)))
    row = np.array([[1000, 0, 1010, 0, 0, 1020, 0]], np.uint16)
    out.append(("1 x N", row, np.array([[1000, 1005, 1010, 0, 0, 1020, 0]], np.uint16)))
    out.append(("N x 1", row.T.copy(), np.array([[1000, 1005, 1010, 0, 0, 1020, 0]], np.uint16).T.copy()))
    out.append(("1 x 2", np.array([[0, 9]], np.uint16), np.array([[0, 9]], np.uint16)))
    out.append(("2 x 2", np.array([[0, 9], [9, 9]], np.uint16), np.array([[0, 9], [9, 9]], np.uint16)))
    return out


# ---- seeded frames --------------------------------------------------------------------------------------------------------------------
def seeded_frame(w, h, zeros, seed, seams=True):
    """a ramp with a far wall behind it, noise within the default tol, `zeros` of the pixels invalid; with seams, holes and one-pixel slits
    (a far sample between near ones) planted on the strip (x = 7 | 8), the wave (x = 511 | 512), the block (x = 2047 | 2048) and the tile
    (rows 31 | 32) seams wherever the frame holds them"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    f = 2000 + 6 * x + 9 * y + rng.integers(-12, 13, (h, w))
    wall = rng.random((h, w)) < 0.08
    f = np.where(wall, f + 3000 + rng.integers(0, 2000, (h, w)), f)
    f = np.where(rng.random((h, w)) < zeros, 0, f)
    if seams:
        for sx in (7, 8, 511, 512, 2047, 2048):
            for sy in range(0, h, 3):
                if sx < w:
                    f[sy, sx] = 0 if (sy // 3) % 2 == 0 else 60000
        for sy in (31, 32, 63, 64):
            for sx in range(1, w, 3):
                if sy < h:
                    f[sy, sx] = 0 if (sx // 3) % 2 == 0 else 60000
    return np.clip(f, 0, 65535).astype(np.uint16)


def set_across(frames, w, h, spots):
    """the hand-made 3 x 3 frames set into one w x h frame of zeros with their centres on `spots` [(row, column)], which lie at least
    three apart in one direction, so no frame lies on another and a centre sees its own frame alone: -> (frame, [(y, x, expected output,
    expected class, name)])"""
    f = np.zeros((h, w), np.uint16)
    marks = []
    for i, (cy, cx) in enumerate(spots):
        assert 1 <= cx < w - 1 and 1 <= cy < h - 1 and all(abs(cy - y) >= 3 or abs(cx - x) >= 3 for y, x in spots[:i])
    for (name, rule, small, want, cls), (cy, cx) in zip(frames, spots):
        f[cy - 1:cy + 2, cx - 1:cx + 2] = small
        marks.append((cy, cx, want, cls, name))
    return f, marks


# ---- the accuracy recipe (tools/depth_fill_accuracy.py records it, tests/test_depth_fill.py holds the host statement to it) ---------------
APPROACH = ((50.0, 0.0, 1.0, 0.0), (50.0, 0.0, 1.0, 0.30))         # the clean frame of the first pose warped to the second: 30 cm nearer
PULLS = (0.1, 0.2, 0.4)


def accuracy_figures(ssd):
    """host statements only, warp_model's recipes unchanged, the default rule, one pass -> dict of (before, after) figures"""
    fill = lambda f, **kw: ssd.depth_fill_host(np.ascontiguousarray(f), make_rule(ssd, kw))[0]                      # noqa: E731
    W, H = wm.ACC_W, wm.ACC_H
    a = wm.accuracy_figures(ssd)
    clean, dst, warped = a["target_clean"], a["dst"], a["warped"]
    out = dict(base=a)
    # a view that magnifies: the share of all pixels that are not 0
    src = wm.scene_src(ssd, W, H)
    scene = wm.scene_frames(ssd, W, H)[0]
    out["pull"] = []
    for by in PULLS:
        w = ssd.depth_warp_host(scene, wm.pull_near_view(ssd, src, by), src)[0]
        out["pull"].append((float((w != 0).mean()), float((fill(w) != 0).mean())))
    # the approach
    near = ssd.synth_depth_host([wm.pose_scene(ssd, APPROACH[0]), wm.pose_scene(ssd, APPROACH[1])])
    adst = ssd.intrinsics_for_scene(wm.pose_scene(ssd, APPROACH[1]))
    w = ssd.depth_warp_host(near[0], wm.pose_view(ssd, APPROACH[0], APPROACH[1]), adst)[0]
    out["approach"] = dict(before=wm.against(w, near[1]), after=wm.against(fill(w), near[1]), no_cover=wm.against(fill(w, cover=0), near[1]))
    # each clean moved pose warped
    views = [wm.pose_view(ssd, p, wm.ACC_POSES[0]) for p in wm.ACC_POSES]
    moved = ssd.synth_depth_host([wm.pose_scene(ssd, p) for p in wm.ACC_POSES])
    out["clean"] = []
    for f, v in list(zip(moved, views))[1:]:
        w = ssd.depth_warp_host(f, v, dst)[0]
        out["clean"].append((wm.against(w, clean), wm.against(fill(w), clean)))
    # noisy, warped, filled and fused
    filled = np.array([fill(f) for f in warped])
    fuse = lambda fr: ssd.depth_fuse_host(np.ascontiguousarray(fr))[0]                                             # noqa: E731
    out["fused3"] = (wm.against(fuse(warped[1:4]), clean), wm.against(fuse(filled[1:4]), clean))
    out["fused5"] = (wm.against(fuse(warped), clean), wm.against(fuse(filled), clean))
    out["filled"] = filled
    # the clean target frame itself
    out["changed"] = (int((fill(clean) != clean).sum()), int(clean.size))
    return out


def accuracy_rows(a):
    """the figures as the rows of profiles/depth_fill_accuracy.txt: [(label, before cells, after cells)]"""
    pct = lambda v: "%.2f" % (100 * v)                                                                              # noqa: E731
    tri = lambda t: [pct(t[0]), "%.3f" % (100 * t[1]), "%.2f" % t[2]]                                                # noqa: E731
    rows = [("pull_near_view %.1f m: non-zero %%" % by, [pct(b)], [pct(f)]) for by, (b, f) in zip(PULLS, a["pull"])]
    ap = a["approach"]
    rows.append(("30 cm approach: valid %, far %, rms", tri(ap["before"]), tri(ap["after"])))
    rows.append(("30 cm approach, cover 0: valid %, far %, rms", tri(ap["before"]), tri(ap["no_cover"])))
    rows += [("clean pose %d warped: valid %%, far %%, rms" % (i + 1), tri(b), tri(f)) for i, (b, f) in enumerate(a["clean"])]
    rows.append(("noisy poses 1 .. 3 warped, fused n = 3: valid %, far %, rms", tri(a["fused3"][0]), tri(a["fused3"][1])))
    rows.append(("noisy poses 0 .. 4 warped, fused n = 5: valid %, far %, rms", tri(a["fused5"][0]), tri(a["fused5"][1])))
    rows.append(("clean target frame: pixels changed of %d" % a["changed"][1], ["n/a"], ["%d" % a["changed"][0]]))
    return rows
