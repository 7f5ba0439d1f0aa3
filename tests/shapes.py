"""Hand-built clouds whose plateaus are NOT rectangles (test_shapes.py, test_gpu_shapes.py), as clouds.py builds blocks.

The staircase generator, clouds.py and the fuzzers all give k_outline / k_final rectangles in the top-down image: both halves
of the outline alike, long edge lists, four corners from intersections, a ground whose front edge spans the image.  Here a
surface is a vectorised predicate mask(x, y) over world coordinates (metres; the default measuring range x -0.6 .. 0.6,
y 0.1 .. 1.3, image column = (x + 0.6) W / 1.2, image row = (1.3 - y) H / 1.2, scan columns at W/2 + 25 j) and a height.

CATALOGUE names every shape with the branch it was built for; SIGNATURES (below it) is what the oracle records for it at
640 x 480 with the identity calibration of clouds.py - test_shapes.py asserts it, the GPU tests assert it before they compare.
"""
import numpy as np

import clouds

X_MIN, X_MAX, Y_MIN, Y_MAX = -0.6, 0.6, 0.1, 1.3          # ssd.default_config's measuring range
Z_GROUND, Z_STEP = 0.005, 0.1755                          # height bins 10 (below minHeight = 15) and 27


def grid_points(width, height, mask, z, sub=1):
    """the points of one surface: a grid of `sub` x `sub` points per pixel of the top-down image, centred in the pixels (so that
    no pixel whose centre the mask holds stays unlit, and no float32 rounding moves a point across a pixel's border)"""
    nx, ny = width * sub, height * sub
    x = X_MIN + (np.arange(nx) + 0.5) * ((X_MAX - X_MIN) / nx)
    y = Y_MAX - (np.arange(ny) + 0.5) * ((Y_MAX - Y_MIN) / ny)
    gx, gy = np.meshgrid(x, y)
    m = np.asarray(mask(gx, gy), dtype=bool)
    return np.stack([gx[m], gy[m], np.full(int(m.sum()), float(z))], 1)


def shape_cloud(width, height, parts, seed=0, z_shift=clouds.Z_SHIFT, extra=None, sub=1):
    """parts: list of (mask, z) -> float32 camera frame [height, width, 3] for clouds.calibration(ssd, z_shift); the points land
    on the frame's pixels the way clouds.cloud places them.  extra: further world points (x, y, z)."""
    pts = [grid_points(width, height, mask, z, sub) for mask, z in parts]
    if extra is not None and len(extra):
        pts.append(np.asarray(extra, dtype=np.float64).reshape(-1, 3))
    p = np.concatenate(pts) if pts else np.zeros((0, 3))
    if len(p) > width * height:
        raise ValueError("shape_cloud: %d points do not fit a frame of %d x %d" % (len(p), width, height))
    return clouds.cloud([], width, height, extra=p, seed=seed, z_shift=z_shift)


def pixel_point(width, height, col, row, z):
    """the world point at the centre of top-down pixel (col, row)"""
    return [X_MIN + (col + 0.5) * (X_MAX - X_MIN) / width, Y_MAX - (row + 0.5) * (Y_MAX - Y_MIN) / height, z]


# ---- masks
def rect(x0, x1, y0, y1):
    return lambda x, y: (x > x0) & (x < x1) & (y > y0) & (y < y1)


def _saw(x):
    t = (x + 0.4) / 0.16
    return t - np.floor(t)


SHAPES = {
    "rect": rect(-0.4, 0.4, 0.55, 1.05),                                          # the control
    "rect_left": rect(-0.55, 0.03, 0.55, 1.05),                                   # scansLeft.size() >= half
    "rect_right": rect(-0.03, 0.55, 0.55, 1.05),                                  # scansRight.size() > half, no left scan
    "rect_right_5": rect(-0.01, 0.2, 0.55, 1.05),                                 # five right scans, none left
    "cols2": rect(-0.06, 0.02, 0.55, 1.05),                                       # two scan columns: no outline
    "cols3": rect(-0.06, 0.06, 0.55, 1.05),                                       # edge lists of 2
    "cols4": rect(-0.06, 0.10, 0.55, 1.05),                                       # 2 left, 3 right
    "cols5": rect(-0.10, 0.10, 0.55, 1.05),                                       # lists of 3
    "cols7": rect(-0.15, 0.15, 0.55, 1.05),                                       # lists of 4
    # the centre column finds nothing deep enough: no scans at all on a large plateau
    "slot": lambda x, y: rect(-0.5, 0.5, 0.55, 1.05)(x, y) & (np.abs(x) > 0.012),
    "bow_tie": lambda x, y: (np.abs(x) < 0.5) & (np.abs(y - 0.8) < 0.6 * np.abs(x)),
    "thin_strip": lambda x, y: (rect(-0.5, 0.5, 0.55, 1.05)(x, y) & (np.abs(x) > 0.03)) | ((np.abs(x) < 0.04) & (np.abs(y - 0.8) < 0.03)),
    "triangle_near": lambda x, y: (y > 0.55) & (y < 1.1 - 1.375 * np.abs(x)),     # base near the camera
    "triangle_far": lambda x, y: (y < 1.1) & (y > 0.55 + 1.375 * np.abs(x)),      # base far
    "trapezoid_near": lambda x, y: (y > 0.55) & (y < 1.05) & (np.abs(x) < 0.5 - 0.7 * (y - 0.55)),
    "trapezoid_far": lambda x, y: (y > 0.55) & (y < 1.05) & (np.abs(x) < 0.15 + 0.7 * (y - 0.55)),
    "lens": lambda x, y: np.abs(y - 0.8) < 0.35 - 1.2 * x * x,
    "diamond": lambda x, y: np.abs(x) / 0.45 + np.abs(y - 0.8) / 0.35 < 1.0,
    "rect45": lambda x, y: (np.abs(x + (y - 0.8)) * 0.7071 < 0.3) & (np.abs(x - (y - 0.8)) * 0.7071 < 0.18),
    "chevron_far": lambda x, y: (np.abs(x) < 0.4) & (np.abs(y - 0.65 - 0.8 * np.abs(x)) < 0.12),     # a V, its point towards the camera
    "chevron_near": lambda x, y: (np.abs(x) < 0.4) & (np.abs(y - 1.0 + 0.8 * np.abs(x)) < 0.12),
    "chevron_unequal": lambda x, y: (x > -0.45) & (x < 0.2) & (np.abs(y - 0.6 - np.where(x < 0, -0.9 * x, 1.4 * x)) < 0.11),
    "dart": lambda x, y: (y < 1.15 - 1.2 * np.abs(x)) & (y > 0.5 + 0.5 * (0.45 - np.abs(x))) & (np.abs(x) < 0.45),
    # a rectangle with a triangular notch beside one end: an outline whose quadrilateral is NOT convex (found by a random search
    # over darts, chevrons, notches and L shapes; the darts and chevrons all came out convex)
    "notch_front": lambda x, y: rect(-0.45, 0.45, 0.55, 1.1)(x, y) & ~((np.abs(x + 0.316) < 0.24) & (y < 0.55 + 0.388 * (1 - np.abs(x + 0.316) / 0.24))),
    "notch_back": lambda x, y: rect(-0.45, 0.45, 0.55, 1.1)(x, y) & ~((np.abs(x - 0.185) < 0.168) & (y > 1.1 - 0.431 * (1 - np.abs(x - 0.185) / 0.168))),
    "parallelogram": lambda x, y: (np.abs(x) < 0.25) & (np.abs(y - 0.8 - 1.2 * x) < 0.15),
    "sawtooth_back": lambda x, y: (np.abs(x) < 0.4) & (y > 0.55) & (y < 0.9 + 0.2 * _saw(x)),
    # for the widths with a scan column on an image border (650: column 0, 651: column W - 1)
    "full": lambda x, y: y > 0.32,
    "left_edge_touch": rect(-0.7, 0.1, 0.55, 1.05),
    "right_edge_touch": rect(-0.1, 0.7, 0.55, 1.05),
    "behind": rect(-0.4, 0.4, 1.0, 1.25),                                         # a step behind a ground in the far half
    "cols3_wide": rect(-0.03, 0.03, 0.55, 1.05),                                  # three scan columns at 1280 pixels
}

GROUNDS = {
    "ground": rect(-0.55, 0.55, 0.15, 0.45),
    "ground_low": rect(-0.55, 0.55, 0.12, 0.30),                                  # in front of "full"
    "ground_left": rect(-0.30, -0.05, 0.15, 0.45),                                # bottomScan's second loop
    "ground_right": rect(0.05, 0.30, 0.15, 0.45),
    "ground_one_column": rect(-0.03, 0.03, 0.12, 0.48),                           # one front-edge point: no front edge
    "ground_far_half": rect(-0.55, 0.55, 0.75, 0.95),                             # nothing in the near half of the image
    "ground_gap": lambda x, y: rect(-0.30, 0.30, 0.15, 0.45)(x, y) & (np.abs(x) > 0.05),
}

# name -> (ground, shape): every shape over the plain ground, then the six ground variants under a rectangle
CATALOGUE = {name: ("ground_low" if name == "full" else "ground", name) for name in SHAPES if name not in ("behind", "cols3_wide")}
CATALOGUE.update({
    "g_left": ("ground_left", "rect"),
    "g_right": ("ground_right", "rect"),
    "g_one_column": ("ground_one_column", "rect"),
    "g_far_half": ("ground_far_half", "behind"),
    "g_gap": ("ground_gap", "rect"),
    "g_low": ("ground_low", "rect"),
})
NAMES = list(CATALOGUE)                                                            # the 640 x 480 cases
WIDE = ["rect_left", "triangle_near", "lens", "diamond", "cols3_wide", "g_left"]  # the cases of the 1280 x 720 test
_PAIRS = dict(CATALOGUE, cols3_wide=("ground", "cols3_wide"))


def parts_of(name, z_step=Z_STEP):
    g, s = _PAIRS[name]
    return [(GROUNDS[g], Z_GROUND), (SHAPES[s], z_step)]


def frame(name, width=640, height=480, seed=0, z_shift=clouds.Z_SHIFT, extra=None):
    return shape_cloud(width, height, parts_of(name), seed=seed, z_shift=z_shift, extra=extra)


# ---- signatures
def signature(res):
    """what the branches of k_outline / k_final leave in a record, of the frame's first step plateau and its ground"""
    steps = [res.plateaus[k] for k in range(res.n_plateaus) if res.plateaus[k].is_step]
    sig = dict(n_steps=res.n_steps, ground_n_pts=res.ground_n_pts, ground_front_valid=res.ground_front_valid)
    if steps:
        p = steps[0]
        sig.update(scans=(p.n_scans_right, p.n_scans_left), outline_found=p.outline_found, valid=p.valid)
        if p.outline_found:
            sig.update(n_edge_pts=list(p.n_edge_pts), n_vpts=list(p.n_vpts), vedge_found=list(p.vedge_found),
                       corner_found=list(p.corner_found))
    return sig


def classes(res):
    """the branch classes a frame's record reaches (the coverage table's rows)"""
    out = set()
    for k in range(res.n_plateaus):
        p = res.plateaus[k]
        if not p.is_step:
            continue
        r, l = p.n_scans_right, p.n_scans_left
        if r == 0:
            out.add("scans: none")
            continue
        if r + l < 3:
            out.add("scans: fewer than three")
            continue
        half = (r + l) // 2 + 1
        out.add("obtainLinePoints: " + ("left >= half" if l >= half else "right > half" if r > half else "neither"))
        if l == 0:
            out.add("obtainLinePoints: no left scan")
        for n in p.n_edge_pts:
            out.add("edge list: " + ("2" if n <= 2 else "3-6" if n <= 6 else "> 6"))
        out.add("corner_found: %s" % list(p.corner_found))
        out.add("vedge_found: %s" % list(p.vedge_found))
        out.add("quadrilateral: " + ("convex" if p.valid else "not convex"))
    if res.first_valid_ind >= 0 and res.ground_ind >= 0:
        n = res.ground_n_pts
        out.add("ground points: " + ("0" if n == 0 else "1" if n == 1 else "2-3" if n <= 3 else "> 3"))
    return out


def edge_lists(p):
    """obtainLinePoints (segmentation.cpp:129-156) restated on a record's scans -> the four BestLine inputs in the record's
    order (front left, front right, back left, back right) as lists of (x, y)"""
    sr = [tuple(s) for s in p.scans_right[:p.n_scans_right]]
    sl = [tuple(s) for s in p.scans_left[:p.n_scans_left]]
    half = (len(sr) + len(sl)) // 2 + 1
    left, right = [], []
    il = ir = 0
    if len(sl) >= half:
        il = len(sl) - half
        right += [sl[i] for i in range(il, -1, -1)]
    else:
        if len(sr) > half:
            ir = len(sr) - half
        left += [sr[i] for i in range(ir, -1, -1)]
    right += sr[ir:]
    left += sl[il:]
    front = lambda scans: [(s[0], s[2]) for s in scans]
    back = lambda scans: [(s[0], s[1]) for s in scans]
    return [front(left), front(right), back(left), back(right)]


# ---- recorded signatures (the oracle's record of each case; asserted, never derived from the HIP path)
SIGNATURES = {
    "rect": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=9, ground_front_valid=1, n_steps=2),
    "rect_left": dict(scans=(1, 11), n_edge_pts=[7, 6, 7, 6], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=6, ground_front_valid=1, n_steps=2),
    "rect_right": dict(scans=(12, 0), n_edge_pts=[6, 7, 6, 7], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=6, ground_front_valid=1, n_steps=2),
    "rect_right_5": dict(scans=(5, 0), n_edge_pts=[3, 3, 3, 3], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=3, ground_front_valid=1, n_steps=2),
    "cols2": dict(scans=(1, 1), outline_found=0, valid=0, ground_n_pts=0, ground_front_valid=0, n_steps=0),
    "cols3": dict(scans=(2, 1), n_edge_pts=[2, 2, 2, 2], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=1, ground_front_valid=0, n_steps=2),
    "cols4": dict(scans=(3, 1), n_edge_pts=[2, 3, 2, 3], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=2, ground_front_valid=1, n_steps=2),
    "cols5": dict(scans=(3, 2), n_edge_pts=[3, 3, 3, 3], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=3, ground_front_valid=1, n_steps=2),
    "cols7": dict(scans=(4, 3), n_edge_pts=[4, 4, 4, 4], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=3, ground_front_valid=1, n_steps=2),
    "slot": dict(scans=(0, 0), outline_found=0, valid=0, ground_n_pts=0, ground_front_valid=0, n_steps=0),
    "bow_tie": dict(scans=(0, 0), outline_found=0, valid=0, ground_n_pts=0, ground_front_valid=0, n_steps=0),
    "thin_strip": dict(scans=(0, 0), outline_found=0, valid=0, ground_n_pts=0, ground_front_valid=0, n_steps=0),
    "triangle_near": dict(scans=(7, 6), n_edge_pts=[7, 7, 7, 7], n_vpts=[5, 5], vedge_found=[1, 1], corner_found=[1, 1, 0, 0], outline_found=1, valid=1, ground_n_pts=7, ground_front_valid=1, n_steps=2),
    "triangle_far": dict(scans=(7, 6), n_edge_pts=[7, 7, 7, 7], n_vpts=[5, 5], vedge_found=[1, 1], corner_found=[0, 0, 1, 1], outline_found=1, valid=1, ground_n_pts=7, ground_front_valid=1, n_steps=2),
    "trapezoid_near": dict(scans=(10, 9), n_edge_pts=[10, 10, 10, 10], n_vpts=[3, 3], vedge_found=[1, 1], corner_found=[1, 1, 0, 0], outline_found=1, valid=1, ground_n_pts=10, ground_front_valid=1, n_steps=2),
    "trapezoid_far": dict(scans=(10, 9), n_edge_pts=[10, 10, 10, 10], n_vpts=[3, 3], vedge_found=[1, 1], corner_found=[0, 0, 1, 1], outline_found=1, valid=1, ground_n_pts=9, ground_front_valid=1, n_steps=2),
    "lens": dict(scans=(11, 10), n_edge_pts=[11, 11, 11, 11], n_vpts=[14, 6], vedge_found=[1, 1], corner_found=[1, 0, 1, 0], outline_found=1, valid=1, ground_n_pts=10, ground_front_valid=1, n_steps=2),
    "diamond": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[3, 3], vedge_found=[1, 1], corner_found=[0, 0, 0, 0], outline_found=1, valid=1, ground_n_pts=9, ground_front_valid=1, n_steps=2),
    "rect45": dict(scans=(7, 6), n_edge_pts=[7, 7, 7, 7], n_vpts=[3, 3], vedge_found=[1, 1], corner_found=[0, 0, 0, 0], outline_found=1, valid=1, ground_n_pts=9, ground_front_valid=1, n_steps=2),
    "chevron_far": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[8, 8], vedge_found=[1, 1], corner_found=[0, 0, 0, 0], outline_found=1, valid=1, ground_n_pts=8, ground_front_valid=1, n_steps=2),
    "chevron_near": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[8, 8], vedge_found=[1, 1], corner_found=[0, 0, 0, 0], outline_found=1, valid=1, ground_n_pts=8, ground_front_valid=1, n_steps=2),
    "chevron_unequal": dict(scans=(5, 9), n_edge_pts=[8, 7, 8, 7], n_vpts=[7, 7], vedge_found=[1, 1], corner_found=[0, 0, 0, 0], outline_found=1, valid=1, ground_n_pts=7, ground_front_valid=1, n_steps=2),
    "dart": dict(scans=(10, 9), n_edge_pts=[10, 10, 10, 10], n_vpts=[4, 4], vedge_found=[1, 1], corner_found=[1, 1, 0, 0], outline_found=1, valid=1, ground_n_pts=9, ground_front_valid=1, n_steps=2),
    "notch_front": dict(scans=(10, 9), n_edge_pts=[10, 10, 10, 10], n_vpts=[7, 20], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=0, ground_n_pts=0, ground_front_valid=0, n_steps=0),
    "notch_back": dict(scans=(10, 9), n_edge_pts=[10, 10, 10, 10], n_vpts=[20, 4], vedge_found=[1, 1], corner_found=[1, 1, 1, 0], outline_found=1, valid=0, ground_n_pts=0, ground_front_valid=0, n_steps=0),
    "parallelogram": dict(scans=(6, 5), n_edge_pts=[6, 6, 6, 6], n_vpts=[10, 10], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=8, ground_front_valid=1, n_steps=2),
    "sawtooth_back": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[14, 19], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=9, ground_front_valid=1, n_steps=2),
    "full": dict(scans=(13, 12), n_edge_pts=[13, 13, 13, 13], n_vpts=[38, 38], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=11, ground_front_valid=1, n_steps=2),
    "left_edge_touch": dict(scans=(3, 12), n_edge_pts=[8, 8, 8, 8], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=7, ground_front_valid=1, n_steps=2),
    "right_edge_touch": dict(scans=(13, 2), n_edge_pts=[8, 8, 8, 8], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=7, ground_front_valid=1, n_steps=2),
    "g_left": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=3, ground_front_valid=1, n_steps=2),
    "g_right": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=3, ground_front_valid=1, n_steps=2),
    "g_one_column": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=1, ground_front_valid=0, n_steps=2),
    "g_far_half": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[8, 8], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=0, ground_front_valid=0, n_steps=2),
    "g_gap": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=3, ground_front_valid=1, n_steps=2),
    "g_low": dict(scans=(9, 8), n_edge_pts=[9, 9, 9, 9], n_vpts=[18, 18], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=9, ground_front_valid=1, n_steps=2),
}
WIDE_SIGNATURES = {
    "rect_left": dict(scans=(2, 23), n_edge_pts=[13, 13, 13, 13], n_vpts=[28, 28], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=12, ground_front_valid=1, n_steps=2),
    "triangle_near": dict(scans=(14, 13), n_edge_pts=[14, 14, 14, 14], n_vpts=[6, 6], vedge_found=[1, 1], corner_found=[1, 1, 0, 0], outline_found=1, valid=1, ground_n_pts=14, ground_front_valid=1, n_steps=2),
    "lens": dict(scans=(22, 21), n_edge_pts=[22, 22, 22, 22], n_vpts=[13, 10], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=21, ground_front_valid=1, n_steps=2),
    "diamond": dict(scans=(17, 16), n_edge_pts=[17, 17, 17, 17], n_vpts=[5, 5], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=17, ground_front_valid=1, n_steps=2),
    "cols3_wide": dict(scans=(2, 1), n_edge_pts=[2, 2, 2, 2], n_vpts=[28, 28], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=1, ground_front_valid=0, n_steps=2),
    "g_left": dict(scans=(18, 17), n_edge_pts=[18, 18, 18, 18], n_vpts=[28, 28], vedge_found=[1, 1], corner_found=[1, 1, 1, 1], outline_found=1, valid=1, ground_n_pts=5, ground_front_valid=1, n_steps=2),
}
