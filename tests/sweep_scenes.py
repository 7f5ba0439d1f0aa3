"""The follow-on sweep's scene list (tests/test_sweep_scenes.py, tests/test_gpu_sweep.py): G staircases x V views as make_scene keyword
sets, a pure function of one seed.  A staircase fixes n_steps, tread, rise, stair_width, first_riser_y and yaw_deg, drawn from the
ranges of tools/fuzz.py (yaw to +-45 degrees for half of them); view v of EVERY staircase is taken by camera v - the base pose moved by
that view's jitter of +-2 degrees of pitch and roll and +-3 cm of height -, so a list has V distinct calibrations and a cameras batch
real per-frame ones; a view's seed, sigma, outlier_frac and invalid_frac are its own.  tools/fuzz.py and its random stream are not
touched: the generator here is separate.  TEST INFRASTRUCTURE; no GPU needed.

SEED and (W, H) are the choice recorded in profiles/follow_on_sweep.txt: the smallest of RESOLUTIONS at which the oracle's results over
the list meet the variety conditions of tests/test_sweep_scenes.py."""
import functools

import numpy as np

G, V = 8, 6
RESOLUTIONS = ((256, 192), (320, 240), (640, 480))
SEED = 5958
W, H = RESOLUTIONS[0]
# the ragged shapes the project's other tests use: neither point count is a multiple of 64 (a partial last cell) and no row of
# 250 vertices ends on a 16-byte boundary (the 12-byte load path); 16-bit depth wants a width that is a multiple of 4
RAGGED = {False: (250, 190), True: (252, 191)}
STEPS = (0, 1, 2, 3, 4, 5, 6, 8)              # one per staircase, dealt by the seed
OUTLIERS, INVALID = (0.0, 0.01, 0.05, 0.15), (0.0, 0.02, 0.2)


@functools.lru_cache(maxsize=None)
def _drawn(seed):
    rng = np.random.default_rng(seed)
    base = dict(cam_height=float(rng.uniform(0.7, 1.5)), pitch_deg=float(rng.uniform(35.0, 62.0)), roll_deg=float(rng.uniform(-4.0, 4.0)))
    jitter = [(0.0, 0.0, 0.0)] + [(float(rng.uniform(-2.0, 2.0)), float(rng.uniform(-2.0, 2.0)), float(rng.uniform(-0.03, 0.03))) for _ in range(V - 1)]
    steps = [int(s) for s in rng.permutation(STEPS)]
    out = []
    for g in range(G):
        stair = dict(n_steps=steps[g], first_riser_y=float(rng.uniform(0.15, 0.7)), tread=float(rng.uniform(0.12, 0.4)),
                     rise=float(rng.uniform(0.08, 0.22)), stair_width=float(rng.uniform(0.4, 1.5)),
                     yaw_deg=float(rng.uniform(-45.0, 45.0)) if rng.random() < 0.5 else float(rng.uniform(-10.0, 10.0)))
        for v in range(V):
            dp, dr, dh = jitter[v]
            out.append((g, v, dict(stair, cam_height=base["cam_height"] + dh, pitch_deg=base["pitch_deg"] + dp, roll_deg=base["roll_deg"] + dr,
                                   seed=int(rng.integers(1, 2 ** 31)), sigma=float(rng.uniform(0.0, 0.004)),
                                   outlier_frac=float(rng.choice(OUTLIERS)), invalid_frac=float(rng.choice(INVALID)))))
    return tuple(out)


def scene_list(seed=SEED):
    """-> [(staircase g, view v, make_scene keywords)] of G x V entries, staircase by staircase"""
    return [(g, v, dict(kw)) for g, v, kw in _drawn(seed)]


def camera_keywords(seed=SEED):
    """-> the pose keywords of camera v (what every staircase's view v is taken with), V entries"""
    return [{k: kw[k] for k in ("cam_height", "pitch_deg", "roll_deg")} for g, v, kw in _drawn(seed) if g == 0]


def ragged_list(seed=SEED):
    """view 1 of every staircase: the G frames that are also run at the ragged shapes"""
    return [(g, v, kw) for g, v, kw in scene_list(seed) if v == 1]


class Sweep:
    """the list's frames and the oracle's word on them, made once per (resolution, input) and shared: scenes, calibrations (one per
    view), frames (float32 vertices, or uint16 depth with the points they deproject to), the oracle's records and the FrameResults
    they stand for, and expected_labels.  Nothing here is written to after it is made."""

    def __init__(self, ssd, oracle, depth=False, shape=None, entries=None, seed=SEED, labels=True):
        import clearance_model as cm
        import oracle_binding as ob
        from test_labels import expected_labels
        self.depth = depth
        self.w, self.h = shape or (W, H)
        self.entries = entries if entries is not None else scene_list(seed)
        self.n = len(self.entries)
        self.group = [g for g, _, _ in self.entries]
        self.view = [v for _, v, _ in self.entries]
        self.kws = [kw for _, _, kw in self.entries]
        self.scenes = [ssd.make_scene(self.w, self.h, **kw) for kw in self.kws]
        self.cfg = ssd.default_config(self.w, self.h, max_frames_per_batch=max(self.n, 2))
        cams = [ssd.make_scene(self.w, self.h, n_steps=0, **kw) for kw in camera_keywords(seed)]
        self.trans = [ssd.transformation_for_scene(sc) for sc in cams]          # per view
        self.cals = [t.constants for t in self.trans]
        self.intr = ssd.intrinsics_for_scene(cams[0]) if depth else None        # the optics are every view's
        if depth:
            self.frames = list(ssd.synth_depth_host(self.scenes))
            self.pts = [ssd.deproject_host(self.intr, f) for f in self.frames]
        else:
            self.frames = list(ssd.synth_host(self.scenes))
            self.pts = self.frames
        ocfg = ob.to_oracle_config(self.cfg)
        self.records = [oracle.process(ocfg, ob.to_oracle_calibration(self.cals[v]), p)[0] for v, p in zip(self.view, self.pts)]
        self.results = [cm.result_of_oracle(ssd, r) for r in self.records]
        self.thrown = [bool(r.status & ob.ST_THROW) for r in self.records]
        self.live = [not t and r.n_steps > 0 for t, r in zip(self.thrown, self.records)]
        self.labels = [expected_labels(oracle, self.cfg, self.cals[v], r, p) for v, r, p in zip(self.view, self.records, self.pts)] if labels else []
        for a in self.frames + self.pts + self.labels:
            a.setflags(write=False)

    def cal_of(self, i):
        return self.cals[self.view[i]]

    def histogram(self):
        """the oracle's step counts: {'throw' | n_steps: frames}"""
        out = {}
        for t, r in zip(self.thrown, self.records):
            key = "throw" if t else int(r.n_steps)
            out[key] = out.get(key, 0) + 1
        return out

    def stair_maps(self, ssd):
        """one map per staircase from ssd_stair_map_from_results over its live views -> [StairMap] of G (an empty map where none is live)"""
        maps = []
        for g in range(G):
            mine = [self.results[i] for i in range(self.n) if self.group[i] == g and self.live[i]]
            maps.append(ssd.stair_map_from_results(mine)[0] if mine else ssd.StairMap())
        return maps


_SWEEPS = {}


def sweep(ssd, oracle, depth=False, ragged=False):
    """the shared Sweep of the list (ragged: of ragged_list at RAGGED[depth])"""
    key = (depth, ragged)
    if key not in _SWEEPS:
        _SWEEPS[key] = Sweep(ssd, oracle, depth, RAGGED[depth] if ragged else None, ragged_list() if ragged else None)
    return _SWEEPS[key]


def variety(sw):
    """the conditions of the issue on the oracle's results alone -> {name: holds}"""
    n = [int(r.n_steps) for r in sw.records]
    live_yaw = sum(1 for i in range(sw.n) if sw.live[i] and n[i] >= 2 and abs(sw.kws[i]["yaw_deg"]) >= 15.0)
    out = {"a thrown frame": any(sw.thrown), "a live frame with 0 steps": any(not t and k == 0 for t, k in zip(sw.thrown, n)),
           "a frame with >= 6 steps": any(not t and k >= 6 for t, k in zip(sw.thrown, n)),
           "a quarter live, >= 2 steps, |yaw| >= 15": 4 * live_yaw >= sw.n,
           "a live frame with outlier_frac 0.15": any(sw.live[i] and sw.kws[i]["outlier_frac"] == 0.15 for i in range(sw.n)),
           "a live frame with invalid_frac 0.2": any(sw.live[i] and sw.kws[i]["invalid_frac"] == 0.2 for i in range(sw.n))}
    for k in (1, 2, 3, 4):
        out["a frame with %d steps" % k] = any(not t and c == k for t, c in zip(sw.thrown, n))
    return out


# ---- rules on an edge ----------------------------------------------------------------------------------------------------------------------
# No frame of a random list puts a point exactly ON one of the rules' inequalities, so a comparison turned from >= to > (or a division
# replaced by a multiplication with the reciprocal, which differs in the last bit) changes no byte on it.  The finders below take a frame
# of the list and, by the numpy models alone, make the RULE for which one of its points lies exactly on an edge: a margin whose square
# times a side's squared length is, in doubles, the point's squared cross product; a reach likewise; a lo that is the point's distance from
# its tread's height; a cell at which v / cell and v * (1 / cell) fall into different rows.  Each returns None where the frame has none.
def _near(x, ulps=16):
    out, lo, hi = [x], x, x
    for _ in range(ulps):
        lo, hi = float(np.nextafter(lo, -np.inf)), float(np.nextafter(hi, np.inf))
        out += [lo, hi]
    return out


def _ring(quad):
    q = [float(v) for v in quad]
    ring = [(q[0], q[1]), (q[2], q[3]), (q[6], q[7]), (q[4], q[5])]
    t = [ring[i][0] * ring[(i + 1) % 4][1] - ring[(i + 1) % 4][0] * ring[i][1] for i in range(4)]
    a2 = ((t[0] + t[1]) + t[2]) + t[3]
    return ring, 1.0 if a2 > 0 else -1.0 if a2 < 0 else 0.0


def edge_margin(cfg, cal, result, pts, lo, hi, tries=400):
    """-> (margin, point): the occupant `point` of `result` lies exactly margin inside the nearest side of its surface - kept by
    c c >= margin^2 (dx^2 + dy^2), dropped by the next margin up"""
    import clearance_model as cm
    import tread_grid_model as tg
    occ = cm.occupants(cfg, cal, result, pts, (0.0, lo, hi))
    _, ex, ey, _ = tg.external(cfg, cal, pts)
    for p in np.flatnonzero(occ)[:tries]:
        ring, o = _ring(result.steps[int(occ[p]) - 1].quad)
        sides = []
        for i in range(4):
            (x0, y0), (x1, y1) = ring[i], ring[(i + 1) % 4]
            dx, dy = x1 - x0, y1 - y0
            sides.append((o * (dx * (float(ey[p]) - y0) - dy * (float(ex[p]) - x0)), dx * dx + dy * dy))
        c, l2 = min(sides, key=lambda s: s[0] / np.sqrt(s[1]))
        if not (c > 0 and l2 > 0):
            continue
        for m in _near(float(np.sqrt(c * c / l2))):
            if 0.0 < m <= 1.0 and (m * m) * l2 == c * c:
                up = float(np.nextafter(m, 2.0))
                if cm.occupants(cfg, cal, result, pts, (m, lo, hi))[p] == occ[p] and cm.occupants(cfg, cal, result, pts, (up, lo, hi))[p] != occ[p]:
                    return m, int(p)
    return None


def edge_lo(cfg, cal, result, pts, rule, tries=400):
    """-> (lo, point): the tread point `point` (under `rule`: margin, lo, hi, cell) lies exactly lo from its surface's height - in its
    slab by !(|ez - h| > lo), out of it were the comparison >="""
    import tread_grid_model as tg
    _, tread = tg.classes(cfg, cal, result, pts, rule)
    _, _, _, ez = tg.external(cfg, cal, pts)
    best = None
    for p in np.flatnonzero(tread)[:tries]:
        d = abs(float(ez[p]) - float(result.steps[int(tread[p]) - 1].height))
        if 0.0 < d < rule[1] and (best is None or d > best[0]):
            best = (d, int(p))                                         # the widest of them: the rule stays near the one it came from
    if best is not None and tg.classes(cfg, cal, result, pts, (rule[0], best[0]) + tuple(rule[2:]))[1][best[1]] == tread[best[1]]:
        return best
    return None


def edge_cell(cfg, cal, result, pts, rule, tries=4000):
    """-> (cell, point): the tread point `point`'s row is floor(v / cell), and floor(v * (1 / cell)) is another, one of them in the grid"""
    import tread_grid_model as tg
    _, tread = tg.classes(cfg, cal, result, pts, rule)
    _, ex, ey, _ = tg.external(cfg, cal, pts)
    for p in np.flatnonzero(tread)[:tries]:
        ax = tg.Axes(result.steps[int(tread[p]) - 1].quad)
        if not ax.live:
            continue
        v = float(ax.uv(np.float64(ex[p]), np.float64(ey[p]))[1])
        for k in range(1, tg.ROWS):
            cell = v / k
            if not (0.005 <= cell <= 1.0):
                continue
            a, b = np.floor(v / cell), np.floor(v * (1.0 / cell))
            if a != b and (0 <= a < tg.ROWS or 0 <= b < tg.ROWS):
                return cell, int(p)
    return None


def edge_reach(cfg, prior, stair_map, pts, rule, tries=400):
    """-> (reach, point): the riser point `point` (under `rule`: margin, band, clear, reach) lies exactly reach from its riser's plane -
    kept by c c <= reach^2 l2, dropped by the next reach down"""
    import stair_pose_model as spm
    st = stair_map.stairs
    cls = spm.classes(cfg, prior, st, pts, rule)
    _, ex, ey, _ = spm.external(cfg, prior, pts)
    for p in np.flatnonzero(cls >= spm.TREADS)[:tries]:
        q = [float(v) for v in st.steps[int(cls[p]) - spm.TREADS + 1].quad]
        dx, dy = q[2] - q[0], q[3] - q[1]
        l2 = dx * dx + dy * dy
        a, b = float(ex[p]) - q[0], float(ey[p]) - q[1]
        c = b * dx - a * dy
        if not (l2 > 0 and c != 0):
            continue
        for m in _near(float(np.sqrt(c * c / l2))):
            if 0.0 < m <= rule[3] and (m * m) * l2 == c * c:
                down = float(np.nextafter(m, 0.0))
                if spm.classes(cfg, prior, st, pts, tuple(rule[:3]) + (m,))[p] == cls[p] and spm.classes(cfg, prior, st, pts, tuple(rule[:3]) + (down,))[p] != cls[p]:
                    return m, int(p)
    return None


def first_edge(sw, find):
    """find(frame index) over the sweep's live frames in list order -> (frame index, what it found), the first that finds something"""
    for i in range(sw.n):
        if sw.live[i]:
            got = find(i)
            if got is not None:
                return i, got
    raise AssertionError("no frame of the list reaches the edge")
