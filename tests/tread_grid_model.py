"""The tread grid rule restated for the tests (include/ssd_hip.h) in numpy, on a result and a calibration: the
class of every point (occupant / tread point of which surface), its cell in the surface's own frame, the three planes per surface, and
the solve - cell states and the best free rectangle by brute force over every rectangle of the grid.
TEST INFRASTRUCTURE; no GPU needed.  Written from the rule's text, vectorised over the points: it shares no structure with the C text.
Builds on clearance_model.world, inside_shrunk and occupants."""
import ctypes as C
import os

import numpy as np

import clearance_model as cm
import ground_model

COLS, ROWS = 32, 8
OUT, FREE, OCCUPIED, UNSEEN = 0, 1, 2, 3
RULE = cm.RULE + (0.04,)                       # margin, lo, hi, cell
WIDE_RULE = cm.WIDE_RULE + (0.02,)             # the full-width frames' (their treads are 0.6 m wide)

# the recipe under the oracle (tools/tread_grid_accuracy.py writes what it gives to profiles/tread_grid_accuracy.txt): the 3-step scene at
# sigma 1 mm, 256 x 192.  A tread holds 3000 - 4500 points, so a cell of 4 cm holds some 50 and the grid (1.28 x 0.32 m) the whole tread
# (0.8 x 0.28 m); a support of 3 keeps single stray points from deciding a cell either way
RECIPE_CELL, RECIPE_MIN_SEEN, RECIPE_MIN_OCC = 0.04, 3, 3
ACCURACY_FILE = os.path.join(ground_model.ROOT, "profiles", "tread_grid_accuracy.txt")


def rule_of(ssd, rule):
    return ssd.TreadGridRule(*rule)


def external(cfg, cal, xyz):
    """float32 camera points -> (valid-and-in-range mask, ex, ey, ez)"""
    ok, wx, wy, wz = cm.world(cfg, cal, xyz)
    r2, t2 = [float(v) for v in cal.r2], [float(v) for v in cal.t2]
    with np.errstate(invalid="ignore", over="ignore"):
        return ok, (r2[0] * wx + r2[1] * wy) + t2[0], (r2[2] * wx + r2[3] * wy) + t2[1], wz + float(cal.world_z)


def classes(cfg, cal, result, xyz, rule):
    """-> (occupant mask, tread mask): uint8 per point, k + 1 on an occupant / a tread point of surface k, 0 elsewhere"""
    margin, lo, hi, _ = rule
    occ = cm.occupants(cfg, cal, result, xyz, rule[:3])
    tread = np.zeros(len(occ), dtype=np.uint8)
    n = int(result.n_steps)
    if (int(result.status) & 1) or n == 0:
        return occ, tread
    ok, ex, ey, ez = external(cfg, cal, xyz)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in reversed(range(n)):                                   # the lowest index wins: written last
            h = float(result.steps[k].height)
            quad = [float(v) for v in result.steps[k].quad]
            take = ok & (occ == 0) & ~(np.abs(ez - h) > lo) & cm.inside_shrunk(quad, margin, ex, ey)
            tread[take] = k + 1
    return occ, tread


class Axes:
    """a surface's own frame: FL, the front edge FL -> FR, its length, the ring's orientation, the least u of the corners"""

    def __init__(self, quad):
        q = [float(v) for v in quad]
        ring = [(q[0], q[1]), (q[2], q[3]), (q[6], q[7]), (q[4], q[5])]
        t = [ring[i][0] * ring[(i + 1) % 4][1] - ring[(i + 1) % 4][0] * ring[i][1] for i in range(4)]
        a2 = ((t[0] + t[1]) + t[2]) + t[3]
        self.o = 1.0 if a2 > 0 else -1.0 if a2 < 0 else 0.0
        self.x0, self.y0 = ring[0]
        self.dx, self.dy = ring[1][0] - ring[0][0], ring[1][1] - ring[0][1]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            self.len = float(np.sqrt(np.float64(self.dx * self.dx + self.dy * self.dy)))
            self.live = self.o != 0.0 and self.len > 0.0
            self.u0 = 0.0
            for x, y in ring[1:]:
                ui = float(self.uv(np.float64(x), np.float64(y))[0])
                if ui < self.u0:
                    self.u0 = ui

    def uv(self, ex, ey):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ax, ay = ex - self.x0, ey - self.y0
            return (self.dx * ax + self.dy * ay) / np.float64(self.len), (self.o * (self.dx * ay - self.dy * ax)) / np.float64(self.len)

    def cells(self, ex, ey, cell):
        """-> (in the grid, row, column) per point; row and column are meaningful where `in` holds"""
        u, v = self.uv(ex, ey)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            c, r = np.floor((u - self.u0) / cell), np.floor(v / cell)
            inside = (c >= 0) & (c < COLS) & (r >= 0) & (r < ROWS)
        if not self.live:
            inside = np.zeros(np.shape(inside), dtype=bool)
        return inside, np.where(inside, r, 0).astype(np.int64), np.where(inside, c, 0).astype(np.int64)

    def world(self, row, col, cell):
        """grid coordinates in cells (a cell's centre: row + .5, col + .5) -> external world x, y"""
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            a, b = (self.u0 + col * cell) / np.float64(self.len), (row * cell) / np.float64(self.len)
            return (self.x0 + a * self.dx) + b * (self.o * -self.dy), (self.y0 + a * self.dy) + b * (self.o * self.dx)


def grids(cfg, cal, result, xyz, rule):
    """-> per surface k < MAX_STEPS a dict: seen, occ, top [ROWS, COLS] and n_seen_out, n_occ_out, top_out, as Python / numpy ints"""
    occ, tread = classes(cfg, cal, result, xyz, rule)
    _, ex, ey, ez = external(cfg, cal, xyz)
    out = []
    for k in range(len(result.steps)):
        g = dict(seen=np.zeros((ROWS, COLS), np.int64), occ=np.zeros((ROWS, COLS), np.int64), top=np.zeros((ROWS, COLS), np.int64),
                 n_seen_out=0, n_occ_out=0, top_out=0)
        mine_t, mine_o = tread == k + 1, occ == k + 1
        if mine_t.any() or mine_o.any():
            ax = Axes(result.steps[k].quad)
            inside, r, c = ax.cells(ex, ey, rule[3])
            np.add.at(g["seen"], (r[mine_t & inside], c[mine_t & inside]), 1)
            g["n_seen_out"] = int(np.count_nonzero(mine_t & ~inside))
            np.add.at(g["occ"], (r[mine_o & inside], c[mine_o & inside]), 1)
            g["n_occ_out"] = int(np.count_nonzero(mine_o & ~inside))
            units = np.rint((ez - float(result.steps[k].height)) * 65536.0)
            np.maximum.at(g["top"], (r[mine_o & inside], c[mine_o & inside]), units[mine_o & inside].astype(np.int64))
            far = units[mine_o & ~inside]
            g["top_out"] = int(max(0, far.max())) if len(far) else 0
        out.append(g)
    return out


def grid_of_record(rec, k):
    """surface k of a FrameTreadGrid in the form of grids()"""
    s = rec.s[k]
    return dict(seen=np.ctypeslib.as_array(s.seen).astype(np.int64), occ=np.ctypeslib.as_array(s.occ).astype(np.int64),
                top=np.ctypeslib.as_array(s.top).astype(np.int64), n_seen_out=int(s.n_seen_out), n_occ_out=int(s.n_occ_out), top_out=int(s.top_out))


def same_grid(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ("seen", "occ", "top")) and all(a[f] == b[f] for f in ("n_seen_out", "n_occ_out", "top_out"))


def assert_record(ssd, rec, want, n_surfaces, ground):
    """a FrameTreadGrid against grids(), cell by cell, and its header; surfaces at k >= n_surfaces hold nothing"""
    assert (rec.n_surfaces, rec.ground, C.sizeof(rec)) == (n_surfaces, ground, 8 + ssd.MAX_STEPS * 3088)
    for k in range(ssd.MAX_STEPS):
        got = grid_of_record(rec, k)
        assert same_grid(got, want[k]), (k, {f: (got[f], want[k][f]) for f in got if not np.array_equal(got[f], want[k][f])})
        assert rec.s[k].reserved == 0


def record_of(ssd, per_surface, n_surfaces, ground=1):
    """a FrameTreadGrid of hand-made planes: per_surface = [dict(seen=, occ=, top=, n_seen_out=, ...)] with any field left out"""
    rec = ssd.FrameTreadGrid()
    rec.n_surfaces, rec.ground = n_surfaces, ground
    for k, g in enumerate(per_surface):
        for f in ("seen", "occ", "top"):
            if f in g:
                np.ctypeslib.as_array(getattr(rec.s[k], f))[:] = np.asarray(g[f])
        for f in ("n_seen_out", "n_occ_out", "top_out"):
            setattr(rec.s[k], f, int(g.get(f, 0)))
    return rec


# ---- the solve ----

def states(g, quad, rule, min_seen, min_occ):
    """[ROWS, COLS] of OUT / FREE / OCCUPIED / UNSEEN for one surface's grid"""
    ax = Axes(quad)
    r, c = np.meshgrid(np.arange(ROWS) + 0.5, np.arange(COLS) + 0.5, indexing="ij")
    x, y = ax.world(r, c, rule[3])
    inside = cm.inside_shrunk([float(v) for v in quad], rule[0], x.reshape(-1), y.reshape(-1)).reshape(ROWS, COLS) & ax.live
    st = np.full((ROWS, COLS), UNSEEN, dtype=np.uint8)
    st[g["seen"] >= max(min_seen, 1)] = FREE
    st[g["occ"] >= max(min_occ, 1)] = OCCUPIED
    st[~inside] = OUT
    return st


def best_rectangle(st, need_cols=1, need_rows=1):
    """every rectangle of the grid: the all-FREE one of the largest area with at least need_cols x need_rows cells; ties: the smallest
    row0, then the smallest col0, then the most cols -> (col0, row0, cols, rows) or None"""
    best = None
    free = st == FREE
    for r0 in range(ROWS):
        for rows in range(1, ROWS - r0 + 1):
            for c0 in range(COLS):
                for cols in range(1, COLS - c0 + 1):
                    if not free[r0:r0 + rows, c0:c0 + cols].all():
                        break                                           # wider ones hold the same cell
                    if cols < need_cols or rows < need_rows:
                        continue
                    key = (-cols * rows, r0, c0, -cols)
                    if best is None or key < best[0]:
                        best = (key, (c0, r0, cols, rows))
    return None if best is None else best[1]


def solve(g, quad, rule, min_seen=1, min_occ=1, foot_along=0.0, foot_deep=0.0):
    """one surface -> dict(state, n_free, n_occupied, n_unseen, tallest, foothold, rect (col0, row0, cols, rows), centre, size)"""
    st = states(g, quad, rule, min_seen, min_occ)
    cell = rule[3]
    rect = best_rectangle(st, max(int(np.ceil(foot_along / cell)), 1), max(int(np.ceil(foot_deep / cell)), 1))
    out = dict(state=st, n_free=int(np.count_nonzero(st == FREE)), n_occupied=int(np.count_nonzero(st == OCCUPIED)),
               n_unseen=int(np.count_nonzero(st == UNSEEN)), tallest=max(int(g["top"].max()), int(g["top_out"])) / 65536.0,
               foothold=0 if rect is None else 1, rect=rect or (0, 0, 0, 0), centre=(0.0, 0.0), size=(0.0, 0.0))
    if rect:
        c0, r0, cols, rows = rect
        x, y = Axes(quad).world(r0 + rows / 2.0, c0 + cols / 2.0, cell)
        out["centre"], out["size"] = (float(x), float(y)), (cols * cell, rows * cell)
    return out


def assert_solved(f, want):
    """an ssd.Foothold against solve()"""
    assert np.array_equal(np.ctypeslib.as_array(f.state), want["state"])
    assert (f.n_free, f.n_occupied, f.n_unseen, f.foothold) == (want["n_free"], want["n_occupied"], want["n_unseen"], want["foothold"])
    assert (f.col0, f.row0, f.cols, f.rows) == tuple(want["rect"]), ((f.col0, f.row0, f.cols, f.rows), want["rect"])
    assert f.tallest == want["tallest"]
    assert np.allclose(list(f.centre), want["centre"], rtol=0, atol=1e-9) and np.allclose(list(f.size), want["size"], rtol=0, atol=1e-12)


# ---- the recipe under the oracle (tests/test_tread_grid.py holds the host functions to it, tools/tread_grid_accuracy.py records it) ----

def recipe(ssd, oracle, sigma=0.001, seed=7, surface=1):
    """the 3-step scene, clean and with cm.patched on `surface`, each under its OWN oracle result, through the model alone ->
    dict(clean=, patched= [per surface solve()], grids_patched=, pulled_cells / vacated_cells = boolean [ROWS, COLS] on `surface`,
    fr=, fr2=, frames=)"""
    import oracle_binding as ob
    from test_labels import expected_labels
    rule = cm.RULE + (RECIPE_CELL,)
    cfg, trans, frame = cm.scene_frame(ssd, sigma, seed)
    cal = trans.constants
    ocfg, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal)
    res = oracle.process(ocfg, ocal, frame)[0]
    fr = cm.result_of_oracle(ssd, res)
    f2, sel = cm.patched(cfg, cal, fr, frame, expected_labels(oracle, cfg, cal, res, frame), surface)
    fr2 = cm.result_of_oracle(ssd, oracle.process(ocfg, ocal, f2)[0])
    out = dict(fr=fr, fr2=fr2, frames=(frame, f2), cfg=cfg, cal=cal, rule=rule, sel=sel)
    for key, f, r in (("clean", frame, fr), ("patched", f2, fr2)):
        g = grids(cfg, cal, r, f, rule)
        out["grids_" + key] = g
        out[key] = [solve(g[k], r.steps[k].quad, rule, RECIPE_MIN_SEEN, RECIPE_MIN_OCC) for k in range(r.n_steps)]
    ax = Axes(fr2.steps[surface].quad)
    for key, f in (("pulled_cells", f2), ("vacated_cells", frame)):
        _, ex, ey, _ = external(cfg, cal, np.asarray(f).reshape(-1, 3)[sel.reshape(-1)])
        inside, r, c = ax.cells(ex, ey, RECIPE_CELL)
        m = np.zeros((ROWS, COLS), dtype=bool)
        m[r[inside], c[inside]] = True
        out[key] = m
    return out
