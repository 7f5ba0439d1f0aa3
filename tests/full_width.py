"""Hand-built frames at the full width of the per-surface and per-riser passes: ground plus 16 step plateaus (SSD_MAX_STEPS = 17
surfaces) and the 16 vertical faces between them (SSD_MAX_RISERS), in pixel layouts that decide what a wave of k_surface_moments,
k_surface_refit and k_riser_moments meets in a point slot.  TEST INFRASTRUCTURE; no GPU needed (tests/test_full_width.py holds the
recipe to its figures under the oracle, tests/test_gpu_full_width.py runs the kernels on the frames).

The calibration is tests/clouds.py's: identity rotation, the camera `z_shift` below the world origin.  Every plane lies on a grid with
one column per pixel column of the top-down image and gets 1.3 times the pixels its rectangle covers there, so that it rasterises to a
solid block; the planes' points get N(0, sigma) in z (exactly flat planes would leave a refit's gate nothing to trim), and under every
step hang 800 points of a vertical face, 2 mm thick.

A layout is a placement of one frame's points on its pixels.  The detection does not depend on it (histograms, images and exact integer
sums commute), so the layouts of one frame share one oracle record; the kernels that keep one surface's sums in a wave's registers
(DESIGN.md sections 7d, 7f, 7g) do: `ordered` never mixes a slot, `slots` changes the surface at every slot without ever mixing one,
`lanes` and `scatter` mix every slot, `sparse` makes the cell list regroup cells that are not neighbours.
"""
import functools

import numpy as np

import clouds
import oracle_binding as ob
import riser_model
from test_labels import expected_labels

W, H = 640, 480
SIGMA = 0.001
N_STEPS = 16                                           # step plateaus: with the ground SSD_MAX_STEPS surfaces, SSD_MAX_RISERS faces
RISE, GOING, DEPTH = 0.06, 0.055, 0.15
FACE_POINTS, FACE_SIGMA = 800, 0.002
FILL = 1.3                                             # points per pixel of a plane's rectangle in the top-down image
X_RANGE, Y_RANGE = 1.2, 1.2                            # the default configuration's x and y extent (-0.6 .. 0.6, 0.1 .. 1.3)
CELL, GROUP = 64, 4                                    # kCell points per cell, four cells per wave iteration (load_cell)
LAYOUTS = ("ordered", "scatter", "lanes", "slots", "sparse")
FULL_LAYOUTS = LAYOUTS[:4]                             # the placements of ALL the frame's points (sparse keeps every second cell's)


def step_z(k):
    return 0.0055 + RISE * (k + 1)


def classes(n_steps=N_STEPS, width=W, height=H, sigma=SIGMA, seed=0, fill=FILL):
    """-> [float64 [n, 3] world points per class]: the ground, step 0 .. n_steps - 1, then the face under step 0 .. n_steps - 1"""
    rng = np.random.default_rng(1000 + seed)
    px, py = width / X_RANGE, height / Y_RANGE          # top-down pixels per metre

    def plane(z, xr, yr):
        cols = max(1, int((xr[1] - xr[0]) * px))
        n = int(fill * cols * int(round((yr[1] - yr[0]) * py)))
        p = clouds.plane_points(z, n, xr, yr, cols)
        p[:, 2] += rng.normal(0.0, sigma, len(p)) if sigma > 0 else 0.0
        return p

    out = [plane(0.005, (-0.3, 0.3), (0.12, 0.22))]
    for k in range(n_steps):
        y0 = 0.25 + GOING * k
        out.append(plane(step_z(k), (-0.2, 0.2), (y0, y0 + DEPTH)))
    for k in range(n_steps):
        below = step_z(k - 1) if k else 0.005
        out.append(np.stack([rng.uniform(-0.2, 0.2, FACE_POINTS), 0.25 + GOING * k + rng.normal(0.0, FACE_SIGMA, FACE_POINTS),
                             rng.uniform(below + 0.02, step_z(k) - 0.02, FACE_POINTS)], 1))
    return out


def _slots_order(sizes, n_pixels):
    """pixel -> (class, index in class) or invalid for the `slots` layout: the class of pixel p depends only on p % 4 and p // 256, the
    four classes of a block of 256 pixels are different ones and change from block to block (round robin over the classes that still
    have points).  A class's last, short run leaves the rest of its 64 pixels invalid, so that no slot ever holds two classes."""
    left = list(sizes)
    cls = np.full(n_pixels, -1, dtype=np.int64)
    at = 0
    n_cls = len(sizes)
    # a run's points go to the block's four cells in turn (row r of the block's 64 is point r % 16 of cell r // 16), and a class's last
    # two runs share what is left, so every run has points in all four cells: no cell of a block is empty, and the cell list keeps
    # the blocks whole
    rows = (np.arange(CELL) % GROUP) * (CELL // GROUP) + np.arange(CELL) // GROUP
    for b in range(n_pixels // (CELL * GROUP)):
        alive = [(at + i) % n_cls for i in range(n_cls) if left[(at + i) % n_cls] > 0][:GROUP]
        if not alive:
            break
        block = cls[b * CELL * GROUP:(b + 1) * CELL * GROUP].reshape(CELL, GROUP)
        for j, c in enumerate(alive):
            take = CELL if left[c] >= 2 * CELL else (left[c] + 1) // 2 if left[c] > CELL else left[c]
            block[rows[:take], j] = c
            left[c] -= take
        at = (alive[-1] + 1) % n_cls
    assert not any(left), "the slots layout does not fit the frame"
    return cls


def place(cls_points, width, height, layout, seed=0, z_shift=clouds.Z_SHIFT):
    """the classes' points on the pixels of a width x height frame -> (float32 [height, width, 3] in camera coordinates, int8 [W H]:
    the class of the point on each pixel, -1 = the pixel is invalid)"""
    n = width * height
    sizes = [len(p) for p in cls_points]
    total = sum(sizes)
    assert total <= n
    rng = np.random.default_rng(2000 + seed)
    cam = np.concatenate([p + np.array([0.0, 0.0, z_shift]) for p in cls_points]).astype(np.float32)
    which = np.concatenate([np.full(s, c, dtype=np.int8) for c, s in enumerate(sizes)])
    start = np.concatenate([[0], np.cumsum(sizes)])
    out = np.zeros((n, 3), dtype=np.float32)
    cls = np.full(n, -1, dtype=np.int8)
    if layout == "ordered":
        # plane after plane in plane order, as clouds.cloud lays them, each from a multiple of 256 pixels; what a plane has left for its
        # last block of 256 goes to that block's four cells in turn, so that every block holds points in all of its cells or in none
        # and the cell list, which keeps four cells to a group, never puts two planes into one group
        block = CELL * GROUP
        at = 0
        for c, size in enumerate(sizes):
            whole = size // block * block
            idx = np.arange(size)
            rest = idx[whole:] - whole
            idx[whole:] = whole + (rest % GROUP) * CELL + rest // GROUP
            assert at + idx.max() < n, "the ordered layout does not fit the frame"
            out[at + idx] = cam[start[c]:start[c + 1]]
            cls[at + idx] = c
            at = (at + size + block - 1) // block * block
    elif layout in ("scatter", "sparse"):
        idx = rng.permutation(n)[:total]
        out[idx] = cam
        cls[idx] = which
        if layout == "sparse":                          # every second 64-point cell all invalid: a group's four cells are no neighbours
            whole = n // CELL * CELL
            out[:whole].reshape(-1, CELL, 3)[1::2] = 0.0
            cls[:whole].reshape(-1, CELL)[1::2] = -1
    elif layout == "lanes":                             # consecutive pixels cycle through the classes while their points last
        rounds = np.concatenate([np.arange(s) for s in sizes])
        order = np.lexsort((which, rounds))              # round 0 of every class, round 1 of every class that has one, ...
        mixed = np.concatenate([start[c] + rng.permutation(s) for c, s in enumerate(sizes)])
        out[:total] = cam[mixed][order]
        cls[:total] = which[order]
    elif layout == "slots":
        cls[:] = _slots_order(sizes, n)
        for c, s in enumerate(sizes):
            out[cls == c] = cam[start[c] + rng.permutation(s)]
    else:
        raise ValueError(layout)
    return out.reshape(height, width, 3), cls


_FRAMES = {}


def _frame(layout, n_steps, width, height, z_shift, sigma, seed, fill):
    key = (layout, n_steps, width, height, z_shift, sigma, seed, fill)
    if key not in _FRAMES:
        f, cls = place(classes(n_steps, width, height, sigma, seed, fill), width, height, layout, seed, z_shift)
        f.setflags(write=False)
        cls.setflags(write=False)
        _FRAMES[key] = (f, cls)
    return _FRAMES[key]


def frame(layout="ordered", n_steps=N_STEPS, width=W, height=H, z_shift=clouds.Z_SHIFT, sigma=SIGMA, seed=0, fill=FILL):
    """a frame of the recipe (cached; treat it as read-only).  n_steps = 16: the full width, 8: the 9-surface frame, 2: three surfaces,
    0: the bare ground (no faces), 17: one past the width (wants 800 x 600)"""
    return _frame(layout, n_steps, width, height, z_shift, sigma, seed, fill)[0]


def frame_classes(layout="ordered", n_steps=N_STEPS, width=W, height=H, z_shift=clouds.Z_SHIFT, sigma=SIGMA, seed=0, fill=FILL):
    """int8 [W H]: the class of the point on each pixel of frame(...) (0 the ground, 1 .. n_steps the steps, then the faces), -1 = none"""
    return _frame(layout, n_steps, width, height, z_shift, sigma, seed, fill)[1]


TILE_CELLS = 16                                        # kTileHost / kCell: a launch's chunks are whole tiles of 1024 points


def census(labels, listed=None, cols=1, chunk_cells=None):
    """The slot composition of a walk over `labels` (uint8, one per point, 0 = none), following load_cell and cell_list_build
    (csrc/ssd_kernels.hip).  The frame is cut into chunks of chunk_cells 64-point cells (a block's share; a multiple of TILE_CELLS in
    a launch, csrc/ssd_chunks.h choose_chunk; None: one chunk spans the frame).  Per chunk: the listed cells in cell_list_build's
    order (cols = 1: ascending, as k_labels, k_surface_moments and k_surface_refit build it; cols > 1: column-major over rows of `cols`
    cells counted from the chunk's first, as k_risers and k_riser_moments do), four consecutive entries per group, the last group
    filled up with invalid points, and in a group lane l's point j = point 4 (l & 15) + j of entry l >> 4: slot j of a group holds the
    points j, j + 4, .. of its four cells.  `listed`: indices of the cells on the list (default: the cells that carry a label; the
    kernels list the cells whose mask of height-bin groups meets a wanted one).  The last cell may be partial.
    -> (n_labels int [slots]: distinct labels per slot, first int [slots]: the label of the slot's first labelled lane, 0 = none)
    A block's groups are dealt to its four waves in runs; that only cuts this sequence."""
    lab = np.asarray(labels, dtype=np.uint8).reshape(-1)
    n_cells = (len(lab) + CELL - 1) // CELL
    full = np.zeros(n_cells * CELL, dtype=np.uint8)
    full[:len(lab)] = lab
    cells = full.reshape(n_cells, CELL)
    if listed is None:
        listed = np.flatnonzero(cells.any(axis=1))
    listed = np.sort(np.asarray(listed, dtype=np.int64))
    chunk = chunk_cells or max(n_cells, 1)
    rel = listed % chunk
    listed = listed[np.lexsort((rel // cols, rel % cols, listed // chunk))]        # by chunk, then column, then row (cols = 1: ascending)
    # a new group at every chunk: entry numbers count from the chunk's first listed cell
    of_chunk = listed // chunk
    first_of_chunk = np.searchsorted(of_chunk, of_chunk)
    entry = np.arange(len(listed)) - first_of_chunk
    groups_before = np.concatenate([[0], np.cumsum((np.bincount(of_chunk, minlength=1) + GROUP - 1) // GROUP)])
    row = (groups_before[of_chunk] + entry // GROUP) * GROUP + entry % GROUP
    rows = np.zeros((int(groups_before[-1]) * GROUP, CELL), dtype=np.uint8)             # entries past a chunk's list: invalid points
    rows[row] = cells[listed]
    # [group, entry, 16 lanes, j] -> [group, j, entry, 16 lanes] = the 64 lanes of slot j in lane order
    slots = rows.reshape(-1, GROUP, CELL // 4, 4).transpose(0, 3, 1, 2).reshape(-1, CELL)
    srt = np.sort(slots, axis=1)
    n_labels = (srt[:, 0] > 0).astype(np.int64) + ((srt[:, 1:] != srt[:, :-1]) & (srt[:, 1:] > 0)).sum(axis=1)
    first = slots[np.arange(len(slots)), (slots > 0).argmax(axis=1)]
    return n_labels, first


def cells_with(mask):
    """indices of the 64-point cells that hold a point of the boolean per-point `mask` (the last cell may be partial)"""
    m = np.asarray(mask, dtype=bool).reshape(-1)
    n_cells = (len(m) + CELL - 1) // CELL
    full = np.zeros(n_cells * CELL, dtype=bool)
    full[:len(m)] = m
    return np.flatnonzero(full.reshape(n_cells, CELL).any(axis=1))


def valid_cells(xyz):
    """the cells that hold a valid point (z > 0): the most a kernel's list can hold"""
    return cells_with(np.asarray(xyz, dtype=np.float32).reshape(-1, 3)[:, 2] > 0)


def surfaces_per_cell(labels):
    """distinct labels per 64-point cell that carries one"""
    lab = np.asarray(labels, dtype=np.uint8).reshape(-1)
    cells = np.sort(lab[:len(lab) // CELL * CELL].reshape(-1, CELL), axis=1)
    n = (cells[:, 0] > 0).astype(np.int64) + ((cells[:, 1:] != cells[:, :-1]) & (cells[:, 1:] > 0)).sum(axis=1)
    return n[n > 0]


TOL, SUPPORT = 0.03, 200                               # the riser rule's tolerance and min_support the references below are made with
_REFS = {}


class Reference:
    """What the oracle and the host restatements say about one frame, each computed on first use and kept; nothing of it comes from a
    GPU.  xyz, classes (frame_classes), cfg, trans, cal (the calibration's constants), ocfg, ocal are there from the start."""

    def __init__(self, ssd, oracle, key):
        self.key, self._ssd, self._oracle = key, ssd, oracle
        self.layout, self.n_steps, self.width, self.height, self.z_shift, fill = key
        self.xyz = frame(self.layout, self.n_steps, self.width, self.height, self.z_shift, fill=fill)
        self.classes = frame_classes(self.layout, self.n_steps, self.width, self.height, self.z_shift, fill=fill)
        self.cfg = ssd.default_config(self.width, self.height)
        self.trans = clouds.calibration(ssd, self.z_shift)
        self.cal = self.trans.constants
        self.ocfg, self.ocal = ob.to_oracle_config(self.cfg), ob.to_oracle_calibration(self.cal)

    @functools.cached_property
    def res(self):
        """the oracle's record of the frame"""
        return self._oracle.process(self.ocfg, self.ocal, self.xyz)[0]

    @property
    def unlimited(self):
        """the oracle, which knows no SSD_MAX_STEPS, reports more surfaces than a handle can: it is no reference for labels then"""
        return self.res.n_steps > self._ssd.MAX_STEPS

    @property
    def ground(self):
        return 1 if (self.res.n_steps > 0 and self.res.ground_ind >= 0) else 0

    @functools.cached_property
    def risers(self):
        """the oracle's list of Riser at TOL and SUPPORT"""
        return self._oracle.risers(self.ocfg, self.ocal, self.xyz, TOL, SUPPORT)

    @functools.cached_property
    def labels(self):
        """the checker's labels (test_labels.expected_labels)"""
        assert not self.unlimited
        return expected_labels(self._oracle, self.cfg, self.cal, self.res, self.xyz)

    @functools.cached_property
    def _evidence(self):
        assert not self.unlimited
        return riser_model.evidence(self.cfg, self.cal, self.res, self.xyz, TOL)

    @property
    def riser_labels(self):
        """riser_model.evidence on the oracle's record: label i + 1 = evidence of riser i"""
        return self._evidence[0]

    @property
    def riser_offsets(self):
        return self._evidence[1]


def reference(ssd, oracle, layout="ordered", n_steps=N_STEPS, width=W, height=H, z_shift=clouds.Z_SHIFT, fill=FILL):
    """the Reference of a frame of the recipe: made once per frame and shared by the CPU and the GPU tests"""
    key = (layout, n_steps, width, height, z_shift, fill)
    if key not in _REFS:
        _REFS[key] = Reference(ssd, oracle, key)
    return _REFS[key]
