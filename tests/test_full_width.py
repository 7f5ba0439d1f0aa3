"""The full-width frames of tests/full_width.py under the oracle and the host functions alone (no GPU): every frame and layout detects
what it was built for (17 surfaces, 16 risers with evidence, every label present), the slot census of every layout is what the layout
is for, the host statements agree with the oracle at that width, and the layouts of one frame share their detection record.  The GPU
tier (tests/test_gpu_full_width.py) runs the kernels on the same frames against the same references."""
import ctypes as C

import numpy as np
import pytest

import full_width as fw
import riser_model as rm

FULL, NINE, THREE, BARE = 16, 8, 2, 0
# (layout, step plateaus, width, height, camera z_shift)
FRAMES = ([(l, FULL, fw.W, fw.H, 0.5) for l in fw.LAYOUTS] + [("scatter", NINE, fw.W, fw.H, 0.5), ("ordered", BARE, fw.W, fw.H, 0.5),
          ("scatter", THREE, fw.W, fw.H, 0.5)] + [(l, FULL, 642, 479, 0.5) for l in fw.LAYOUTS]
          + [(l, FULL, fw.W, fw.H, 0.7) for l in fw.LAYOUTS] + [("scatter", NINE, fw.W, fw.H, 0.7), ("ordered", BARE, fw.W, fw.H, 0.7)])
IDS = ["%s-%d-%dx%d-z%g" % f for f in FRAMES]
MIN_POINTS, K_SIGMA = 200, 2.5

# What this recipe gives, measured under the oracle and the host functions and pinned, so that a change to the recipe shows: the valid
# points, the points per label, the least and the most evidence of a riser, the narrowest and the widest gate in mm (rounded outward
# to a micrometre; the two cameras differ by less than that).  The placements of all points (ordered, scatter, lanes, slots) share one row, both cameras too.
VGA_LABELS = [11076, 16324, 16112, 16112, 16324, 16324, 16324, 16324, 16324, 16324, 16112, 16112, 16112, 16112, 16324, 16324, 16112]
FIGURES = {
    (FULL, fw.W, "all"): (295264, VGA_LABELS, (795, 800), (2.470, 2.529)),
    (NINE, fw.W, "all"): (155952, VGA_LABELS[:9], (795, 800), (2.477, 2.529)),
    (THREE, fw.W, "all"): (51468, VGA_LABELS[:3], (797, 799), (2.477, 2.510)),
    (FULL, 642, "all"): (296564, [11128] + [16401] * 15 + [16188], (800, 800), (2.466, 2.525)),
    (FULL, fw.W, "sparse"): (147731, [5590, 8211, 8047, 8118, 8135, 8174, 8183, 8272, 8082, 8168, 8154, 8051, 8045, 7964, 8081, 8044, 8027],
                             (380, 409), (2.473, 2.527)),
    (FULL, 642, "sparse"): (148412, [5595, 8241, 8235, 8240, 8122, 8384, 8234, 8336, 8209, 8193, 8309, 8192, 8108, 8157, 7955, 8045, 8014],
                            (371, 418), (2.480, 2.542)),
}


def _ref(ssd, oracle, f):
    layout, n_steps, w, h, z = f
    return fw.reference(ssd, oracle, layout, n_steps, w, h, z)


@pytest.mark.parametrize("f", FRAMES, ids=IDS)
def test_every_frame_detects_what_it_was_built_for(ssd, oracle, f):
    """the oracle's record: ground plus every step, status 0, four corners on every step plateau, every riser detected on 795 to 800
    of its 800 points (about half of them on the sparse frames); the checker's labels name every surface; riser_model.evidence gives
    the oracle's counts; the host gates are OK for every surface and lie around 2.5 sigma = 2.5 mm; the host refit trims every surface
    and empties none.  Valid points, points per label, riser counts and gates are this recipe's own figures (FIGURES)."""
    r = _ref(ssd, oracle, f)
    layout, n_steps = r.layout, r.n_steps
    res = r.res
    if n_steps == BARE:
        assert (res.n_plateaus, res.n_steps, res.status) == (1, 0, 0) and len(r.risers) == 0
        assert not r.labels.any() and not r.riser_labels.any()
        return
    n = n_steps + 1
    assert (res.n_plateaus, res.n_steps, res.status, res.ground_ind) == (n, n, 0, 0)
    steps = [res.plateaus[k] for k in range(res.n_plateaus) if res.plateaus[k].is_step]
    assert len(steps) == n_steps and all(p.valid and list(p.corner_found) == [1, 1, 1, 1] for p in steps)
    # valid points: every plane's and every face's (sparse: those of every second cell)
    want_valid, want_labels, (r_lo, r_hi), (g_lo, g_hi) = FIGURES[(n_steps, r.width, "sparse" if layout == "sparse" else "all")]
    valid = int((r.xyz[..., 2] > 0).sum())
    total = sum(len(c) for c in fw.classes(n_steps, r.width, r.height))
    assert valid == want_valid and (valid == total or layout == "sparse")
    assert int((r.classes >= 0).sum()) == valid and np.array_equal(r.classes >= 0, r.xyz.reshape(-1, 3)[:, 2] > 0)
    # risers
    assert len(r.risers) == n_steps and all(o.detected == 1 for o in r.risers)
    counts = [o.n_points for o in r.risers]
    assert (min(counts), max(counts)) == (r_lo, r_hi) and (layout == "sparse" or 795 <= r_lo <= r_hi <= fw.FACE_POINTS), counts
    counts = np.bincount(r.riser_labels, minlength=ssd.MAX_STEPS + 1)[1:]
    assert counts[:n_steps].tolist() == [o.n_points for o in r.risers] and not counts[n_steps:].any()
    got = rm.counts_and_offsets(r.riser_labels, r.riser_offsets, n_steps)
    assert all(abs(m - o.mean_offset) <= 1e-12 for (_, m), o in zip(got, r.risers))
    # labels
    per = np.bincount(r.labels, minlength=ssd.MAX_STEPS + 1)[1:]
    assert (per[:n] > 0).all() and not per[n:].any(), per
    assert per[0] == res.ground_n_in_quad and per[1:n].tolist() == [p.n_in_quad for p in steps]
    assert per[:n].tolist() == want_labels
    # gates and the host refit
    first = ssd.surface_moments_host(r.cfg, r.xyz, r.labels, n, r.ground)
    assert (first.n_surfaces, first.ground) == (n, 1)
    assert [int(first.s[k].m.n + first.s[k].n_far) for k in range(ssd.MAX_STEPS)] == per.tolist()
    gates = ssd.surface_gates_from_moments(first, MIN_POINTS, K_SIGMA, 0.0)
    fits = ssd.surface_fit_solve(first, r.cal, MIN_POINTS)
    assert gates.n_surfaces == n
    widths = [gates.g[k].gate * 1e3 for k in range(n)]
    assert all(fits.s[k].status == ssd.GF_OK for k in range(n))
    assert g_lo <= min(widths) < g_lo + 0.002 and g_hi - 0.002 < max(widths) <= g_hi, (min(widths), max(widths))
    refit = ssd.surface_refit_moments_host(r.cfg, r.xyz, r.labels, gates, n, r.ground)
    for k in range(n):
        assert 0 < refit.s[k].m.n < first.s[k].m.n, k
    used = 8 + n * C.sizeof(ssd.SurfaceMoments)
    assert bytes(refit)[used:] == bytes(C.sizeof(ssd.FrameMoments) - used)


SEVENTEEN = [f for f in FRAMES if f[1] == FULL]


@pytest.mark.parametrize("f", SEVENTEEN, ids=["%s-%d-%dx%d-z%g" % f for f in SEVENTEEN])
def test_the_slot_census_of_every_layout(ssd, oracle, f):
    """conditions on the INPUT, from full_width.census over the checker's labels, for chunks of one tile, of 32 tiles and of the whole
    frame, and for both ends of what a kernel's cell list can hold (every cell with a valid point; those without the face-only cells):
    ordered - no slot holds two labels (and no 64-point cell two surfaces: what tests/clouds.py's frames give);
    slots - no slot holds two labels, and at least 90 % of consecutive labelled slots differ in label (a change-over at every slot,
    no lane on the direct path);
    lanes, scatter, sparse - at least 90 % of labelled slots hold 8 or more labels, and the first labelled lane's label varies"""
    r = _ref(ssd, oracle, f)
    n_cls = 1 + r.n_steps                                             # classes 0 .. n_steps: the planes; above: the faces
    most = fw.valid_cells(r.xyz)                                      # every cell a kernel can list
    least = fw.cells_with((r.classes >= 0) & (r.classes < n_cls))     # without the cells that hold nothing but face points
    if r.layout in ("ordered", "slots"):
        # what keeps a group on one block of 256 pixels, whatever the chunk: every block is listed whole or not at all
        for cells in (most, least):
            per_block = np.bincount(cells // fw.GROUP)
            assert set(per_block.tolist()) <= {0, fw.GROUP}, "a block of four cells is listed in part"
    # one tile per block (what a batch of 8 VGA frames gets: csrc/ssd_chunks.h choose_chunk), 32 tiles, and the frame as one chunk
    for chunk in (fw.TILE_CELLS, 32 * fw.TILE_CELLS, None):
        for cells in (most, least):
            n_labels, first = fw.census(r.labels, cells, chunk_cells=chunk)
            labelled = n_labels > 0
            assert labelled.sum() >= 2000
            lead = first[labelled]
            differ = float((lead[1:] != lead[:-1]).mean())
            if r.layout == "ordered":
                assert int(n_labels.max()) == 1 and int(fw.surfaces_per_cell(r.labels).max()) == 1
                assert differ < 0.01, "a surface's slots follow each other"
            elif r.layout == "slots":
                assert int(n_labels.max()) == 1
                assert differ >= 0.9, differ
            else:
                assert float((n_labels[labelled] >= 8).mean()) >= 0.9
                assert int(n_labels.max()) == ssd.MAX_STEPS
                assert differ >= 0.9 and len(set(lead.tolist())) == ssd.MAX_STEPS, "every surface leads a slot somewhere"
    if r.layout == "sparse":
        assert (most[:-1] % 2 == 0).all() and len(most) >= r.width * r.height // fw.CELL // 2, "every second cell, all of them"
    # the riser kernels' list is column-major over rows of cellCols cells (csrc/ssd_capi.hip: (W + 32) / 64)
    if r.layout in ("scatter", "lanes", "sparse"):
        for chunk in (fw.TILE_CELLS, None):
            n_r, lead_r = fw.census(r.riser_labels, most, cols=(r.width + 32) // 64, chunk_cells=chunk)
            assert int(n_r.max()) >= 4 and len(set(lead_r[n_r > 0].tolist())) == ssd.MAX_RISERS
            assert float((n_r[n_r > 0] >= 2).mean()) >= 0.5, "most slots with evidence hold two risers or more"


def _detection(res):
    """what of a record does not depend on the order of the points (the running-sum means do, in their last bits)"""
    out = [res.status, res.n_nonzero, res.n_inrange, res.n_bins, list(res.hist), res.n_plateaus, res.ground_ind, res.first_valid_ind,
           res.n_steps, res.ground_n_in_quad, list(res.ground_quad_world)]
    for k in range(res.n_plateaus):
        p = res.plateaus[k]
        out.append((p.peak_bin, p.bin_lo, p.bin_hi, p.n_points, p.is_step, p.valid, list(p.corner_found), list(p.quad_world), p.n_in_quad))
    return out


@pytest.mark.parametrize("w,h,z", [(fw.W, fw.H, 0.5), (642, 479, 0.5), (fw.W, fw.H, 0.7)])
def test_the_layouts_of_one_frame_share_their_detection(ssd, oracle, w, h, z):
    """ordered, scatter, lanes and slots place the same points: histogram, plateaus, quadrilaterals, counts and the risers' counts are
    equal, the means (running double sums in point order) to 1e-12; sparse, which keeps half the points, is a frame of its own"""
    refs = [fw.reference(ssd, oracle, l, FULL, w, h, z) for l in fw.FULL_LAYOUTS]
    pts = [np.sort(r.xyz.reshape(-1, 3).view([("x", "f4"), ("y", "f4"), ("z", "f4")]).ravel(), order=("x", "y", "z")) for r in refs]
    for r, p in zip(refs[1:], pts[1:]):
        assert np.array_equal(p, pts[0]), "the layouts are permutations of one set of points"
        assert _detection(r.res) == _detection(refs[0].res), r.layout
        assert [(o.n_points, o.detected) for o in r.risers] == [(o.n_points, o.detected) for o in refs[0].risers], r.layout
        for k in range(r.res.n_plateaus):
            assert abs(r.res.plateaus[k].mean_z - refs[0].res.plateaus[k].mean_z) <= 1e-12
        assert np.array_equal(np.bincount(r.labels, minlength=18), np.bincount(refs[0].labels, minlength=18))
    sparse = fw.reference(ssd, oracle, "sparse", FULL, w, h, z)
    assert not np.array_equal(np.bincount(sparse.labels, minlength=18), np.bincount(refs[0].labels, minlength=18))
    whole = w * h // fw.CELL * fw.CELL
    kept = lambda x: x.reshape(-1, 3)[:whole].reshape(-1, fw.CELL, 3)
    assert np.array_equal(kept(sparse.xyz)[::2], kept(refs[1].xyz)[::2]) and not kept(sparse.xyz)[1::2].any(), "scatter's even cells"


def test_one_step_past_the_width_is_eighteen_plateaus(ssd, oracle):
    """ground plus 17 step plateaus at 800 x 600 (1.25 points per pixel: 1.3 do not fit): the oracle, which knows no SSD_MAX_STEPS,
    reports 18 plateaus and 18 steps, every one valid, and 17 risers"""
    r = fw.reference(ssd, oracle, "scatter", 17, 800, 600, fill=1.25)
    assert (r.res.n_plateaus, r.res.n_steps, r.res.status) == (18, 18, 0) and r.unlimited
    assert all(r.res.plateaus[k].valid for k in range(1, 18))
    assert len(r.risers) == 17 and all(o.detected for o in r.risers)
    r16 = fw.reference(ssd, oracle, "scatter", FULL, 800, 600)
    assert (r16.res.n_plateaus, r16.res.n_steps) == (17, 17), "the 16-step recipe reaches 17 surfaces at 800 x 600 too"


def test_the_census_on_a_hand_made_walk():
    """full_width.census itself: four cells whose points' labels are their index modulo 4 + 1 give four slots of one label each; the
    same labels cell-wise give four slots of four labels; a dropped cell regroups; column-major order for cols > 1"""
    lab = np.tile(np.arange(4, dtype=np.uint8) + 1, 64)                       # point p: label p % 4 + 1
    n, first = fw.census(lab)
    assert n.tolist() == [1, 1, 1, 1] and first.tolist() == [1, 2, 3, 4]
    lab = np.repeat(np.arange(4, dtype=np.uint8) + 1, 64)                     # cell c: label c + 1
    n, first = fw.census(lab)
    assert n.tolist() == [4, 4, 4, 4] and first.tolist() == [1, 1, 1, 1]
    lab = np.repeat(np.array([1, 0, 2, 3, 4, 5], dtype=np.uint8), 64)         # cell 1 carries nothing: cells 0, 2, 3, 4 | 5
    n, first = fw.census(lab)
    assert n.tolist() == [4] * 4 + [1] * 4 and first.tolist() == [1] * 4 + [5] * 4
    n, first = fw.census(lab, listed=np.arange(6))                            # listed all the same: cells 0 .. 3 | 4, 5
    assert n.tolist() == [3] * 4 + [2] * 4 and first.tolist() == [1] * 4 + [4] * 4
    lab = np.repeat(np.arange(8, dtype=np.uint8) + 1, 64)                     # two columns: cells 0, 2, 4, 6 | 1, 3, 5, 7
    n, first = fw.census(lab, cols=2)
    assert n.tolist() == [4] * 8 and first.tolist() == [1] * 4 + [2] * 4
    lab = np.zeros(70, dtype=np.uint8)                                        # a partial last cell
    lab[69] = 7
    n, first = fw.census(lab)
    assert n.tolist() == [0, 1, 0, 0] and first.tolist() == [0, 7, 0, 0]

    lab = np.repeat(np.array([1, 0, 2, 3, 4, 5], dtype=np.uint8), 64)         # chunks of four cells: 0, 2, 3 | 4, 5
    n, first = fw.census(lab, chunk_cells=4)
    assert n.tolist() == [3] * 4 + [2] * 4 and first.tolist() == [1] * 4 + [4] * 4
    lab = np.repeat(np.arange(8, dtype=np.uint8) + 1, 64)                     # two columns inside chunks of four: 0, 2, 1, 3 | 4, 6, 5, 7
    n, first = fw.census(lab, cols=2, chunk_cells=4)
    assert n.tolist() == [4] * 8 and first.tolist() == [1] * 4 + [5] * 4
