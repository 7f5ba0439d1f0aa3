"""Riser labels (include/ssd_hip.h), the CPU tier: ssd_labels_split, and the recipe the GPU tests
(test_gpu_riser_labels.py) rely on, under the oracle - a surface label and a riser label never meet at a pixel, and every riser those
tests count on has evidence.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import full_width as fw
import ground_model as gm
import oracle_binding as ob
import riser_model as rm
from test_labels import expected_labels

TOL = fw.TOL
BASE = 32
ACCEPTED, REFUSED = (0, 17, 32, 47), (18, 31, 48, 255)


def _split(ssd, labels, surfaces, risers):
    """the C entry point on numpy arrays (None: a NULL output)"""
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return ssd.lib().ssd_labels_split(ptr(labels), labels.size, ptr(surfaces), ptr(risers))


def _every_label():
    """every accepted value, the boundaries at both ends of a run of others"""
    return np.array(list(range(0, 18)) + list(range(32, 48)) + [0, 47, 17, 32, 1, 33], dtype=np.uint8)


def _want(labels):
    lab = labels.astype(np.int64)
    return np.where(lab <= 17, lab, 0).astype(np.uint8), np.where(lab >= BASE, lab - BASE + 1, 0).astype(np.uint8)


def test_the_constants_and_the_names(ssd):
    assert ssd.LABEL_RISER_BASE == BASE > ssd.MAX_STEPS == 17 and ssd.MAX_RISERS == 16
    for n in ("ssd_set_riser_labels", "ssd_get_riser_labels_time_back", "ssd_labels_split"):
        assert n in ssd.EXPORTS and hasattr(ssd.lib(), n)
    for m in ("set_riser_labels", "riser_labels_time_ms"):
        assert callable(getattr(ssd.Detector, m))
    assert ssd.lib().ssd_set_riser_labels(None, 1) == -1 and b"null" in ssd.lib().ssd_last_error()
    ms = C.c_float(0.0)
    assert ssd.lib().ssd_get_riser_labels_time_back(None, 0, C.byref(ms)) == -1


def test_split_gives_both_halves(ssd):
    """surfaces keeps 0 .. SSD_MAX_STEPS and zeroes the rest, risers holds i + 1 for SSD_LABEL_RISER_BASE + i and zero elsewhere: each
    in the form ssd_surface_moments_host accepts (at most 17 and 16)"""
    labels = _every_label()
    keep = labels.copy()
    surfaces, risers = np.full_like(labels, 0xA5), np.full_like(labels, 0xA5)
    assert _split(ssd, labels, surfaces, risers) == 0
    ws, wr = _want(keep)
    assert np.array_equal(surfaces, ws) and np.array_equal(risers, wr) and np.array_equal(labels, keep)
    assert int(surfaces.max()) == 17 and int(risers.max()) == 16 and not ((surfaces > 0) & (risers > 0)).any()
    s2, r2 = ssd.labels_split(keep.reshape(2, -1))
    assert s2.shape == r2.shape == (2, len(keep) // 2) and np.array_equal(s2.reshape(-1), ws) and np.array_equal(r2.reshape(-1), wr)


def test_split_with_a_null_output_and_in_place(ssd):
    labels = _every_label()
    ws, wr = _want(labels)
    only = np.full_like(labels, 0xA5)
    assert _split(ssd, labels, only, None) == 0 and np.array_equal(only, ws)
    only[:] = 0xA5
    assert _split(ssd, labels, None, only) == 0 and np.array_equal(only, wr)
    assert _split(ssd, labels, None, None) == 0
    # either output may be the input
    a, other = labels.copy(), np.full_like(labels, 0xA5)
    assert _split(ssd, a, a, other) == 0 and np.array_equal(a, ws) and np.array_equal(other, wr)
    a, other = labels.copy(), np.full_like(labels, 0xA5)
    assert _split(ssd, a, other, a) == 0 and np.array_equal(a, wr) and np.array_equal(other, ws)
    a = labels.copy()
    assert _split(ssd, a, None, a) == 0 and np.array_equal(a, wr)
    empty = np.zeros(0, dtype=np.uint8)
    assert ssd.lib().ssd_labels_split(None, 0, None, None) == 0 and _split(ssd, empty, empty, empty) == 0


@pytest.mark.parametrize("value", ACCEPTED)
def test_split_accepts_the_boundary_labels(ssd, value):
    labels = np.array([3, value, 40], dtype=np.uint8)
    surfaces, risers = ssd.labels_split(labels)
    assert surfaces.tolist() == [3, value if value <= 17 else 0, 0]
    assert risers.tolist() == [0, value - BASE + 1 if value >= BASE else 0, 9]


@pytest.mark.parametrize("value", REFUSED)
@pytest.mark.parametrize("at", [0, 4])
def test_split_refuses_a_label_of_neither_range_before_it_writes(ssd, value, at):
    """SSD_E_ARG and both outputs untouched - also the entries in front of the bad label, also in place"""
    labels = np.array([1, 33, 17, 47, 0], dtype=np.uint8)
    labels[at] = value
    keep = labels.copy()
    surfaces, risers = np.full_like(labels, 0xA5), np.full_like(labels, 0xA5)
    assert _split(ssd, labels, surfaces, risers) == -1 and b"ssd_labels_split" in ssd.lib().ssd_last_error()
    assert np.all(surfaces == 0xA5) and np.all(risers == 0xA5) and np.array_equal(labels, keep)
    assert _split(ssd, labels, labels, None) == -1 and _split(ssd, labels, None, labels) == -1 and np.array_equal(labels, keep)
    with pytest.raises(ssd.SsdError):
        ssd.labels_split(labels)


def _both(oracle, cfg, cal, xyz):
    ocfg, ocal = ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal)
    rec = oracle.process(ocfg, ocal, xyz)[0]
    return rec, expected_labels(oracle, cfg, cal, rec, xyz), rm.riser_labels(cfg, cal, rec, xyz, TOL)


def test_the_recipe_on_the_three_step_scene(ssd, oracle):
    """ground_model's 256 x 192 scene: three surfaces, two risers with evidence, no pixel with both kinds of label, and the riser
    labels count what the oracle's risers count"""
    sc = gm.scene(ssd, "steps")
    cfg, trans = ssd.default_config(gm.W, gm.H), ssd.transformation_for_scene(sc)
    xyz = ssd.synth_host([sc])[0]
    rec, surfaces, risers = _both(oracle, cfg, trans.constants, xyz)
    assert rec.n_steps == 3 and int(surfaces.max()) == 3 and int(risers.max()) == 2
    assert not ((surfaces > 0) & (risers > 0)).any(), "a surface label and a riser label at one pixel"
    counts = np.bincount(risers, minlength=3)[1:]
    assert counts.min() >= 1
    ora = oracle.risers(ob.to_oracle_config(cfg), ob.to_oracle_calibration(trans.constants), xyz, TOL, 1)
    assert [r.n_points for r in ora] == counts.tolist()
    # the mask the product writes: one byte holds both, and the split gives them back
    mask = np.where(risers > 0, risers + (BASE - 1), surfaces).astype(np.uint8)
    s, r = ssd.labels_split(mask)
    assert np.array_equal(s, surfaces) and np.array_equal(r, risers)


@pytest.mark.parametrize("layout,n_steps", [("scatter", 16), ("sparse", 16), ("scatter", 8)])
def test_the_recipe_at_sixteen_risers(ssd, oracle, layout, n_steps):
    """full_width's frames: every one of the 16 (8) risers has evidence, no pixel carries both kinds of label, and the riser labels of
    the 17-surface frame reach SSD_LABEL_RISER_BASE + 15 = 47 in the product's mask"""
    r = fw.reference(ssd, oracle, layout, n_steps)
    assert r.res.n_steps == n_steps + 1 and not r.unlimited
    surfaces, risers = r.labels, r.riser_labels
    assert not ((surfaces > 0) & (risers > 0)).any(), "a surface label and a riser label at one pixel"
    counts = np.bincount(risers, minlength=n_steps + 1)[1:]
    assert len(counts) == n_steps and counts.min() >= 1 and [x.n_points for x in r.risers] == counts.tolist()
    mask = np.where(risers > 0, risers + (BASE - 1), surfaces).astype(np.uint8)
    assert int(mask.max()) == BASE + n_steps - 1
    s, rr = ssd.labels_split(mask)
    assert np.array_equal(s, surfaces) and np.array_equal(rr, risers)
    want = ssd.surface_moments_host(r.cfg, r.xyz, risers, n_steps, 0)
    assert bytes(ssd.surface_moments_host(r.cfg, r.xyz, rr, n_steps, 0)) == bytes(want)
