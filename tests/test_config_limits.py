"""Every limit ssd_create enforces, at the limit (accepted) and one step past it (refused with a message that names the
limit).  make_params runs before ssd_create looks for a device: without a GPU an accepted configuration returns
SSD_E_NODEVICE, with one it returns SSD_OK (the handle is destroyed again).

The numbers come from the header's constants and the formulas of make_params (ssd_capi.hip), not from a copy of them."""
import ctypes as C
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NODEVICE = -1, -4


def _header_constants():
    text = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(SSD_MAX_\w+)\s+(\d+)\b", text, flags=re.M)}


K = _header_constants()
# scan columns of an image: (W - 1) / 25 + 2 <= SSD_MAX_SCANS
MAX_WIDTH = 25 * (K["SSD_MAX_SCANS"] - 1)
# vertical-edge probe rows: (H - 1) / 10 + 1 <= SSD_MAX_EDGE_PTS
MAX_HEIGHT = 10 * K["SSD_MAX_EDGE_PTS"]
# frames of a batch lie on a grid dimension of at most 65535 blocks
MAX_FRAMES = 0xFFFF
FIXED_POINT_SUM = 2.0 ** 23          # max|z| * W * H below it: the sum of round(z * 2^40) over a frame stays an int64
Z_ABS = 2048.0                       # |z| below it: the magic-constant add that rounds z to the 2^-40 grid is exact


def n_bins(z_min, z_max, height_interval):
    """pointcloud.cpp:196 as make_params evaluates it"""
    return int((z_max - z_min) * (1 / height_interval)) + 1


def _interval_for(bins, z_min=-0.1, z_max=1.1):
    """a height interval that gives `bins` bins with the quotient half-way between two integers (no rounding can move it)"""
    h = (z_max - z_min) / (bins - 0.5)
    q = (z_max - z_min) * (1 / h)
    assert abs(q - round(q)) > 0.4 and n_bins(z_min, z_max, h) == bins
    return h


def _bins_cfg(bins):
    return dict(height_interval=_interval_for(bins))


def _z_cfg(width, height, z_abs, sign, interval):
    """z range [-0.1, z_abs] (sign > 0) or [-z_abs, 0.1]: max|z| = z_abs"""
    d = dict(width=width, height=height, height_interval=interval)
    d.update(dict(z_min=-0.1, z_max=z_abs) if sign > 0 else dict(z_min=-z_abs, z_max=0.1))
    return d


# XGA: max|z| just below / at 2^23 / (W * H), 8.5 cm bins (127 bins)
_XGA = 1024 * 768
_Z_XGA_IN = math.floor(FIXED_POINT_SUM / _XGA * 1000) / 1000
_Z_XGA_OUT = math.ceil(FIXED_POINT_SUM / _XGA * 1000) / 1000
# |z| just below 2048 m on a frame small enough for the product limit, 16.1 m bins (128 bins)
_SMALL = (64, 64)

# (id, overrides at the limit, overrides one step past it, what the refusal names)
LIMITS = [
    ("width", dict(width=MAX_WIDTH, height=2), dict(width=MAX_WIDTH + 1, height=2), "SSD_MAX_SCANS"),
    ("height", dict(width=3, height=MAX_HEIGHT), dict(width=3, height=MAX_HEIGHT + 1), "SSD_MAX_EDGE_PTS"),
    ("row_key", dict(width=3, height=MAX_HEIGHT), dict(width=3, height=8065), "8064"),
    ("smallest", dict(width=1, height=1), dict(width=0, height=1), "resolution"),
    ("smallest_h", dict(width=1, height=1), dict(width=1, height=0), "resolution"),
    ("bins_max", _bins_cfg(K["SSD_MAX_BINS"]), _bins_cfg(K["SSD_MAX_BINS"] + 1), "bins"),
    ("bins_min", _bins_cfg(3), _bins_cfg(2), "bins"),
    ("fixed_point_pos", _z_cfg(1024, 768, _Z_XGA_IN, 1, 0.085), _z_cfg(1024, 768, _Z_XGA_OUT, 1, 0.085), "2^23"),
    ("fixed_point_neg", _z_cfg(1024, 768, _Z_XGA_IN, -1, 0.085), _z_cfg(1024, 768, _Z_XGA_OUT, -1, 0.085), "2^23"),
    ("largest_frame", dict(width=MAX_WIDTH, height=int(FIXED_POINT_SUM / 1.1 / MAX_WIDTH)),
     dict(width=MAX_WIDTH, height=int(FIXED_POINT_SUM / 1.1 / MAX_WIDTH) + 1), "2^23"),
    ("z_abs_pos", _z_cfg(*_SMALL, Z_ABS - 0.1, 1, 16.1), _z_cfg(*_SMALL, Z_ABS, 1, 16.1), "2048"),
    ("z_abs_neg", _z_cfg(*_SMALL, Z_ABS - 0.1, -1, 16.1), _z_cfg(*_SMALL, Z_ABS, -1, 16.1), "2048"),
    ("step_plateaus_max", dict(max_step_plateaus=K["SSD_MAX_STEP_IMAGES"]), dict(max_step_plateaus=K["SSD_MAX_STEP_IMAGES"] + 1),
     "max_step_plateaus"),
    ("step_plateaus_min", dict(max_step_plateaus=1), dict(max_step_plateaus=0), "max_step_plateaus"),
    ("frames_max", dict(width=64, height=16, max_frames_per_batch=MAX_FRAMES, max_step_plateaus=1),
     dict(width=64, height=16, max_frames_per_batch=MAX_FRAMES + 1, max_step_plateaus=1), "max_frames_per_batch"),
    ("frames_min", dict(max_frames_per_batch=1), dict(max_frames_per_batch=0), "max_frames_per_batch"),
]


def _config(ssd, overrides):
    cfg = ssd.default_config(640, 480, max_frames_per_batch=1)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def _create(ssd, cfg):
    L = ssd.lib()
    cal = ssd.GeometricTransformation().constants
    h = C.c_void_p()
    rc = L.ssd_create(C.byref(cfg), C.byref(cal), 0, C.byref(h))
    msg = L.ssd_last_error().decode()
    if rc == 0:
        L.ssd_destroy(h)
    return rc, msg


def test_limit_table_is_what_make_params_states():
    """the derived limits are the ones the documentation states"""
    assert (MAX_WIDTH - 1) // 25 + 2 == K["SSD_MAX_SCANS"] and MAX_WIDTH // 25 + 2 > K["SSD_MAX_SCANS"]
    assert (MAX_HEIGHT - 1) // 10 + 1 == K["SSD_MAX_EDGE_PTS"] and MAX_HEIGHT // 10 + 1 > K["SSD_MAX_EDGE_PTS"]
    header = open(os.path.join(ROOT, "include", "ssd_hip.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for doc in (header, integration):
        assert re.search(r"width <= %d|W ≤ %d" % (MAX_WIDTH, MAX_WIDTH), doc)
        assert re.search(r"height <= %d|H ≤ %d" % (MAX_HEIGHT, MAX_HEIGHT), doc)
    assert _Z_XGA_IN * _XGA < FIXED_POINT_SUM <= _Z_XGA_OUT * _XGA
    assert n_bins(-0.1, _Z_XGA_OUT, 0.085) <= K["SSD_MAX_BINS"] and n_bins(-_Z_XGA_OUT, 0.1, 0.085) <= K["SSD_MAX_BINS"]
    assert n_bins(-0.1, Z_ABS, 16.1) <= K["SSD_MAX_BINS"] and (Z_ABS - 0.1) * _SMALL[0] * _SMALL[1] < FIXED_POINT_SUM


@pytest.mark.parametrize("name,at,past,names", LIMITS, ids=[r[0] for r in LIMITS])
def test_limit_accepted_at_and_refused_past(ssd, name, at, past, names):
    accepted = 0 if ssd.device_count() > 0 else E_NODEVICE
    rc, msg = _create(ssd, _config(ssd, at))
    assert rc == accepted, (name, "at the limit", rc, msg)
    rc, msg = _create(ssd, _config(ssd, past))
    assert rc == E_ARG, (name, "past the limit", rc, msg)
    assert names in msg, (name, msg)
