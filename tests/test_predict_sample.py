"""k_predict's sample of a vertex frame (csrc/ssd_predict.h: predict_sample_run, run on the host through the test hook): the points that
lie wholly inside one 128-byte line of memory out of every fifteen consecutive lines.  No GPU: the rule's properties on every geometry of
tests/test_gpu_single_pass.py::test_single_pass_forced_on_small_batches (128 x 100 and 427 x 321 end mid-line and mid-point) at frame
bases 0, 4 and 8 bytes into a line; tests/test_gpu_predict_sample.py checks that the kernel counts exactly these points."""
import numpy as np
import pytest

SAMPLE = 16          # kSpecSample: a sample count stands for 16 points
LINE = 128           # bytes
POINT = 12
LINE_POINTS = 10     # whole points in a line, wherever it starts in a point
BASE = 0x7F3A00000000                      # a multiple of 128: only the base's place in its line matters
GEOMETRIES = [(1024, 768), (512, 384), (256, 192), (640, 480), (848, 480), (1280, 720), (1920, 1080), (600, 450), (427, 321), (128, 100)]


def _sampled(ssd, base, n):
    first, count = ssd.predict_sample_host(base, n)
    assert len(first) == len(count) >= 1
    idx = np.concatenate([np.arange(f, f + c, dtype=np.int64) for f, c in zip(first, count)])
    return first.astype(np.int64), count.astype(np.int64), idx


@pytest.mark.parametrize("shift", [0, 4, 8])
@pytest.mark.parametrize("W,H", GEOMETRIES)
def test_sampled_points_lie_in_whole_lines_once_and_are_a_sixteenth(ssd, W, H, shift):
    n, base = W * H, BASE + shift
    first, count, idx = _sampled(ssd, base, n)
    # inside the frame, and wholly inside ONE line: the first byte of a run's first point and the last byte of its last
    assert idx.min() >= 0 and idx.max() < n
    assert (count >= 0).all() and (count <= LINE_POINTS).all()
    some = count > 0
    lo = (base + POINT * first[some]) // LINE
    hi = (base + POINT * (first[some] + count[some]) - 1) // LINE
    assert (lo == hi).all()
    # one line of every group of fifteen, counted from the line the frame begins in; groups ascend
    groups = np.arange(len(first))[some]
    in_group = lo - (base // LINE + 15 * groups)
    assert (in_group >= 0).all() and (in_group < 15).all()
    # the place in the group varies: it creeps by a sixth of a line per group, so G groups take min(15, G // 7) places at the least
    assert len(np.unique(in_group)) >= min(15, len(groups) // 7)
    # a line that lies wholly inside the frame gives all ten of its points
    whole = (LINE * lo >= base) & (LINE * (lo + 1) <= base + POINT * n)
    assert (count[some][whole] == LINE_POINTS).all()
    # no point twice
    assert len(np.unique(idx)) == len(idx)
    # a sixteenth of the points, give or take one group's ten
    assert abs(len(idx) - n / SAMPLE) <= LINE_POINTS, (len(idx), n / SAMPLE)
    # a group for every fifteen lines the frame touches, the last one short
    lines = (base % LINE + POINT * n + LINE - 1) // LINE
    assert len(first) == (lines + 14) // 15


@pytest.mark.parametrize("shift", [0, 4, 8])
@pytest.mark.parametrize("W,H", [g for g in GEOMETRIES if g[0] >= 256])
def test_every_band_of_columns_gets_its_share(ssd, W, H, shift):
    """The sampled line's place in its group must not lock onto the camera's columns (an XGA row is 96 lines and 96 mod 15 = 6): every
    band of 64 columns - the last one narrower where 64 does not divide the width - receives between 0.75 and 1.25 of its even share."""
    _, _, idx = _sampled(ssd, BASE + shift, W * H)
    bands = -(-W // 64)
    got = np.bincount((idx % W) // 64, minlength=bands).astype(np.float64)
    width = np.minimum(64, W - 64 * np.arange(bands))
    share = len(idx) * width / W
    ratio = got / share
    assert ratio.min() >= 0.75 and ratio.max() <= 1.25, (ratio.min(), ratio.max())


def test_the_hook_refuses_what_the_rule_is_not_stated_for(ssd):
    with pytest.raises(ssd.SsdError):
        ssd.predict_sample_host(BASE, 0)
    with pytest.raises(ssd.SsdError):
        ssd.predict_sample_host(BASE, (1 << 26) + 1)
    first, count = ssd.predict_sample_host(BASE + 4, 3)          # a frame shorter than a line: its three points, once
    assert list(first) == [0] and list(count) == [3]
