"""The depth fusion's host statement (ssd_depth_fuse_default_rule, ssd_depth_fuse_host; include/ssd_hip.h) on the CPU:
against tests/fuse_model.py, the rule in numpy written from its text, byte for byte on frame, support and record; on a frame built for
the rule's edges, one pixel per case with what the text says must come out; on the conditions the figures of
profiles/depth_fuse_accuracy.txt meet; and end to end through the CPU oracle.  No GPU is needed: tests/test_gpu_depth_fuse.py holds the
kernel to this statement."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import fuse_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 3, 5, 8, 13, 16)


def test_exports_and_structure_sizes(ssd):
    names = ("ssd_depth_fuse_default_rule", "ssd_depth_fuse_host", "ssd_enqueue_depth_fuse", "ssd_fetch_depth_fuse", "ssd_get_depth_fuse_time",
             "ssd_process_depth_host_fused")
    assert all(n in ssd.EXPORTS and hasattr(ssd.lib(), n) for n in names)
    assert C.sizeof(ssd.FuseStats) == 64 and C.sizeof(ssd.FuseRule) == 16
    assert [f for f, _ in ssd.FuseStats._fields_] == list(fm.STATS)
    assert (ssd.FUSE_MAX_FRAMES, ssd.FUSE_TOL) == (16, 40)


def test_the_default_rule(ssd):
    for n in range(1, 17):
        r = ssd.depth_fuse_default_rule(n)
        assert (r.min_valid, r.min_agree, r.tol, r.reserved) == ((n + 1) // 2, (n + 1) // 2, 40, 0) == fm.default_rule(n) + (0,)
    for n in (0, -1, 17):
        with pytest.raises(ssd.SsdError):
            ssd.depth_fuse_default_rule(n)
    assert ssd.lib().ssd_depth_fuse_default_rule(3, None) == -1


def test_every_refusal_of_the_host_statement(ssd):
    L = ssd.lib()
    f = np.full((2, 2, 3), 100, np.uint16)
    out, sup, st = np.zeros(6, np.uint16), np.zeros(6, np.uint8), ssd.FuseStats()
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                                   # noqa: E731

    def call(w=3, h=2, frames=p(f), stride=12, n=2, rule=None, o=p(out), s=p(sup), stats=C.byref(st)):
        return L.ssd_depth_fuse_host(w, h, frames, stride, n, None if rule is None else C.byref(rule), o, s, stats)
    R = ssd.FuseRule
    refused = [call(frames=None), call(o=None), call(stats=None), call(w=0), call(h=0), call(w=-3), call(n=0), call(n=17), call(stride=10),
               call(stride=13), call(rule=R(0, 1, 40, 0)), call(rule=R(3, 1, 40, 0)), call(rule=R(1, 0, 40, 0)), call(rule=R(1, 3, 40, 0)),
               call(rule=R(1, 1, -1, 0)), call(rule=R(1, 1, 65536, 0))]
    assert refused == [-1] * len(refused)
    assert b"ssd_depth_fuse_host" in L.ssd_last_error()
    assert call() == 0 and call(s=None) == 0 and call(rule=R(2, 2, 0, 0)) == 0 and call(rule=R(1, 1, 65535, 0)) == 0
    assert call(n=1, stride=0) == 0, "one frame: any even stride"
    assert st.n_fused == 6 and (out == 100).all()


@pytest.fixture(scope="module")
def scene16(ssd):
    return fm.scene_frames(ssd, 64, 48, 16)


@pytest.mark.parametrize("n", NS)
def test_the_host_statement_equals_the_model_on_the_scene(ssd, scene16, n):
    frames = np.ascontiguousarray(scene16[:n])
    want_o, want_s, want_st = fm.fuse_np(frames)
    out, st, sup = ssd.depth_fuse_host(frames, support=True)
    assert (out == want_o).all() and (sup == want_s).all() and fm.stats_dict(st) == want_st
    out2, st2 = ssd.depth_fuse_host(frames)                                      # support NULL
    assert (out2 == out).all() and bytes(st2) == bytes(st)
    # a padded stride: the frames 6 bytes apart from packed, and the bytes between them poisoned
    fb = 64 * 48 * 2
    padded = np.full(n * (fb + 6), 0xEE, np.uint8)
    for j in range(n):
        padded[j * (fb + 6):j * (fb + 6) + fb] = frames[j].reshape(-1).view(np.uint8)
    view = np.lib.stride_tricks.as_strided(padded[:fb].view(np.uint16), shape=(n, 48, 64), strides=(fb + 6, 128, 2), writeable=False)
    out3, st3, sup3 = ssd.depth_fuse_host(view, support=True, stride_bytes=fb + 6)
    assert (out3 == out).all() and (sup3 == sup).all() and bytes(st3) == bytes(st)
    assert want_st["n_fused"] + want_st["n_empty"] + want_st["n_few"] + want_st["n_split"] == 64 * 48
    tight = (n, n, 3)
    o4, s4, st4 = fm.fuse_np(frames, tight)
    out4, stats4, sup4 = ssd.depth_fuse_host(frames, fm.rule_of(ssd, tight), support=True)
    assert (out4 == o4).all() and (sup4 == s4).all() and fm.stats_dict(stats4) == st4


@pytest.mark.parametrize("n", NS)
def test_the_edge_frame_equals_the_model(ssd, n):
    for k, rule in enumerate([None, (1, 1, 0), (n, n, 40), (1, n, 65535), ((n + 1) // 2, 1, 1)]):
        frames, names = fm.edge_frame(n, rule or fm.default_rule(n), 16, 9, seed=k)
        want_o, want_s, want_st = fm.fuse_np(frames, rule)
        out, st, sup = ssd.depth_fuse_host(frames, fm.rule_of(ssd, rule), support=True)
        bad = [names[p] if p < len(names) else "pixel %d" % p for p in np.flatnonzero((out != want_o).reshape(-1) | (sup != want_s).reshape(-1))]
        assert not bad, "n %d rule %s: %s" % (n, rule, bad)
        assert fm.stats_dict(st) == want_st
        assert st.n_fused + st.n_empty + st.n_few + st.n_split == 16 * 9 and st.reserved == 0


def _one(ssd, samples, n, rule):
    """one pixel: its samples (the rest of the n invalid, in an order that is not sorted) -> (output, support, class)"""
    col = np.array(fm._column(n, samples), np.uint16).reshape(n, 1, 1)
    out, st, sup = ssd.depth_fuse_host(col, ssd.FuseRule(*rule, 0), support=True)
    cls = [k for k in ("n_fused", "n_empty", "n_few", "n_split") if getattr(st, k)]
    assert len(cls) == 1 and int(st.sum_valid) == sum(1 for s in samples if s)
    return int(out[0, 0]), int(sup[0, 0]), cls[0][2:]


@pytest.mark.parametrize("n", (3, 4, 8, 16))
def test_the_rules_edges_by_hand(ssd, n):
    """what the rule's text says must come out, one pixel per case, stated here and not taken from any implementation"""
    k = (n + 1) // 2
    rule = (k, k, 40)
    one = lambda samples, r=rule: _one(ssd, samples, n, r)                                        # noqa: E731
    assert one([]) == (0, 0, "empty")
    assert one([20000] * (k - 1)) == ((0, 0, "few") if k > 1 else (0, 0, "empty"))
    assert one([20000] * k) == (20000, k, "fused")
    # all n valid, the median in a camp of min_agree - 1 resp. min_agree equal samples, everybody else far from it and from each other
    def camp(size):
        below = (n - 1) // 2 - (size - 1)
        return [1000 + 1000 * i for i in range(below)] + [20000] * size + [40000 + 1000 * i for i in range(n - below - size)]
    assert one(camp(k - 1)) == (0, 0, "split")
    assert one(camp(k)) == (20000, k, "fused")
    # exactly tol away agrees, tol + 1 does not, on both sides (k samples at the median, one beside them)
    if n > k:
        base = [30000] * k
        assert one(base + [30040]) == ((2 * (30000 * k + 30040) + k + 1) // (2 * (k + 1)), k + 1, "fused")
        assert one(base + [30041]) == (30000, k, "fused")
        assert one(base + [29960]) == ((2 * (30000 * k + 29960) + k + 1) // (2 * (k + 1)), k + 1, "fused")
        assert one(base + [29959]) == (30000, k, "fused")
        # a difference that wraps in 16 bits would come back small: 3 against 65500 is 65497 away, not 39
        assert one([3] * k + [65500]) == (3, k, "fused")
        assert one([65534] * k + [1]) == (65534, k, "fused")
    # tol = 0: only the median's duplicates agree
    assert one([500, 700, 700][:n], (1, 1, 0)) == (700, 2, "fused")
    assert one([500, 700][:n], (1, 1, 0)) == (500, 1, "fused"), "even m: the LOWER median"
    assert one([500, 700][:n], (1, 2, 40)) == (0, 0, "split"), "... and the upper one does not agree with it"
    if n >= 4:
        assert one([1000, 1010, 2000, 2010], (1, 1, 40)) == (1005, 2, "fused"), "m = 4: the median is the second smallest"
        assert one([500, 700, 700, 700, 900][:n], (1, 1, 0))[:2] == (700, 3)
    # a mean that ends in exactly one half rounds up, with even and with odd c
    assert one([1000, 1001], (1, 1, 40)) == (1001, 2, "fused")
    assert one([1000, 1000, 1003][:n], (1, 1, 40))[:2] == (1001, 3), "3003 / 3 = 1001 exactly"
    if n >= 4:
        assert one([10, 11, 11, 12], (1, 1, 40)) == (11, 4, "fused")
        assert one([10, 10, 11, 11], (1, 1, 40)) == (11, 4, "fused"), "10.5 -> 11"
    if n >= 6:
        assert one([10, 10, 10, 11, 11, 11], (1, 1, 40)) == (11, 6, "fused")
    assert one([7, 8, 8][:n], (1, 1, 40)) == (8, 3, "fused"), "23 / 3 = 7.67 -> 8"
    assert one([7, 7, 8][:n], (1, 1, 40)) == (7, 3, "fused"), "22 / 3 = 7.33 -> 7"
    # the ends of the range
    assert one([1] * k) == (1, k, "fused")
    assert one([65535] * k) == (65535, k, "fused")
    assert one([65535] * n, (n, n, 0)) == (65535, n, "fused")
    # a median within tol of 65535 while invalid samples are present: an implementation that lets a sentinel 0xFFFF agree counts too many
    if n > k:
        assert one([65530] * k) == (65530, k, "fused")
        assert one([65530] * (k - 1) + [65535]) == ((2 * (65530 * (k - 1) + 65535) + k) // (2 * k), k, "fused")
    assert one([65535], (1, 1, 40)) == (65535, 1, "fused")
    assert one([1], (1, 1, 65535)) == (1, 1, "fused")


@pytest.fixture(scope="module")
def table_row(ssd):
    frames = fm.scene_frames(ssd, fm.ACC_W, fm.ACC_H, fm.ACC_N)
    return frames, fm.clean_frame(ssd, fm.ACC_W, fm.ACC_H)


def test_the_tables_numbers_as_conditions(ssd, table_row):
    """256 x 192, seeds 1000 .. 1007, sigma 2 mm, 5 % outliers, 2 % invalid, n = 8, the default rule, against the sigma = 0 frame.  Measured
    (profiles/depth_fuse_accuracy.txt): far pixels 5.06 % -> none, invalid 1.90 % -> 0.02 %, rms 8.04 -> 2.98 raw units"""
    frames, clean = table_row
    fused, stats = ssd.depth_fuse_host(frames)
    assert (fused == fm.fuse_np(frames)[0]).all()
    single, got = fm.pixel_figures(frames[0], clean), fm.pixel_figures(fused, clean)
    print("far %.4f -> %.4f, rms %.3f -> %.3f, invalid %.4f -> %.4f" % (single[0], got[0], single[1], got[1], single[2], got[2]))
    assert single[0] > 0.04, "the single frame carries its outliers"
    assert got[0] <= 0.001, "at most 0.1 % of the fused pixels lie more than 40 raw units from the clean frame"
    assert got[2] < single[2], "fewer fused pixels are invalid than in the single frame"
    assert got[1] <= 0.5 * single[1], "the rms error of the remaining pixels is at most half the single frame's"
    assert got[1] >= single[1] / math.sqrt(8) * 0.9, "(1 / sqrt(8) is the floor)"
    assert stats.n_fused == int((fused != 0).sum())


def test_end_to_end_through_the_oracle(ssd, oracle):
    d = fm.detection_figures(ssd, oracle)
    print(d)
    assert d["clean_steps"] == 3
    wrong = [i for i, n in enumerate(d["single_steps"]) if n != d["clean_steps"]]
    right = [e for i, e in enumerate(d["single_worst"]) if i not in wrong]
    # (the oracle reports all three steps for every single frame here: profiles/depth_fuse_accuracy.txt; the step-count half of the
    # comparison binds only for frames it gets wrong)
    assert d["fused_steps"] == d["clean_steps"]
    assert not right or d["fused_worst"] <= max(right), "the fused frame's worst step height error is no larger than the worst single frame's"
    assert math.isfinite(d["fused_worst"])


def test_the_recorded_accuracy_is_this_codes(ssd):
    """profiles/depth_fuse_accuracy.txt's rows, computed again"""
    path = os.path.join(ROOT, "profiles", "depth_fuse_accuracy.txt")
    rows = [l for l in open(path).read().splitlines() if l and l[0] == " "]
    got = fm.accuracy_rows(ssd)
    assert len(rows) == len(got)
    for line, r in zip(rows, got):
        s, f = r["single"], r["fused"]
        cells = [c.split() for c in line.split("|")]
        assert int(cells[0][3]) == r["n"]
        assert [cells[1][0], cells[1][2]] == ["%.3f" % (100 * s[0]), "%.3f" % (100 * f[0])]
        assert [cells[2][0], cells[2][2]] == ["%.2f" % s[1], "%.2f" % f[1]]
        assert [cells[3][0], cells[3][2]] == ["%.2f" % (100 * s[2]), "%.2f" % (100 * f[2])]


def test_the_sanitizer_program_runs_clean():
    """tools/host_sanitize.sh depth_fuse: csrc/ssd_host.cpp and a stand-alone program under AddressSanitizer and UBSan, on the CPU"""
    import shutil
    if shutil.which("hipconfig") is None:
        pytest.skip("hipconfig is not installed")
    run = subprocess.run(["bash", os.path.join(ROOT, "tools", "host_sanitize.sh"), "depth_fuse"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "depth fusion host functions: clean" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
