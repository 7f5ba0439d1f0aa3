"""k_predict counts exactly the points csrc/ssd_predict.h says it samples, each in the reference's height bin: the frame with every
other point blanked, through the oracle's complete histogram, equals FrameState::predSample bin for bin - on frames that end mid-line
and mid-point, at bases 0, 4, 8 and 12 bytes into a line, and on a cloud made for the band where single precision cannot call the bin
(the points the kernel hands to the reference's doubles).  tests/test_predict_sample.py checks the rule itself without a GPU."""
import numpy as np
import pytest

import oracle_binding as ob
import scenes
from test_gpu_quirks import _bin_edge_cloud

pytestmark = pytest.mark.gpu


def _upload(ssd, gpu_device, frames, stride):
    """frames [n, H, W, 3] float32 -> a device buffer with frame i at i * stride bytes"""
    n, nbytes = len(frames), frames[0].nbytes
    raw = np.zeros((n - 1) * stride + nbytes, dtype=np.uint8)
    for i in range(n):
        raw[i * stride:i * stride + nbytes] = frames[i].view(np.uint8).reshape(-1)
    buf = ssd.DeviceBuffer(raw.size, gpu_device)
    buf.upload(raw)
    return buf


def _check(ssd, oracle, det, cfg, calib, frames, buf, stride):
    n, (H, W) = len(frames), frames[0].shape[:2]
    det.single_pass(1)
    det.enqueue(buf.ptr, n, stride_bytes=stride)
    det.fetch(n)
    assert det.single_pass_stats(n)["ran"]
    for i in range(n):
        first, count = ssd.predict_sample_host(buf.ptr + i * stride, W * H)
        keep = np.zeros(W * H, dtype=bool)
        for f, c in zip(first, count):
            keep[f:f + c] = True
        assert abs(int(keep.sum()) - W * H / 16) <= 10
        only = frames[i].reshape(-1, 3).copy()
        only[~keep] = 0.0                                              # z = 0: no measurement (pointcloud.cpp:143-146)
        res, *_ = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(calib), only.reshape(H, W, 3), images=0, ground_images=False)
        want = np.array(res.hist[:ssd.MAX_BINS], dtype=np.uint32)
        got = det.single_pass_sample(i)
        assert int(want.sum()) > 0
        assert np.array_equal(got, want), ("frame %d at %d bytes into its line" % (i, (buf.ptr + i * stride) % 128), np.flatnonzero(got != want))


@pytest.mark.parametrize("W,H", [(256, 192), (427, 321)])
def test_the_kernel_counts_the_sampled_points_and_no_others(ssd, oracle, gpu_device, W, H):
    """four frames, back to back (256 x 192: every frame begins a line; 427 x 321: 4 bytes more than a whole number of lines, and
    12-byte loads) and at a stride 4 bytes longer, as tests/test_gpu_single_pass.py shifts its vertices"""
    n = 4
    sc = scenes.batch_scenes(ssd, W, H, n, base_seed=61000 + W, rng_seed=61)
    trans = ssd.transformation_for_scene(sc[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n)
    frames = ssd.synth_host(sc)
    det = ssd.Detector(cfg, trans, gpu_device)
    for stride in (W * H * 12, W * H * 12 + 4):
        buf = _upload(ssd, gpu_device, frames, stride)
        _check(ssd, oracle, det, cfg, trans.constants, frames, buf, stride)
        buf.free()
    det.close()


def test_sampled_points_on_bin_edges_take_the_doubles(ssd, oracle, gpu_device):
    """The cloud tests/test_gpu_quirks.py makes for the band around the bin edges (world z on every edge of a height bin, plus or minus
    nothing .. 1e-3 of a bin), put where the kernel samples: the single-precision bin is wrong for some of them unless the band goes to
    the doubles (a build with -DSSD_SABOTAGE_PRE=1 fails here: profiles/predict_whole_lines.txt)."""
    W, H = 640, 480
    sc = ssd.make_scene(W, H, n_steps=2, seed=78, pitch_deg=46.0, roll_deg=-2.5, yaw_deg=-9.0, sigma=0.001)
    trans = ssd.transformation_for_scene(sc)
    cfg = ssd.default_config(W, H, max_frames_per_batch=1)
    a = np.array(list(trans.constants.a), dtype=np.float64).reshape(3, 3)
    b = np.array(list(trans.constants.b), dtype=np.float64)
    rng = np.random.default_rng(6)
    xyz = ssd.synth_host([sc])[0].reshape(-1, 3).copy()
    buf = ssd.DeviceBuffer(xyz.nbytes, gpu_device)
    first, count = ssd.predict_sample_host(buf.ptr, W * H)
    sampled = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)])
    edges = _bin_edge_cloud(cfg, a, b, rng, 150)
    edges = edges[rng.permutation(len(edges))[:len(sampled)]]
    assert len(edges) > len(sampled) * 3 // 4
    xyz[rng.permutation(sampled)[:len(edges)]] = edges
    frames = xyz.reshape(1, H, W, 3)
    buf.upload(frames)
    det = ssd.Detector(cfg, trans, gpu_device)
    _check(ssd, oracle, det, cfg, trans.constants, frames, buf, xyz.nbytes)
    det.close()
    buf.free()
