#!/usr/bin/env python3
"""tools/depth_warp_time.py [ROUNDS] [OUT] - what the depth warp (k_depth_warp) costs beside its yardsticks, by the
method of tools/depth_edges_time.py: one resident batch of XGA x 256 16-bit depth frames (3 steps, sigma 2 mm, 5 % outliers, 2 % invalid,
seeds 1000 ..; 403 MB), bench.py's half-second warm-up, then ROUNDS (15) rounds of every leg once, so the legs alternate; median with
min .. max.
The legs: the plain read (ssd.stream_read_ms, its own device events); k_depth_fuse at n = 1, hop = 1, which reads and writes the same
bytes and is the yardstick the edge filter used; k_depth_warp under a seeded small-motion view per frame, wide and narrow (the same frames
at a pointer and strides that are multiples of 2 only), under the identity, and under the push-away view, the contention case; the chain
fuse n = 8 + detection of the 32 fused frames, and warp + fuse n = 8 + detection beside it, on one stream with no host wait.
Every leg but the read is timed by a host clock around the enqueue and the fetch that waits for it; a stand-alone pass's own device events
(the zeroing of its output and records and their copy included, the views' upload not) stand beside it in [..], and the multiples come from
them.  Frame 0 is checked against ssd_depth_warp_host.  Nothing is fixed in advance: the figures are what they are.
Writes profiles/depth_warp_time.txt (or OUT).  TEST INFRASTRUCTURE."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import numpy as np  # noqa: E402
import warp_model as wm  # noqa: E402

W, H, F = 1024, 768, 256


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "depth_warp_time.txt")
    scs = [ssd.make_scene(W, H, n_steps=3, seed=1000 + i, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02) for i in range(F)]
    trans, intr = ssd.transformation_for_scene(scs[0]), ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    frame = W * H * 2
    nbytes = F * frame
    det = ssd.Detector(cfg, trans, 0)
    nstride, ostride = frame + 6, frame + 4                                 # the narrow leg: the input off 16 bytes, the output on 4
    buf, out, mid = ssd.DeviceBuffer(nbytes, 0), ssd.DeviceBuffer(4 + F * ostride, 0), ssd.DeviceBuffer(F // 8 * frame, 0)
    nbuf = ssd.DeviceBuffer(2 + F * nstride, 0)
    table = lambda views: (ssd.WarpView * F)(*views)                                                   # noqa: E731
    small = table(wm.seeded_views(ssd, intr, F, seed=11, max_deg=1.0, max_shift=0.03))
    ident, push = table([wm.identity_view(ssd, intr)] * F), table([wm.push_away_view(ssd, intr)] * F)
    lines = ["# tools/depth_warp_time.py %d: XGA x %d resident depth frames (%d bytes), %d timed rounds, every leg once per round" % (rounds, F, nbytes, rounds),
             "# ms per leg, median (min .. max): host clock around enqueue and fetch; [..]: the leg's own device events; x read / x fuse1: the multiple",
             "# of the plain read's and of k_depth_fuse n = 1's median; GB/s: bytes of input the leg reads per second"]
    bad = 0
    try:
        det.set_intrinsics(intr)
        det.set_timing(True)
        ssd.synth_depth_device(scs, buf.ptr, device=0)
        ssd.lib().ssd_device_sync(0)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
        assert hip.hipMemcpy2D(nbuf.ptr + 2, nstride, buf.ptr, frame, frame, F, 3) == 0         # device to device

        def clock(fn, fetch):
            t0 = time.perf_counter()
            fn()
            fetch()
            return (time.perf_counter() - t0) * 1e3

        def fuse1():
            host = clock(lambda: det.enqueue_depth_fuse(buf.ptr, F, 1, out.ptr, 1), lambda: det.fetch_depth_fuse(1))
            return host, det.depth_fuse_time_ms(), nbytes

        def warp(views, wide=True):
            src, dst, stride, ostr = (buf.ptr, out.ptr, frame, frame) if wide else (nbuf.ptr + 2, out.ptr + 4, nstride, ostride)
            host = clock(lambda: det.enqueue_depth_warp(src, F, views, intr, dst, stride, ostr), lambda: det.fetch_depth_warp(1))
            return host, det.depth_warp_time_ms(), nbytes

        def fuse_detect():
            def go():
                groups = det.enqueue_depth_fuse(buf.ptr, F, 8, mid.ptr)
                det.enqueue_depth(mid.ptr, groups)
            return clock(go, lambda: det.fetch(F // 8)), None, nbytes

        def warp_fuse_detect():
            def go():
                det.enqueue_depth_warp(buf.ptr, F, small, intr, out.ptr, frame, frame)
                groups = det.enqueue_depth_fuse(out.ptr, F, 8, mid.ptr)
                det.enqueue_depth(mid.ptr, groups)
            return clock(go, lambda: det.fetch(F // 8)), None, nbytes

        legs = [("plain read", lambda: (None, ssd.stream_read_ms(buf.ptr, nbytes, reps=1), nbytes)),
                ("k_depth_fuse n 1 hop 1", fuse1),
                ("k_depth_warp small motion, wide", lambda: warp(small)),
                ("k_depth_warp small motion, narrow", lambda: warp(small, False)),
                ("k_depth_warp identity", lambda: warp(ident)),
                ("k_depth_warp push-away (contention)", lambda: warp(push)),
                ("fuse n 8 + detect 32 frames", fuse_detect),
                ("warp + fuse n 8 + detect 32 frames", warp_fuse_detect)]

        def one_round():
            return [leg() for _, leg in legs]
        c0 = time.perf_counter()
        while time.perf_counter() - c0 < 0.5:                              # bench.py's warm-up: load until the device has been busy a while
            one_round()
        took = [one_round() for _ in range(rounds)]
        read = statistics.median(r[0][1] for r in took)
        yard = statistics.median(r[1][1] for r in took)
        for k, (name, _) in enumerate(legs):
            host = [r[k][0] for r in took if r[k][0] is not None]
            dev = [r[k][1] for r in took if r[k][1] is not None]
            moved = took[0][k][2]
            best = statistics.median(dev) if dev else statistics.median(host)
            cells = ["%-40s" % name]
            cells.append("%8.3f (%.3f .. %.3f)" % (statistics.median(host), min(host), max(host)) if host else "%8s" % "-")
            cells.append("[%.3f (%.3f .. %.3f)]" % (statistics.median(dev), min(dev), max(dev)) if dev else "[-]")
            cells.append("%.2f x read, %.2f x fuse1, %.0f GB/s" % (best / read, best / yard, moved / best / 1e6))
            lines.append("  ".join(cells))
        # the bytes: frame 0 against the host statement, under the small motion and pushed away
        first = ssd.synth_depth_host(scs[:1])[0]
        for name, views in (("small motion", small), ("push-away", push)):
            det.enqueue_depth_warp(buf.ptr, F, views, intr, out.ptr, frame, frame)
            stats = det.fetch_depth_warp(1)[0]
            got = out.download(frame, dtype=np.uint16).reshape(H, W)
            want, want_stats = ssd.depth_warp_host(first, views[0], intr)
            same = bool((got == want).all()) and bytes(stats) == bytes(want_stats)
            bad += 0 if same else 1
            lines.append("frame 0 equal to ssd_depth_warp_host under the %s view, frame and record: %s (%d of %d samples landed on %d pixels)"
                         % (name, same, stats.n_landed, W * H, stats.n_filled))
    finally:
        for b in (buf, out, mid, nbuf):
            b.free()
        det.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
