#!/usr/bin/env python3
"""tools/depth_fill_time.py [ROUNDS] [OUT] - what the depth fill (k_depth_fill) costs beside its yardsticks, by the
method of tools/depth_edges_time.py: one resident batch of XGA x 256 16-bit depth frames (3 steps, sigma 2 mm, 5 % outliers, 2 % invalid,
seeds 1000 ..; 403 MB), bench.py's half-second warm-up, then ROUNDS (15) rounds of every leg once, so the legs alternate; median with
min .. max.
The legs: the plain read (ssd.stream_read_ms, its own device events); k_depth_fuse at n = 1, hop = 1, which reads and writes the same
bytes with no neighbours; k_depth_edges wide and narrow (the same frames at a pointer and strides that are multiples of 2 only) - the
yardstick: the same stencil skeleton over the same bytes in the same visit; k_depth_fill wide and narrow, each with and without the class
map and with cover 0 and 1; and the chain warp + fill + fuse n = 8 + detection of the 32 fused frames beside warp + fuse + detection, on
one stream with no host wait, under a seeded small-motion view per frame.
Every leg but the read is timed by a host clock around the enqueue and the fetch that waits for it; a stand-alone pass's own device events
(the zeroing of its records and their copy included) stand beside it in [..], and the multiples come from them.  Frame 0 is checked
against ssd_depth_fill_host, as it is and warped.  Nothing is fixed in advance: the figures are what they are.
Writes profiles/depth_fill_time.txt (or OUT).  TEST INFRASTRUCTURE."""
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
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "depth_fill_time.txt")
    scs = [ssd.make_scene(W, H, n_steps=3, seed=1000 + i, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02) for i in range(F)]
    trans, intr = ssd.transformation_for_scene(scs[0]), ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    frame = W * H * 2
    nbytes = F * frame
    det = ssd.Detector(cfg, trans, 0)
    # the narrow legs: the same frames 2 bytes further on, at strides 6 bytes wider
    nstride = frame + 6
    buf, out, cls = ssd.DeviceBuffer(nbytes, 0), ssd.DeviceBuffer(2 + F * nstride, 0), ssd.DeviceBuffer(8 + F * (frame // 2 + 3), 0)
    nbuf, mid, warped = ssd.DeviceBuffer(2 + F * nstride, 0), ssd.DeviceBuffer(F // 8 * frame, 0), ssd.DeviceBuffer(nbytes, 0)
    small = (ssd.WarpView * F)(*wm.seeded_views(ssd, intr, F, seed=11, max_deg=1.0, max_shift=0.03))
    no_cover = ssd.depth_fill_default_rule()
    no_cover.cover = 0
    lines = ["# tools/depth_fill_time.py %d: XGA x %d resident depth frames (%d bytes), %d timed rounds, every leg once per round" % (rounds, F, nbytes, rounds),
             "# ms per leg, median (min .. max): host clock around enqueue and fetch; [..]: the leg's own device events; x read / x edges: the multiple",
             "# of the plain read's median and of k_depth_edges' median at the same alignment (the chains: wide); GB/s: bytes of input the leg reads per second"]
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

        def stencil(enqueue, fetch, took, wide, classes, rule=None):
            src, dst, stride = (buf.ptr, out.ptr, frame) if wide else (nbuf.ptr + 2, out.ptr + 2, nstride)
            c = None if not classes else cls.ptr if wide else cls.ptr + 1
            host = clock(lambda: enqueue(src, F, dst, rule, c, stride, stride, frame // 2 if wide else frame // 2 + 3), lambda: fetch(1))
            return host, took(), nbytes

        def edges(wide, classes=False):
            return stencil(det.enqueue_depth_edges, det.fetch_depth_edges, det.depth_edges_time_ms, wide, classes)

        def fill(wide, classes, rule=None):
            return stencil(det.enqueue_depth_fill, det.fetch_depth_fill, det.depth_fill_time_ms, wide, classes, rule)

        def chain(with_fill):
            def go():
                det.enqueue_depth_warp(buf.ptr, F, small, intr, warped.ptr, frame, frame)
                if with_fill:
                    det.enqueue_depth_fill(warped.ptr, F, out.ptr)
                groups = det.enqueue_depth_fuse(out.ptr if with_fill else warped.ptr, F, 8, mid.ptr)
                det.enqueue_depth(mid.ptr, groups)
            return clock(go, lambda: det.fetch(F // 8)), None, nbytes

        legs = [("plain read", lambda: (None, ssd.stream_read_ms(buf.ptr, nbytes, reps=1), nbytes)),
                ("k_depth_fuse n 1 hop 1", fuse1),
                ("k_depth_edges wide", lambda: edges(True)),
                ("k_depth_edges narrow", lambda: edges(False))]
        for wide in (True, False):
            for classes in (False, True):
                for rule, rname in ((None, "cover 1"), (no_cover, "cover 0")):
                    legs.append(("k_depth_fill %s%s, %s" % ("wide" if wide else "narrow", " + class map" if classes else "", rname),
                                 lambda wide=wide, classes=classes, rule=rule: fill(wide, classes, rule)))
        legs += [("warp + fuse n 8 + detect 32 frames", lambda: chain(False)),
                 ("warp + fill + fuse n 8 + detect 32 frames", lambda: chain(True))]

        def one_round():
            return [leg() for _, leg in legs]
        c0 = time.perf_counter()
        while time.perf_counter() - c0 < 0.5:                              # bench.py's warm-up: load until the device has been busy a while
            one_round()
        took = [one_round() for _ in range(rounds)]
        read = statistics.median(r[0][1] for r in took)
        yard = {True: statistics.median(r[2][1] for r in took), False: statistics.median(r[3][1] for r in took)}
        for k, (name, _) in enumerate(legs):
            host = [r[k][0] for r in took if r[k][0] is not None]
            dev = [r[k][1] for r in took if r[k][1] is not None]
            moved = took[0][k][2]
            best = statistics.median(dev) if dev else statistics.median(host)
            cells = ["%-44s" % name]
            cells.append("%8.3f (%.3f .. %.3f)" % (statistics.median(host), min(host), max(host)) if host else "%8s" % "-")
            cells.append("[%.3f (%.3f .. %.3f)]" % (statistics.median(dev), min(dev), max(dev)) if dev else "[-]")
            cells.append("%.2f x read, %.2f x edges, %.0f GB/s" % (best / read, best / yard["narrow" not in name], moved / best / 1e6))
            lines.append("  ".join(cells))
        # the bytes: frame 0 against the host statement, as it is and behind the warp
        first = ssd.synth_depth_host(scs[:1])[0]
        for name, src_frame in (("the frame as it is", first), ("the warped frame", ssd.depth_warp_host(first, small[0], intr)[0])):
            if src_frame is first:
                det.enqueue_depth_fill(buf.ptr, F, out.ptr, None, cls.ptr)
            else:
                det.enqueue_depth_warp(buf.ptr, F, small, intr, warped.ptr, frame, frame)
                det.enqueue_depth_fill(warped.ptr, F, out.ptr, None, cls.ptr)
            stats = det.fetch_depth_fill(1)[0]
            got = out.download(frame, dtype=np.uint16).reshape(H, W)
            gotc = cls.download(frame // 2).reshape(H, W)
            want, want_stats, wantc = ssd.depth_fill_host(src_frame, classes=True)
            same = bool((got == want).all()) and bool((gotc == wantc).all()) and bytes(stats) == bytes(want_stats)
            bad += 0 if same else 1
            lines.append("frame 0 equal to ssd_depth_fill_host on %s, frame, class map and record: %s (of %d pixels %d kept, %d empty, %d filled, %d covered)"
                         % (name, same, W * H, stats.n_kept, stats.n_empty, stats.n_filled, stats.n_covered))
    finally:
        for b in (buf, out, cls, nbuf, mid, warped):
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
