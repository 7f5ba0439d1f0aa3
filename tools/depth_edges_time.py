#!/usr/bin/env python3
"""tools/depth_edges_time.py [ROUNDS] [OUT] [PARENT_LIB] - what the depth edge filter (k_depth_edges) costs beside its
yardstick, by the method of tools/depth_fuse_time.py: one resident batch of XGA x 256 16-bit depth frames (3 steps, sigma 2 mm, 5 %
outliers, 2 % invalid, seeds 1000 ..; 403 MB), bench.py's half-second warm-up, then ROUNDS (15) rounds of every leg once, so the legs
alternate; median with min .. max.
The legs: the plain read (ssd.stream_read_ms, its own device events); k_depth_fuse at n = 1, hop = 1 - it reads and writes the same bytes
with no neighbours, so it is the yardstick - from this build and, where PARENT_LIB names the parent commit's libssd_hip.so, from that
build through a handle of its own, the two alternating; k_depth_edges wide and narrow (the same frames at a pointer and strides that are
multiples of 2 only), with and without the class map; the detection of the 256 frames alone and behind the filter on one stream with no
host wait; the chain fuse n = 8 + filter + detection of the 32 fused frames.
Every leg but the read is timed by a host clock around the enqueue and the fetch that waits for it; a stand-alone pass's own device
events (the zeroing of its records and their copy included) stand beside it in [..], and the multiples come from them.  Frame 0 is checked
against ssd_depth_edges_host.  Nothing is fixed in advance: the figures are what they are.
Writes profiles/depth_edges_time.txt (or OUT).  TEST INFRASTRUCTURE."""
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

W, H, F = 1024, 768, 256


class ParentFuse:
    """a handle of the parent commit's library, for its k_depth_fuse alone"""

    def __init__(self, path, cfg, trans):
        vp, i32, sz = C.c_void_p, C.c_int32, C.c_size_t
        self.L = L = C.CDLL(path)
        L.ssd_create.argtypes = [C.POINTER(ssd.Config), C.POINTER(ssd.Calibration), i32, C.POINTER(vp)]
        L.ssd_destroy.argtypes = [vp]
        L.ssd_set_timing.argtypes = [vp, i32]
        L.ssd_enqueue_depth_fuse.argtypes = [vp, vp, sz, i32, vp, i32, i32, vp, vp, sz, vp, sz]
        L.ssd_fetch_depth_fuse.argtypes = [vp, C.POINTER(ssd.FuseStats), i32, vp]
        L.ssd_get_depth_fuse_time.argtypes = [vp, C.POINTER(C.c_float)]
        self.h = vp()
        cal = trans.constants
        assert L.ssd_create(C.byref(cfg), C.byref(cal), 0, C.byref(self.h)) == 0
        assert L.ssd_set_timing(self.h, 1) == 0

    def fuse1(self, src, out, frame):
        st, ms = (ssd.FuseStats * 1)(), C.c_float()
        t0 = time.perf_counter()
        assert self.L.ssd_enqueue_depth_fuse(self.h, src, frame, F, None, 1, 1, None, out, frame, None, 0) == 0
        assert self.L.ssd_fetch_depth_fuse(self.h, st, 1, None) == 0
        host = (time.perf_counter() - t0) * 1e3
        assert self.L.ssd_get_depth_fuse_time(self.h, C.byref(ms)) == 0
        return host, float(ms.value)

    def close(self):
        self.L.ssd_destroy(self.h)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "depth_edges_time.txt")
    parent_path = sys.argv[3] if len(sys.argv) > 3 else None
    scs = [ssd.make_scene(W, H, n_steps=3, seed=1000 + i, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02) for i in range(F)]
    trans, intr = ssd.transformation_for_scene(scs[0]), ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    frame = W * H * 2
    nbytes = F * frame
    det = ssd.Detector(cfg, trans, 0)
    parent = ParentFuse(parent_path, cfg, trans) if parent_path else None
    # the narrow legs: the same frames 2 bytes further on, at strides 6 bytes wider
    nstride = frame + 6
    buf, out, cls = ssd.DeviceBuffer(nbytes, 0), ssd.DeviceBuffer(2 + F * nstride, 0), ssd.DeviceBuffer(8 + F * (frame // 2 + 3), 0)
    nbuf, mid = ssd.DeviceBuffer(2 + F * nstride, 0), ssd.DeviceBuffer(F // 8 * frame, 0)
    lines = ["# tools/depth_edges_time.py %d: XGA x %d resident depth frames (%d bytes), %d timed rounds, every leg once per round" % (rounds, F, nbytes, rounds),
             "# ms per leg, median (min .. max): host clock around enqueue and fetch; [..]: the leg's own device events; x read / x fuse1: the multiple",
             "# of the plain read's and of this build's k_depth_fuse n = 1 median; GB/s: bytes of input the leg reads per second"]
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

        def edges(wide, classes):
            src, dst, stride = (buf.ptr, out.ptr, frame) if wide else (nbuf.ptr + 2, out.ptr + 2, nstride)
            c = None if not classes else cls.ptr if wide else cls.ptr + 1
            host = clock(lambda: det.enqueue_depth_edges(src, F, dst, None, c, stride, stride, frame // 2 if wide else frame // 2 + 3),
                         lambda: det.fetch_depth_edges(1))
            return host, det.depth_edges_time(), nbytes

        def edges_detect():
            def go():
                det.enqueue_depth_edges(buf.ptr, F, out.ptr)
                det.enqueue_depth(out.ptr, F)
            return clock(go, lambda: det.fetch(F)), None, nbytes

        def chain():
            def go():
                groups = det.enqueue_depth_fuse(buf.ptr, F, 8, out.ptr)
                det.enqueue_depth_edges(out.ptr, groups, mid.ptr)
                det.enqueue_depth(mid.ptr, groups)
            return clock(go, lambda: det.fetch(F // 8)), None, nbytes

        legs = [("plain read", lambda: (None, ssd.stream_read_ms(buf.ptr, nbytes, reps=1), nbytes)),
                ("k_depth_fuse n 1 hop 1, this build", fuse1)]
        if parent:
            legs.append(("k_depth_fuse n 1 hop 1, parent build", lambda: parent.fuse1(buf.ptr, out.ptr, frame) + (nbytes,)))
        legs += [("k_depth_edges wide", lambda: edges(True, False)),
                 ("k_depth_edges wide + class map", lambda: edges(True, True)),
                 ("k_depth_edges narrow", lambda: edges(False, False)),
                 ("k_depth_edges narrow + class map", lambda: edges(False, True)),
                 ("detect 256 frames", lambda: (clock(lambda: det.enqueue_depth(buf.ptr, F), lambda: det.fetch(F)), None, nbytes)),
                 ("edges + detect 256 frames", edges_detect),
                 ("fuse n 8 + edges + detect 32 frames", chain)]

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
        # the bytes: frame 0 against the host statement
        det.enqueue_depth_edges(buf.ptr, F, out.ptr, None, cls.ptr)
        stats = det.fetch_depth_edges(1)[0]
        got = out.download(frame, dtype=np.uint16).reshape(H, W)
        gotc = cls.download(frame // 2).reshape(H, W)
        want, want_stats, wantc = ssd.depth_edges_host(ssd.synth_depth_host(scs[:1])[0], classes=True)
        same = bool((got == want).all()) and bool((gotc == wantc).all()) and bytes(stats) == bytes(want_stats)
        bad += 0 if same else 1
        lines.append("frame 0 equal to ssd_depth_edges_host, frame, class map and record: %s (%d of %d pixels kept, %d lone, %d bridge)"
                     % (same, stats.n_kept, W * H, stats.n_lone, stats.n_bridge))
        if not parent:
            lines.append("# the parent build's k_depth_fuse was not measured: no PARENT_LIB given")
    finally:
        for b in (buf, out, cls, nbuf, mid):
            b.free()
        det.close()
        if parent:
            parent.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
