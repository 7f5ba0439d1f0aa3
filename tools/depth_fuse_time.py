#!/usr/bin/env python3
"""tools/depth_fuse_time.py [ROUNDS] [OUT] - what the depth fusion (k_depth_fuse) costs beside its yardstick, a plain
read of the same bytes (ssd.stream_read_ms), on one resident batch in one run: XGA x 256 16-bit depth frames of ONE still scene (3 steps,
sigma 2 mm, 5 % outliers, 2 % invalid, seeds 1000 ..), 403 MB.
A round is every leg once, so the legs alternate, after bench.py's half-second warm-up: the plain read; the depth leg of
k_ground_moments; k_depth_fuse at n = 4, 8 and 16 with hop == n (64, 32 and 16 groups); k_depth_fuse at n = 8 with hop == 1 (249 groups:
every frame is read eight times) in the product's grid order and - where the loaded library is a tools build (make EXTRA=-DSSD_TUNING,
named by SSD_HIP_LIB), which reads SSD_FUSE_GROUP_FASTEST in ssd_create - in the other one; the chain of n = 8 fusion plus detection of
the 32 fused frames on one stream with no host wait; the detection of all 256 frames.
The read is timed by the hook's own device events; every other leg by a host clock around the enqueue and the fetch that waits for it,
and the fusion's own device events (ssd_get_depth_fuse_time: the zeroing of its records and their copy included) stand beside it in [..].
Multiples of the plain read and bytes of input per second come from the device events where a leg has them.  Group 0 of n = 8 is checked
against ssd_depth_fuse_host.  Nothing is fixed in advance: the figures are what they are.
Writes profiles/depth_fuse_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/fuse_model.py)."""
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

W, H, F, TOL = 1024, 768, 256, 0.03


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "depth_fuse_time.txt")
    orders = bool(os.environ.get("SSD_HIP_LIB"))
    scs = [ssd.make_scene(W, H, n_steps=3, seed=1000 + i, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02) for i in range(F)]
    trans, intr = ssd.transformation_for_scene(scs[0]), ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    frame = W * H * 2
    nbytes = F * frame
    dets = [ssd.Detector(cfg, trans, 0)]
    if orders:
        os.environ["SSD_FUSE_GROUP_FASTEST"] = "1"
        dets.append(ssd.Detector(cfg, trans, 0))
        del os.environ["SSD_FUSE_GROUP_FASTEST"]
    buf, out = ssd.DeviceBuffer(nbytes, 0), ssd.DeviceBuffer(nbytes, 0)
    lines = ["# tools/depth_fuse_time.py %d: XGA x %d resident depth frames of one still scene (%d bytes), %d timed rounds, every leg once per round"
             % (rounds, F, nbytes, rounds),
             "# ms per leg, median (min .. max): host clock around enqueue and fetch; [..]: the leg's own device events; x read: the multiple of the",
             "# plain read's median; GB/s: bytes of input the leg reads per second (hop == 1 reads every frame n times: the bytes its groups name)"]
    bad = 0
    try:
        for det in dets:
            det.set_intrinsics(intr)
            det.set_timing(True)
        det = dets[0]
        ssd.synth_depth_device(scs, buf.ptr, device=0)
        ssd.lib().ssd_device_sync(0)

        def clock(fn, fetch):
            t0 = time.perf_counter()
            fn()
            fetch()
            return (time.perf_counter() - t0) * 1e3

        def fuse(d, n, hop):
            groups = (F - n) // hop + 1
            host = clock(lambda: d.enqueue_depth_fuse(buf.ptr, F, n, out.ptr, hop), lambda: d.fetch_depth_fuse(1))
            return host, d.depth_fuse_time_ms(), groups * n * frame

        def chain():
            def go():
                groups = det.enqueue_depth_fuse(buf.ptr, F, 8, out.ptr)
                det.enqueue_depth(out.ptr, groups)
            return clock(go, lambda: det.fetch(F // 8))

        legs = [("plain read", lambda: (None, ssd.stream_read_ms(buf.ptr, nbytes, reps=1), nbytes)),
                ("k_ground_moments, depth", lambda: (clock(lambda: det.enqueue_ground_fit(buf.ptr, F, TOL, depth=True),
                                                           lambda: det.fetch_ground_fit(1, min_points=1)), None, nbytes)),
                ("k_depth_fuse n 4 hop 4", lambda: fuse(det, 4, 4)),
                ("k_depth_fuse n 8 hop 8", lambda: fuse(det, 8, 8)),
                ("k_depth_fuse n 16 hop 16", lambda: fuse(det, 16, 16)),
                ("k_depth_fuse n 8 hop 1, chunk-fastest", lambda: fuse(det, 8, 1))]
        if orders:
            legs.append(("k_depth_fuse n 8 hop 1, group-fastest", lambda: fuse(dets[1], 8, 1)))
        legs += [("fuse n 8 + detect 32 fused frames", lambda: (chain(), None, nbytes)),
                 ("detect all 256 frames", lambda: (clock(lambda: det.enqueue_depth(buf.ptr, F), lambda: det.fetch(F)), None, nbytes))]

        def one_round():
            return [leg() for _, leg in legs]
        c0 = time.perf_counter()
        while time.perf_counter() - c0 < 0.5:                              # bench.py's warm-up: load until the device has been busy a while
            one_round()
        took = [one_round() for _ in range(rounds)]
        read = statistics.median(r[0][1] for r in took)
        for k, (name, _) in enumerate(legs):
            host = [r[k][0] for r in took if r[k][0] is not None]
            dev = [r[k][1] for r in took if r[k][1] is not None]
            moved = took[0][k][2]
            best = statistics.median(dev) if dev else statistics.median(host)
            cells = ["%-40s" % name]
            cells.append("%8.3f (%.3f .. %.3f)" % (statistics.median(host), min(host), max(host)) if host else "%8s" % "-")
            cells.append("[%.3f (%.3f .. %.3f)]" % (statistics.median(dev), min(dev), max(dev)) if dev else "[-]")
            cells.append("%.2f x read, %.0f GB/s" % (best / read, moved / best / 1e6))
            lines.append("  ".join(cells))
        # the bytes: group 0 of n = 8 against the host statement
        det.enqueue_depth_fuse(buf.ptr, F, 8, out.ptr)
        stats = det.fetch_depth_fuse(1)[0]
        got = out.download(frame, dtype=np.uint16).reshape(H, W)
        want, want_stats = ssd.depth_fuse_host(ssd.synth_depth_host(scs[:8]))
        same = bool((got == want).all()) and bytes(stats) == bytes(want_stats)
        bad += 0 if same else 1
        lines.append("group 0 of n = 8 equal to ssd_depth_fuse_host, frame and record: %s (%d of %d pixels fused)" % (same, stats.n_fused, W * H))
        if not orders:
            lines.append("# the group-fastest grid order was not measured: the loaded library is no tools build")
    finally:
        buf.free()
        out.free()
        for d in dets:
            d.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
