#!/usr/bin/env python3
"""tools/ground_fit_time.py [ROUNDS] [OUT] - the ground fit's pass over XGA x 1024 frames resident in device memory, as vertices and
as 16-bit depth, beside the plain read stream over the same buffer (stream_read_ms, the yardstick K1 is held to): after bench.py's
half-second warm-up the legs alternate, each timed with a host clock around work that ends in a device synchronise.  Checks the first
and the last frame's moments against ssd_ground_moments_host.  Writes both times and their ratio to profiles/ground_fit_time.txt (or
OUT); bench.py's own figures of the parent and of this build are appended to that file by whoever runs both (the tool cannot build
the parent).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import scenes  # noqa: E402

W, H, F, STEPS, TOL = 1024, 768, 1024, 10, 0.03


def timed(fn, n):
    ssd.lib().ssd_device_sync(0)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    ssd.lib().ssd_device_sync(0)
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ground_fit_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    intr = ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F)
    det = ssd.Detector(cfg, trans, 0)
    det.set_intrinsics(intr)
    lines = ["# tools/ground_fit_time.py %d: XGA x %d resident frames, tol %g, %d calls per leg and round, legs alternated; ms per call" % (rounds, F, TOL, STEPS)]
    bad = 0
    for name, depth, per in (("vertices", False, 12), ("depth16", True, 2)):
        nbytes = F * W * H * per
        buf = ssd.DeviceBuffer(nbytes, 0)
        (ssd.synth_depth_device if depth else ssd.synth_device)(scs, buf.ptr, device=0)
        ssd.lib().ssd_device_sync(0)
        fit = lambda: det.enqueue_ground_fit(buf.ptr, F, TOL, depth=depth)      # noqa: E731
        read = lambda: ssd.stream_read_ms(buf.ptr, nbytes, reps=1)              # noqa: E731
        c0 = time.perf_counter()
        while time.perf_counter() - c0 < 0.5:                                   # bench.py's warm-up: load until the device has been busy a while
            fit()
            det.fetch_ground_fit(1)
        read()
        got = det.fetch_ground_fit(F, min_points=1)
        for i in (0, F - 1):
            host = (ssd.synth_depth_host if depth else ssd.synth_host)([scs[i]])[0]
            want = ssd.ground_moments_host(cfg, (trans, intr), host, TOL, depth=depth)
            same = bytes(got[i].m) == bytes(want)
            bad += 0 if same else 1
            lines.append("%s frame %d: %d floor points, equal to the host's moments: %s" % (name, i, got[i].m.n, same))
        t_fit, t_read, t_hook = [], [], []
        for r in range(rounds):
            t_fit.append(timed(fit, STEPS))
            t_read.append(timed(read, STEPS))
            t_hook.append(float(np.mean([read() for _ in range(STEPS)])))
            lines.append("%s round %d: ground fit %.3f ms, read stream %.3f ms (its own device events: %.3f ms)" % (name, r, t_fit[-1], t_read[-1], t_hook[-1]))
        mf, mr, mh = float(np.median(t_fit)), float(np.median(t_read)), float(np.median(t_hook))
        lines.append("%s median: ground fit %.3f ms = %.0f GB/s, read stream %.3f ms = %.0f GB/s (device events %.3f ms); read / ground fit = %.3f (events: %.3f)"
                     % (name, mf, nbytes / mf / 1e6, mr, nbytes / mr / 1e6, mh, mr / mf, mh / mf))
        buf.free()
    det.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
