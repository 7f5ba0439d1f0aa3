#!/usr/bin/env python3
"""tools/depth_host_pre_time.py [ROUNDS] [OUT] - what the host-fed depth pre-passes cost end to end (process_depth_host_pre, DESIGN.md section
7u): ssd_process_depth_host_fused at n = 8 and ssd_process_depth_host_edges over 64 XGA 16-bit depth frames of one still scene in pinned
host memory, results only.  Two warm-up calls of each, then ROUNDS (15) rounds of both, so the legs alternate; a host clock around each
call, which returns with its last slice collected.  The library is the one the package loads (SSD_HIP_LIB names another build's).
Prints the lines and, with OUT, writes them there.  Nothing is fixed in advance: the figures are what they are.  TEST INFRASTRUCTURE."""
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ssd = importlib.import_module("stair-step-detector_amd")

W, H, F, N = 1024, 768, 64, 8


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    scs = [ssd.make_scene(W, H, n_steps=3, seed=1000 + i, sigma=0.002, outlier_frac=0.05, invalid_frac=0.02) for i in range(F)]
    det = ssd.Detector(ssd.default_config(W, H, max_frames_per_batch=F), ssd.transformation_for_scene(scs[0]), 0)
    pinned = ssd.PinnedArray((F, H, W), "uint16")
    try:
        det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
        pinned.array[:] = ssd.synth_depth_host(scs)
        legs = [("process_depth_host_fused n = 8", lambda: det.process_depth_host_fused(pinned.array, N)),
                ("process_depth_host_edges", lambda: det.process_depth_host_edges(pinned.array))]
        took = {name: [] for name, _ in legs}
        for r in range(rounds + 2):
            for name, call in legs:
                t0 = time.perf_counter()
                res = call()
                ms = (time.perf_counter() - t0) * 1e3
                if r >= 2:
                    took[name].append(ms)
                assert len(res) == (F // N if "fused" in name else F) and max(x.n_steps for x in res) >= 3, name
        lines = ["# tools/depth_host_pre_time.py %d: %d XGA depth frames in pinned host memory, %d timed rounds, the legs alternating; ms per call" % (rounds, F, rounds)]
        lines += ["%-32s median %8.3f   (min %8.3f .. max %8.3f)" % (name, statistics.median(t), min(t), max(t)) for name, t in took.items()]
    finally:
        pinned.free()
        det.close()
    print("\n".join(lines))
    if len(sys.argv) > 2:
        open(sys.argv[2], "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
