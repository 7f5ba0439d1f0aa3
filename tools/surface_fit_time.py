#!/usr/bin/env python3
"""tools/surface_fit_time.py [ROUNDS] [OUT] - what the surface-moments pass costs beside its yardstick, k_labels, on the same batch in
the same run: XGA x 1024 frames resident in device memory (scenes.batch_scenes, the bench's), as vertices and as 16-bit depth, one
workspace, timing on; legs alternated (labels, moments, labels, ...) after bench.py's half-second warm-up.  Per leg the device time
of the pass alone (ssd_get_labels_time_back / ssd_get_surface_moments_time_back: the latter includes the memset of the records) and
of the whole enqueue.  The new pass walks the same cells and writes 1.5 KB per frame where k_labels writes a byte per point.
Writes profiles/surface_fit_time.txt (or OUT); bench.py's own line of the parent and of this build on one box are appended to that
file by whoever runs both (the tool cannot build the parent).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
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
import scenes  # noqa: E402

W, H, F, STEPS = 1024, 768, 1024, 5


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "surface_fit_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    wh = W * H
    lines = ["# tools/surface_fit_time.py %d: XGA x %d resident frames, one workspace, %d timed enqueues per leg and round, legs alternated" % (rounds, F, STEPS),
             "# ms per enqueue of %d frames, median over all timed enqueues (min .. max): the pass alone | the seven stages" % F]
    for depth in (False, True):
        det = ssd.Detector(cfg, trans, 0)
        buf = ssd.DeviceBuffer(F * wh * (2 if depth else 12), 0)
        lab = ssd.DeviceBuffer(F * wh, 0)
        mom = ssd.DeviceBuffer(F * C.sizeof(ssd.FrameMoments), 0)
        try:
            if depth:
                det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
                ssd.synth_depth_device(scs, buf.ptr, device=0)
            else:
                ssd.synth_device(scs, buf.ptr, device=0)
            ssd.lib().ssd_device_sync(0)
            det.set_timing(True)
            legs = {
                "k_labels": (lambda: (det.enqueue_depth_labels if depth else det.enqueue_labels)(buf.ptr, F, lab.ptr), det.labels_time_ms),
                "k_surface_moments": (lambda: det.enqueue_surface_moments(buf.ptr, F, mom.ptr, depth=depth), det.surface_moments_time_ms),
            }
            c0 = time.perf_counter()
            while time.perf_counter() - c0 < 0.5:                          # bench.py's warm-up: load until the device has been busy a while
                for enq, _ in legs.values():
                    enq()
                    det.fetch(F)
            took = {k: ([], []) for k in legs}
            for _ in range(rounds):
                for name, (enq, pass_ms) in legs.items():
                    for _ in range(STEPS):
                        enq()
                        det.fetch(F)
                        took[name][0].append(pass_ms(0))
                        took[name][1].append(sum(det.stage_times_ms(0).values()))
            for name, (p, s) in took.items():
                lines.append("%-8s %-18s %.3f (%.3f .. %.3f) | %.3f (%.3f .. %.3f)" % ("depth16" if depth else "vertices", name, statistics.median(p), min(p), max(p),
                                                                                       statistics.median(s), min(s), max(s)))
            a, b = statistics.median(took["k_surface_moments"][0]), statistics.median(took["k_labels"][0])
            lines.append("%-8s k_surface_moments / k_labels = %.2f" % ("depth16" if depth else "vertices", a / b))
        finally:
            buf.free()
            lab.free()
            mom.free()
            det.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
