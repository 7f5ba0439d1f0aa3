#!/usr/bin/env python3
"""tools/surface_refit_time.py [ROUNDS] [OUT] - what the trimmed refit pass (k_surface_refit) costs beside its
yardstick, the first pass (k_surface_moments), on the same batch in the same run: XGA x 1024 frames resident in device memory
(scenes.batch_scenes, the bench's), as vertices and as 16-bit depth, one workspace, timing on.  A round is one enqueue with surface
moments (the first pass's time: ssd_get_surface_moments_time_back) and one refit pass behind it (ssd_get_surface_refit_time), gated at
2.5 rms by the planes of that first pass - so the legs alternate, after bench.py's half-second warm-up.  Both times include the memset
of the records in front of the kernel.  The refit reads the same cells: the expectation is "about the first pass".
Writes profiles/surface_refit_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import scenes  # noqa: E402

W, H, F = 1024, 768, 1024


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "surface_refit_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    wh, rec = W * H, C.sizeof(ssd.FrameMoments)
    lines = ["# tools/surface_refit_time.py %d: XGA x %d resident frames, one workspace, %d timed rounds; a round = one enqueue with surface" % (rounds, F, rounds),
             "# moments, then one refit pass behind it (gates: 2.5 rms of that first pass).  ms per pass over %d frames, median (min .. max)" % F]
    for depth in (False, True):
        det = ssd.Detector(cfg, trans, 0)
        buf = ssd.DeviceBuffer(F * wh * (2 if depth else 12), 0)
        mom = ssd.DeviceBuffer(F * rec, 0)
        out = ssd.DeviceBuffer(F * rec, 0)
        try:
            if depth:
                det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
                ssd.synth_depth_device(scs, buf.ptr, device=0)
            else:
                ssd.synth_device(scs, buf.ptr, device=0)
            ssd.lib().ssd_device_sync(0)
            det.set_timing(True)
            det.enqueue_surface_moments(buf.ptr, F, mom.ptr, depth=depth)
            det.fetch(F)
            first = (ssd.FrameMoments * F).from_buffer_copy(np.ascontiguousarray(mom.download(F * rec)).tobytes())
            gates = (ssd.FrameGates * F)(*[ssd.surface_gates_from_moments(m, 200, 2.5, 0.0) for m in first])

            def one_round():
                det.enqueue_surface_moments(buf.ptr, F, mom.ptr, depth=depth)
                det.fetch(F)
                a = det.surface_moments_time_ms(0)
                det.enqueue_surface_refit(buf.ptr, F, gates, out.ptr, depth=depth)
                det.fetch_surface_refit()
                return a, det.surface_refit_time_ms()

            c0 = time.perf_counter()
            while time.perf_counter() - c0 < 0.5:                          # bench.py's warm-up: load until the device has been busy a while
                one_round()
            took = [one_round() for _ in range(rounds)]
            a, b = [t[0] for t in took], [t[1] for t in took]
            refit = (ssd.FrameMoments * F).from_buffer_copy(np.ascontiguousarray(out.download(F * rec)).tobytes())
            kept = sum(int(m.s[k].m.n + m.s[k].n_far) for m in refit for k in range(m.n_surfaces))
            full = sum(int(m.s[k].m.n + m.s[k].n_far) for m in first for k in range(m.n_surfaces))
            tag = "depth16" if depth else "vertices"
            lines.append("%-8s k_surface_moments %.3f (%.3f .. %.3f)" % (tag, statistics.median(a), min(a), max(a)))
            lines.append("%-8s k_surface_refit   %.3f (%.3f .. %.3f)   kept %d of %d labelled points" % (tag, statistics.median(b), min(b), max(b), kept, full))
            lines.append("%-8s k_surface_refit / k_surface_moments = %.2f" % (tag, statistics.median(b) / statistics.median(a)))
        finally:
            buf.free()
            mom.free()
            out.free()
            det.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
