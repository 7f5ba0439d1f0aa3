#!/usr/bin/env python3
"""tools/clearance_time.py [ROUNDS] [OUT] - what the tread clearance pass (k_clearance) costs beside its yardsticks,
k_labels and the riser labels' pass (k_riser_labels: the riser pass's walk), on the same batch in the same run: XGA x 256 frames resident in
device memory (scenes.batch_scenes, the bench's), as vertices and as 16-bit depth, one workspace, timing on, risers and riser labels on.
A round is one enqueue with labels (ssd_get_labels_time_back, ssd_get_riser_labels_time_back), one clearance pass with the mask behind it
and one without (ssd_get_clearance_time; both include the zeroing in front of the kernel) - so the legs alternate, after bench.py's
half-second warm-up.  Nothing is fixed in advance: the figures are what they are.
Writes profiles/clearance_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
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

W, H, F = 1024, 768, 256


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "clearance_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    wh, rec = W * H, C.sizeof(ssd.FrameMoments)
    rule = ssd.ClearanceRule()
    lines = ["# tools/clearance_time.py %d: XGA x %d resident frames, one workspace, %d timed rounds; a round = one enqueue with labels and riser" % (rounds, F, rounds),
             "# labels, then a clearance pass with the mask and one without (rule %g / %g / %g).  ms per pass over %d frames, median (min .. max)"
             % (rule.margin, rule.lo, rule.hi, F)]
    for depth in (False, True):
        det = ssd.Detector(cfg, trans, 0)
        buf = ssd.DeviceBuffer(F * wh * (2 if depth else 12), 0)
        lab = ssd.DeviceBuffer(F * wh, 0)
        mask = ssd.DeviceBuffer(F * wh, 0)
        out = ssd.DeviceBuffer(F * rec, 0)
        try:
            if depth:
                det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
                ssd.synth_depth_device(scs, buf.ptr, device=0)
            else:
                ssd.synth_device(scs, buf.ptr, device=0)
            ssd.lib().ssd_device_sync(0)
            det.set_risers(True)
            det.set_riser_labels(True)
            det.set_timing(True)

            def one_round():
                (det.enqueue_depth_labels if depth else det.enqueue_labels)(buf.ptr, F, lab.ptr)
                det.fetch(F)
                a, b = det.labels_time_ms(0), det.riser_labels_time_ms(0)
                det.enqueue_clearance(buf.ptr, F, out.ptr, rule, mask.ptr, depth=depth)
                det.fetch_clearance()
                c = det.clearance_time_ms()
                det.enqueue_clearance(buf.ptr, F, out.ptr, rule, depth=depth)
                det.fetch_clearance()
                return a, b, c, det.clearance_time_ms()

            c0 = time.perf_counter()
            while time.perf_counter() - c0 < 0.5:                          # bench.py's warm-up: load until the device has been busy a while
                one_round()
            took = [one_round() for _ in range(rounds)]
            recs = (ssd.FrameMoments * F).from_buffer_copy(np.ascontiguousarray(out.download(F * rec)).tobytes())
            occupants = sum(int(m.s[k].m.n + m.s[k].n_far) for m in recs for k in range(m.n_surfaces))
            tag = "depth16" if depth else "vertices"
            for name, col in (("k_labels", 0), ("k_riser_labels", 1), ("k_clearance, mask", 2), ("k_clearance, no mask", 3)):
                t = [x[col] for x in took]
                lines.append("%-8s %-22s %.3f (%.3f .. %.3f)" % (tag, name, statistics.median(t), min(t), max(t)))
            lines.append("%-8s occupants in the batch: %d" % (tag, occupants))
        finally:
            for b in (buf, lab, mask, out):
                b.free()
            det.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
