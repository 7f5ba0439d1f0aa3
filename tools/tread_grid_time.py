#!/usr/bin/env python3
"""tools/tread_grid_time.py [ROUNDS] [OUT] - what the tread grid pass (k_tread_grid) costs beside its yardsticks,
k_labels and the clearance pass (k_clearance, without a mask), on the same batch in the same run: XGA x 256 frames resident in device
memory (scenes.batch_scenes, the bench's), as vertices and as 16-bit depth, one workspace, timing on.
A round is one enqueue with labels (ssd_get_labels_time_back), one clearance pass (ssd_get_clearance_time) and one tread grid pass
(ssd_get_tread_grid_time; both passes' times include the zeroing in front of the kernel) - so the legs alternate, after bench.py's
half-second warm-up.  Nothing is fixed in advance: the figures are what they are.
Writes profiles/tread_grid_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
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
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "tread_grid_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    wh, rec, grid = W * H, C.sizeof(ssd.FrameMoments), C.sizeof(ssd.FrameTreadGrid)
    rule = ssd.TreadGridRule()
    lines = ["# tools/tread_grid_time.py %d: XGA x %d resident frames, one workspace, %d timed rounds; a round = one enqueue with labels, then a" % (rounds, F, rounds),
             "# clearance pass without a mask and a tread grid pass (rule %g / %g / %g, cell %g).  ms per pass over %d frames, median (min .. max)"
             % (rule.clearance.margin, rule.clearance.lo, rule.clearance.hi, rule.cell, F)]
    for depth in (False, True):
        det = ssd.Detector(cfg, trans, 0)
        buf = ssd.DeviceBuffer(F * wh * (2 if depth else 12), 0)
        lab = ssd.DeviceBuffer(F * wh, 0)
        out = ssd.DeviceBuffer(F * rec, 0)
        gout = ssd.DeviceBuffer(F * grid, 0)
        try:
            if depth:
                det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
                ssd.synth_depth_device(scs, buf.ptr, device=0)
            else:
                ssd.synth_device(scs, buf.ptr, device=0)
            ssd.lib().ssd_device_sync(0)
            det.set_timing(True)

            def one_round():
                (det.enqueue_depth_labels if depth else det.enqueue_labels)(buf.ptr, F, lab.ptr)
                det.fetch(F)
                a = det.labels_time_ms(0)
                det.enqueue_clearance(buf.ptr, F, out.ptr, rule.clearance, depth=depth)
                det.fetch_clearance()
                b = det.clearance_time_ms()
                det.enqueue_tread_grid(buf.ptr, F, gout.ptr, rule, depth=depth)
                det.fetch_tread_grid()
                return a, b, det.tread_grid_time_ms()

            c0 = time.perf_counter()
            while time.perf_counter() - c0 < 0.5:                          # bench.py's warm-up: load until the device has been busy a while
                one_round()
            took = [one_round() for _ in range(rounds)]
            raw = np.ascontiguousarray(out.download(F * rec)).tobytes()
            occupants = sum(int(m.s[k].m.n + m.s[k].n_far) for m in (ssd.FrameMoments * F).from_buffer_copy(raw) for k in range(m.n_surfaces))
            words = np.frombuffer(np.ascontiguousarray(gout.download(F * grid)).tobytes(), dtype=np.uint32).reshape(F, grid // 4)[:, 2:]
            words = words.reshape(F, ssd.MAX_STEPS, 3088 // 4)
            seen = int(words[:, :, 0].sum(dtype=np.int64) + words[:, :, 4:260].sum(dtype=np.int64))
            occ = int(words[:, :, 1].sum(dtype=np.int64) + words[:, :, 260:516].sum(dtype=np.int64))
            tag = "depth16" if depth else "vertices"
            for name, col in (("k_labels", 0), ("k_clearance, no mask", 1), ("k_tread_grid", 2)):
                t = [x[col] for x in took]
                lines.append("%-8s %-22s %.3f (%.3f .. %.3f)" % (tag, name, statistics.median(t), min(t), max(t)))
            lines.append("%-8s in the batch: %d tread points and %d occupants in the grids' records, %d occupants in the clearance records"
                         % (tag, seen, occ, occupants))
        finally:
            for b in (buf, lab, out, gout):
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
