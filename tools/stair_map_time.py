#!/usr/bin/env python3
"""tools/stair_map_time.py [ROUNDS] [OUT] - what the stair map pass (k_stair_map) costs beside its yardstick, the
tread grid pass (k_tread_grid) it shares its walk with, on the same batch in the same run: XGA x 256 frames resident in device memory
(scenes.batch_scenes, the bench's), as vertices and as 16-bit depth, one workspace, timing on.
A round is one whole enqueue, then a tread grid pass (ssd_get_tread_grid_time), a stair map pass with ONE map that all 256 frames name
and a stair map pass with 16 maps dealt round-robin (ssd_get_stair_map_time; every pass's time includes the zeroing in front of the
kernel: 256 records for the tread grid, 1 or 16 for the stair map) - so the legs alternate, after bench.py's half-second warm-up.  The
maps are the fetched results of the batch's first frames.  With one map every block's flush goes to the same few hundred words; with
16 the same atomics spread over 16 records: the difference between the two legs is what the shared addresses cost.
Nothing is fixed in advance: the figures are what they are.
Writes profiles/stair_map_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
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

W, H, F, MAPS = 1024, 768, 256, 16


def totals(buf, n):
    """tread points and occupants in n records of a device buffer"""
    grid = C.sizeof(ssd.FrameTreadGrid)
    words = np.frombuffer(np.ascontiguousarray(buf.download(n * grid)).tobytes(), dtype=np.uint32).reshape(n, grid // 4)[:, 2:]
    words = words.reshape(n, ssd.MAX_STEPS, 3088 // 4)
    return (int(words[:, :, 0].sum(dtype=np.int64) + words[:, :, 4:260].sum(dtype=np.int64)),
            int(words[:, :, 1].sum(dtype=np.int64) + words[:, :, 260:516].sum(dtype=np.int64)))


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stair_map_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    wh, grid = W * H, C.sizeof(ssd.FrameTreadGrid)
    rule = ssd.TreadGridRule()
    lines = ["# tools/stair_map_time.py %d: XGA x %d resident frames, one workspace, %d timed rounds; a round = one whole enqueue, then a tread"
             % (rounds, F, rounds),
             "# grid pass, a stair map pass with 1 map for all frames and one with %d maps dealt round-robin (rule %g / %g / %g, cell %g)."
             % (MAPS, rule.clearance.margin, rule.clearance.lo, rule.clearance.hi, rule.cell),
             "# ms per pass over %d frames, the zeroing included, median (min .. max)" % F]
    for depth in (False, True):
        det = ssd.Detector(cfg, trans, 0)
        buf = ssd.DeviceBuffer(F * wh * (2 if depth else 12), 0)
        gout = ssd.DeviceBuffer(F * grid, 0)
        mout = ssd.DeviceBuffer(MAPS * grid, 0)
        try:
            if depth:
                det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
                ssd.synth_depth_device(scs, buf.ptr, device=0)
            else:
                ssd.synth_device(scs, buf.ptr, device=0)
            ssd.lib().ssd_device_sync(0)
            det.set_timing(True)
            (det.enqueue_depth if depth else det.enqueue)(buf.ptr, F)
            res = det.fetch_list(F)
            maps = [ssd.StairMap() for _ in range(MAPS)]
            for m, r in zip(maps, res):
                C.memmove(C.byref(m.stairs), C.byref(r), C.sizeof(ssd.FrameResult))
                m.ground = 1
            dealt = [i % MAPS for i in range(F)]

            def one_round():
                (det.enqueue_depth if depth else det.enqueue)(buf.ptr, F)
                det.fetch(F)
                det.enqueue_tread_grid(buf.ptr, F, gout.ptr, rule, depth=depth)
                det.fetch_tread_grid()
                a = det.tread_grid_time_ms()
                det.enqueue_stair_map(buf.ptr, F, maps, mout.ptr, dealt, rule, depth=depth)
                det.fetch_stair_map()
                c = det.stair_map_time_ms()
                det.enqueue_stair_map(buf.ptr, F, maps[:1], mout.ptr, None, rule, depth=depth)
                det.fetch_stair_map()
                return a, det.stair_map_time_ms(), c

            c0 = time.perf_counter()
            while time.perf_counter() - c0 < 0.5:                          # bench.py's warm-up: load until the device has been busy a while
                one_round()
            took = [one_round() for _ in range(rounds)]
            own, one = totals(gout, F), totals(mout, 1)
            det.enqueue_stair_map(buf.ptr, F, maps, mout.ptr, dealt, rule, depth=depth)
            det.fetch_stair_map()
            many = totals(mout, MAPS)
            tag = "depth16" if depth else "vertices"
            for name, col in (("k_tread_grid", 0), ("k_stair_map, 1 map", 1), ("k_stair_map, %d maps" % MAPS, 2)):
                t = [x[col] for x in took]
                lines.append("%-8s %-22s %.3f (%.3f .. %.3f)" % (tag, name, statistics.median(t), min(t), max(t)))
            med = [statistics.median([x[col] for x in took]) for col in range(3)]
            lines.append("%-8s ratios of the medians: 1 map / k_tread_grid %.3f, %d maps / k_tread_grid %.3f, 1 map / %d maps %.3f"
                         % (tag, med[1] / med[0], MAPS, med[2] / med[0], MAPS, med[1] / med[2]))
            lines.append("%-8s tread points | occupants: %d | %d in the frames' own grids, %d | %d in the one map, %d | %d in the %d maps"
                         % (tag, own[0], own[1], one[0], one[1], many[0], many[1], MAPS))
        finally:
            for b in (buf, gout, mout):
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
