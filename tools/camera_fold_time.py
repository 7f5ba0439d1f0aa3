#!/usr/bin/env python3
"""tools/camera_fold_time.py [ROUNDS] [OUT] [BENCH_LINES] - what the camera fold on the device (k_camera_fold, k_camera_ground_gates,
DESIGN.md section 7j) costs, timing on, after bench.py's half-second warm-up, legs alternating within a round, median of ROUNDS (25).

 (i)  The kernels: k_camera_fold and the overlay (k_camera_ground_gates) alone over the first-pass records of a resident XGA batch of
      256 and of 1024 frames (vertices, scenes.batch_scenes, one workspace, one camera's table entry repeated), under 1, 16 and 256
      cameras (frame i names camera i mod cameras), each by a pair of events around its launch on the null stream.  The yardsticks of
      the same run: k_surface_gates alone on the same records, and ssd_get_surface_refit_time of a host-gated pass.  The expectation
      they are held to: a launch's latency, small against a refit pass.
 (ii) The host path: wall time of Detector.camera_drift, XGA, 64 frames from pinned memory (two slices), passes 2, with device_fold
      False (the parent commit's code path: the yardstick; device_gates on) and True.  Both legs must give the same bytes.
 (iii) BENCH_LINES, when given: a file of "<label><TAB><bench.py's JSON line>" rows from alternating runs of the parent commit's tree
      and this build on one box (bench.py launches none of the new code); copied into the report with value and ms_per_step.

Writes profiles/camera_fold_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py and torch's events)."""
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import scenes  # noqa: E402

W, H = 1024, 768
RULE = dict(min_points=200, k_sigma=2.5, gate_min=0.0)
FOLD_MIN = 2000
CAMERAS = (1, 16, 256)


def spread(v):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def warm(one_round):
    c0 = time.perf_counter()
    while time.perf_counter() - c0 < 0.5:                                  # bench.py's warm-up: load until the device has been busy a while
        one_round()


def kernel_part(rounds, F, lines):
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    rec, gsz, fsz = C.sizeof(ssd.FrameMoments), C.sizeof(ssd.FrameGates), C.sizeof(ssd.CameraFold)
    det = ssd.Detector(cfg, trans, 0)
    bufs = [ssd.DeviceBuffer(F * W * H * 12, 0), ssd.DeviceBuffer(F * rec, 0), ssd.DeviceBuffer(F * rec, 0), ssd.DeviceBuffer(F * gsz, 0),
            ssd.DeviceBuffer(F * 4, 0), ssd.DeviceBuffer(max(CAMERAS) * fsz, 0)]
    buf, mom, out_h, gates_d, ind, fold = bufs
    try:
        ssd.synth_device(scs, buf.ptr, device=0)
        ssd.lib().ssd_device_sync(0)
        det.set_timing(True)
        det.set_cameras([trans] * max(CAMERAS))
        which = np.zeros(F, dtype=np.uint16)
        det.enqueue_cameras_surface_moments(buf.ptr, F, which, mom.ptr)
        det.fetch(F)
        first = (ssd.FrameMoments * F).from_buffer_copy(np.ascontiguousarray(mom.download(F * rec)).tobytes())
        gates = (ssd.FrameGates * F)(*[ssd.surface_gates_from_moments(m, **RULE) for m in first])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]

        def timed(k, call):
            ev[k].record()
            call()
            ev[k + 1].record()

        for ncams in CAMERAS:
            idx = (np.arange(F) % ncams).astype(np.int32)
            ind.upload(idx)

            def one_round():
                det.enqueue_cameras_surface_refit(buf.ptr, F, gates, out_h.ptr)
                det.fetch_surface_refit()
                a = det.surface_refit_time_ms()
                timed(0, lambda: det.enqueue_surface_gates(mom.ptr, F, gates_d.ptr, **RULE))
                ev[1].synchronize()
                b = ev[0].elapsed_time(ev[1])
                timed(0, lambda: det.enqueue_camera_fold(mom.ptr, ind.ptr, F, ncams, fold.ptr))
                timed(2, lambda: det.enqueue_camera_ground_gates(mom.ptr, ind.ptr, F, fold.ptr, ncams, gates_d.ptr, fold_min_points=FOLD_MIN,
                                                                 k_sigma=RULE["k_sigma"], gate_min=RULE["gate_min"]))
                ev[3].synchronize()
                return a, b, ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])

            warm(one_round)
            took = [one_round() for _ in range(rounds)]
            drift = ssd.camera_drift_fold(first, idx.astype(np.uint16), [trans] * ncams, min_points=FOLD_MIN)
            assert fold.download(ncams * fsz).tobytes() == b"".join(bytes(d)[:fsz] for d in drift), "the kernel's fold is the host function's"
            want = ssd.camera_ground_gates(first, idx.astype(np.uint16), drift, list(gates), RULE["k_sigma"], RULE["gate_min"])
            assert gates_d.download(F * gsz).tobytes() == b"".join(bytes(g) for g in want), "the kernel's gates are the host functions'"
            a, b, c, d = ([t[k] for t in took] for k in range(4))
            lines.append("%4d frames %3d cameras  host-gated pass (ssd_get_surface_refit_time)  %s ms" % (F, ncams, spread(a)))
            lines.append("%4d frames %3d cameras  k_surface_gates alone (events)               %s ms" % (F, ncams, spread(b)))
            lines.append("%4d frames %3d cameras  k_camera_fold alone (events)                 %s ms" % (F, ncams, spread(c)))
            lines.append("%4d frames %3d cameras  k_camera_ground_gates alone (events)         %s ms" % (F, ncams, spread(d)))
            lines.append("%4d frames %3d cameras  (fold + overlay) / host-gated pass = %.4f" % (F, ncams, (statistics.median(c) + statistics.median(d)) / statistics.median(a)))
    finally:
        for x in bufs:
            x.free()
        det.close()


def host_part(rounds, lines):
    F = 64
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    det = ssd.Detector(cfg, trans, 0)
    pinned = ssd.PinnedArray((F, H, W, 3), np.float32)
    try:
        pinned.array[...] = ssd.synth_host(scs)
        det.set_timing(True)
        det.set_cameras([trans] * 4)
        which = [i % 4 for i in range(F)]

        def leg(device_fold):
            c0 = time.perf_counter()
            got = det.camera_drift(pinned, which, min_points=FOLD_MIN, passes=2, device_gates=True, device_fold=device_fold)
            return (time.perf_counter() - c0) * 1e3, got

        def one_round():
            a, x = leg(False)
            b, y = leg(True)
            assert [[bytes(v) for v in p] for p in x] == [[bytes(v) for v in p] for p in y], "both legs give the same bytes"
            return a, b

        warm(one_round)
        took = [one_round() for _ in range(rounds)]
        a, b = [t[0] for t in took], [t[1] for t in took]
        lines.append("passes 2  device_fold=False %s ms   device_fold=True %s ms   True / False = %.3f"
                     % (spread(a), spread(b), statistics.median(b) / statistics.median(a)))
    finally:
        pinned.free()
        det.close()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "camera_fold_time.txt")
    bench_lines = sys.argv[3] if len(sys.argv) > 3 else None
    lines = ["# tools/camera_fold_time.py %d: timing on, half a second of warm-up per part, legs alternating within a round, %d rounds;" % (rounds, rounds),
             "# median (min .. max)", "", "## (i) k_camera_fold and k_camera_ground_gates on a resident XGA batch (vertices), beside k_surface_gates and a refit pass of the same handle"]
    for F in (256, 1024):
        kernel_part(rounds, F, lines)
    lines += ["", "## (ii) Detector.camera_drift, XGA, 64 frames from pinned memory (two slices of 32), passes 2, device gates: wall time per call"]
    host_part(rounds, lines)
    if bench_lines:
        lines += ["", "## (iii) bench.py, the parent commit's tree and this build alternating on one box (bench.py launches none of the new code)"]
        for row in open(bench_lines):
            if "\t" not in row:
                continue
            label, text = row.rstrip("\n").split("\t", 1)
            try:
                j = json.loads(text)
                lines.append("%-12s value %.1f   ms_per_step %.4f" % (label, j["value"], j["ms_per_step"]))
            except (ValueError, KeyError):
                lines.append("%-12s %s" % (label, text))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
