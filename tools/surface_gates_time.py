#!/usr/bin/env python3
"""tools/surface_gates_time.py [ROUNDS] [OUT] [BENCH_LINES] - what the gates on the device (k_surface_gates) cost
and what they buy, timing on, after bench.py's half-second warm-up, legs alternating within a round, median of ROUNDS (25) rounds.

 (i)  The kernel: k_surface_gates alone over the first-pass records of a resident XGA batch of 256 and of 1024 frames (vertices,
      scenes.batch_scenes, one workspace), by a pair of events around its launch on the null stream, beside
      ssd_get_surface_refit_time of a host-gated pass and of a device-gated pass (which includes the kernel) of the same handle.
      The expectation it is held to: small against a refit pass.
 (ii) The host path: wall time of process_host_surfaces_refit with device_gates False (the parent commit's code path: the yardstick)
      and True, XGA, 64 frames from pinned memory (two slices), passes 1, 2 and 4.  Both legs must give the same bytes.
 (iii) BENCH_LINES, when given: a file of "<label><TAB><bench.py's JSON line>" rows from alternating runs of the parent commit's tree
      and this build on one box (bench.py launches none of the new code); copied into the report with value and ms_per_step.

Writes profiles/surface_gates_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py and torch's events)."""
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


def spread(v):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def warm(one_round):
    c0 = time.perf_counter()
    while time.perf_counter() - c0 < 0.5:                                  # bench.py's warm-up: load until the device has been busy a while
        one_round()


def kernel_part(rounds, F, lines):
    scs = scenes.batch_scenes(ssd, W, H, F)
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    rec, gsz = C.sizeof(ssd.FrameMoments), C.sizeof(ssd.FrameGates)
    det = ssd.Detector(cfg, ssd.transformation_for_scene(scs[0]), 0)
    bufs = [ssd.DeviceBuffer(F * W * H * 12, 0), ssd.DeviceBuffer(F * rec, 0), ssd.DeviceBuffer(F * rec, 0), ssd.DeviceBuffer(F * rec, 0),
            ssd.DeviceBuffer(F * gsz, 0)]
    buf, mom, out_h, out_d, gates_d = bufs
    try:
        ssd.synth_device(scs, buf.ptr, device=0)
        ssd.lib().ssd_device_sync(0)
        det.set_timing(True)
        det.enqueue_surface_moments(buf.ptr, F, mom.ptr)
        det.fetch(F)
        first = (ssd.FrameMoments * F).from_buffer_copy(np.ascontiguousarray(mom.download(F * rec)).tobytes())
        gates = (ssd.FrameGates * F)(*[ssd.surface_gates_from_moments(m, **RULE) for m in first])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def one_round():
            det.enqueue_surface_refit(buf.ptr, F, gates, out_h.ptr)
            det.fetch_surface_refit()
            a = det.surface_refit_time_ms()
            e0.record()
            det.enqueue_surface_gates(mom.ptr, F, gates_d.ptr, **RULE)
            e1.record()
            e1.synchronize()
            b = e0.elapsed_time(e1)
            det.enqueue_surface_refit_device(buf.ptr, F, mom.ptr, out_d.ptr, **RULE)
            det.fetch_surface_refit()
            return a, b, det.surface_refit_time_ms()

        warm(one_round)
        took = [one_round() for _ in range(rounds)]
        assert gates_d.download(F * gsz).tobytes() == bytes(gates), "the kernel's gates are the host function's"
        assert out_d.download(F * rec).tobytes() == out_h.download(F * rec).tobytes(), "both passes give the same records"
        a, b, c = ([t[k] for t in took] for k in range(3))
        lines.append("%4d frames  host-gated pass (ssd_get_surface_refit_time)    %s ms" % (F, spread(a)))
        lines.append("%4d frames  k_surface_gates alone (events)                 %s ms" % (F, spread(b)))
        lines.append("%4d frames  device-gated pass (kernel included)            %s ms" % (F, spread(c)))
        lines.append("%4d frames  k_surface_gates / host-gated pass = %.4f; device-gated pass / host-gated pass = %.4f"
                     % (F, statistics.median(b) / statistics.median(a), statistics.median(c) / statistics.median(a)))
    finally:
        for x in bufs:
            x.free()
        det.close()


def host_part(rounds, lines):
    F = 64
    scs = scenes.batch_scenes(ssd, W, H, F)
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    det = ssd.Detector(cfg, ssd.transformation_for_scene(scs[0]), 0)
    pinned = ssd.PinnedArray((F, H, W, 3), np.float32)
    try:
        pinned.array[...] = ssd.synth_host(scs)
        det.set_timing(True)
        for passes in (1, 2, 4):
            def leg(device_gates):
                c0 = time.perf_counter()
                got = det.process_host_surfaces_refit(pinned.array, passes=passes, moments=True, device_gates=device_gates, **RULE)
                return (time.perf_counter() - c0) * 1e3, got

            def one_round():
                a, x = leg(False)
                b, y = leg(True)
                assert [[bytes(v) for v in p] for p in x] == [[bytes(v) for v in p] for p in y], "both legs give the same bytes"
                return a, b

            warm(one_round)
            took = [one_round() for _ in range(rounds)]
            a, b = [t[0] for t in took], [t[1] for t in took]
            lines.append("passes %d  device_gates=False %s ms   device_gates=True %s ms   True / False = %.3f"
                         % (passes, spread(a), spread(b), statistics.median(b) / statistics.median(a)))
    finally:
        pinned.free()
        det.close()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "surface_gates_time.txt")
    bench_lines = sys.argv[3] if len(sys.argv) > 3 else None
    lines = ["# tools/surface_gates_time.py %d: timing on, half a second of warm-up per part, legs alternating within a round, %d rounds;" % (rounds, rounds),
             "# median (min .. max)", "", "## (i) k_surface_gates on a resident XGA batch (vertices), beside a refit pass of the same handle"]
    for F in (256, 1024):
        kernel_part(rounds, F, lines)
    lines += ["", "## (ii) process_host_surfaces_refit, XGA, 64 frames from pinned memory (two slices of 32): wall time per call"]
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
