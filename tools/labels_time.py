#!/usr/bin/env python3
"""Per-pixel labels: what they cost.  For XGA x 1024, FHD stress x 64 and depth-16 x 1024 (frames resident in device memory,
BATCHES_IN_FLIGHT_THROUGHPUT), prints one JSON line each:
  labels_ms      k_labels' device time (ssd_get_labels_time_back), median over the timed batches
  bytes          what it must move: the points of the cells it walks plus W H written.  The walked cells are bounded from below
                 by those holding a non-zero label and from above by all cells (the exact set lies in K1's cell records)
  floor_ms       those bytes over 8 TB/s
  fps_plain / fps_labels   frames/s of enqueue + fetch_back loops without and with labels, alternating on the same box
Usage: python tools/labels_time.py [--reps 20] [--rounds 3]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import importlib  # noqa: E402

ssd = importlib.import_module("stair-step-detector_amd")
import scenes  # noqa: E402

CELL = 64


def loop(det, n, reps, enqueue):
    """enqueue ahead, fetch the one before: frames/s over `reps` batches"""
    enqueue()
    t0 = time.perf_counter()
    for _ in range(reps):
        enqueue()
        det.fetch(n, back=1)
    det.fetch(n, back=0)
    return reps * n / (time.perf_counter() - t0)


def case(name, reps, rounds):
    depth = name == "depth1024"
    if name == "fhd64":
        W, H, n = 1920, 1080, 64
        scs = scenes.fhd_stress_scenes(ssd, n)
    else:
        W, H, n = 1024, 768, 1024
        scs = scenes.batch_scenes(ssd, W, H, n)
    wh = W * H
    cfg = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=ssd.BATCHES_IN_FLIGHT_THROUGHPUT)
    det = ssd.Detector(cfg, ssd.transformation_for_scene(scs[0]), 0)
    fb = wh * (2 if depth else 12)
    buf = ssd.DeviceBuffer(fb * n, 0)
    lbuf = ssd.DeviceBuffer(wh * n, 0)
    if depth:
        det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
        ssd.synth_depth_device(scs, buf.ptr)
        plain = lambda: det.enqueue_depth(buf.ptr, n)
        labelled = lambda: det.enqueue_depth_labels(buf.ptr, n, lbuf.ptr)
    else:
        ssd.synth_device(scs, buf.ptr)
        plain = lambda: det.enqueue(buf.ptr, n)
        labelled = lambda: det.enqueue_labels(buf.ptr, n, lbuf.ptr)
    for f in (plain, labelled):
        loop(det, n, 2, f)
    fps_p, fps_l = [], []
    for _ in range(rounds):
        fps_p.append(loop(det, n, reps, plain))
        fps_l.append(loop(det, n, reps, labelled))
    det.set_timing(True)
    ms = []
    for _ in range(reps):
        labelled()
        det.fetch(n)
        ms.append(det.labels_time_ms(0))
    lab = lbuf.download(wh * n).reshape(n, wh)
    ncell = (wh + CELL - 1) // CELL
    pad = np.zeros((n, ncell * CELL - wh), dtype=np.uint8)
    cells_labelled = int(np.concatenate([lab, pad], 1).reshape(n, ncell, CELL).any(2).sum())
    pt = 2 if depth else 12
    lo = cells_labelled * CELL * pt + n * wh
    hi = n * ncell * CELL * pt + n * wh
    out = dict(case=name, frames=n, labels_ms=statistics.median(ms), bytes_min=lo, bytes_max=hi,
               floor_ms_min=lo / 8e12 * 1e3, floor_ms_max=hi / 8e12 * 1e3,
               fps_plain=statistics.median(fps_p), fps_labels=statistics.median(fps_l),
               ratio=statistics.median(fps_l) / statistics.median(fps_p))
    buf.free()
    lbuf.free()
    det.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="xga1024,fhd64,depth1024")
    a = ap.parse_args()
    for c in a.cases.split(","):
        print(json.dumps(case(c, a.reps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
