#!/usr/bin/env python3
"""tools/cameras_time.py [ROUNDS] [OUT] - what per-frame calibration costs and what it replaces, on one box, legs alternated, after
bench.py's half-second warm-up, with the bench scenes (scenes.batch_scenes), frames resident in device memory, three batches in
flight as bench.py keeps them.  Legs at XGA x 1024:
  plain    ssd_enqueue, the handle's one calibration
  cams1    ssd_enqueue_cameras with a table of ONE camera (the same calibration): the cost of the fetch alone
  cams1024 ssd_enqueue_cameras with 1024 cameras, one per frame (each scene's own transformation_for_scene); its results are
           checked against the oracle on every 64th frame, with that frame's calibration
and the status quo the feature replaces: 256 frames as 256 one-camera handles with one frame per call, against ONE 256-frame cameras
batch.  Writes profiles/cameras_time.txt (or OUT); bench.py's own figures of the parent and of this build are appended to that file
by whoever runs both (the tool cannot build the parent).  TEST INFRASTRUCTURE (uses tests/scenes.py, tests/parity.py, the oracle)."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import oracle_binding as ob  # noqa: E402
import parity  # noqa: E402
import scenes  # noqa: E402

W, H, F, DEPTH, STEPS = 1024, 768, 1024, 3, 10


def pipelined(enqueue, fetch, n_steps):
    ahead = DEPTH - 1
    for i in range(n_steps):
        enqueue()
        if i >= ahead:
            fetch(ahead)
    for back in range(min(ahead, n_steps) - 1, -1, -1):
        fetch(back)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "cameras_time.txt")
    oracle = ob.load_oracle()
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = [ssd.transformation_for_scene(sc) for sc in scs]
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=DEPTH)
    buf = ssd.DeviceBuffer(F * W * H * 12, 0)
    ssd.synth_device(scs, buf.ptr, device=0)
    ssd.lib().ssd_device_sync(0)
    det = ssd.Detector(cfg, trans[0], 0)
    det1 = ssd.Detector(cfg, trans[0], 0)
    det1.set_cameras([trans[0]])
    detN = ssd.Detector(cfg, ssd.GeometricTransformation(), 0)
    detN.set_cameras(trans)
    zeros, each = np.zeros(F, dtype=np.uint16), np.arange(F, dtype=np.uint16)
    legs = {"plain": (lambda: det.enqueue(buf.ptr, F), det), "cams1": (lambda: det1.enqueue_cameras(buf.ptr, F, zeros), det1),
            "cams1024": (lambda: detN.enqueue_cameras(buf.ptr, F, each), detN)}
    lines = ["# tools/cameras_time.py %d: XGA x %d resident frames, %d batches in flight, %d timed steps per leg and round, legs alternated" % (rounds, F, DEPTH, STEPS)]
    c0 = time.perf_counter()
    while time.perf_counter() - c0 < 0.5:                                 # bench.py's warm-up: load until the device has been busy a while
        pipelined(legs["plain"][0], lambda b: det.fetch(F, back=b), 4)
    for name, (enq, d) in legs.items():
        pipelined(enq, lambda b, d=d: d.fetch(F, back=b), 3)
    # the same bytes from the one-camera table as from the plain call; the 1024-camera batch against the oracle on every 64th frame
    det.enqueue(buf.ptr, F)
    plain = [bytes(r) for r in det.fetch_list(F)]
    det1.enqueue_cameras(buf.ptr, F, zeros)
    same = [bytes(r) for r in det1.fetch_list(F)] == plain
    detN.enqueue_cameras(buf.ptr, F, each)
    resN = detN.fetch_list(F)
    checked = bad = 0
    ocfg = ob.to_oracle_config(cfg)
    for i in range(0, F, 64):
        xyz = buf.download(W * H * 12, offset=i * W * H * 12, dtype=np.float32).reshape(H, W, 3)
        try:
            parity.compare_results_only(ssd, oracle, resN[i], oracle.process_lean(ocfg, ob.to_oracle_calibration(trans[i].constants), xyz))
        except parity.Mismatch as e:
            bad += 1
            lines.append("frame %d: %s" % (i, e))
        checked += 1
    lines.append("one-camera table == plain enqueue, byte for byte: %s; 1024 cameras: %d frames checked against the oracle, %d mismatches" % (same, checked, bad))
    rates = {k: [] for k in legs}
    for r in range(rounds):
        for name, (enq, d) in legs.items():
            ssd.lib().ssd_device_sync(0)
            t0 = time.perf_counter()
            pipelined(enq, lambda b, d=d: d.fetch(F, back=b), STEPS)
            ssd.lib().ssd_device_sync(0)
            rates[name].append(F * STEPS / (time.perf_counter() - t0))
        lines.append("round %d: " % r + ", ".join("%s %.1f k frames/s" % (k, v[-1] / 1e3) for k, v in rates.items()))
    med = {k: float(np.median(v)) for k, v in rates.items()}
    lines.append("median: " + ", ".join("%s %.1f k frames/s (min %.1f, max %.1f)" % (k, med[k] / 1e3, min(rates[k]) / 1e3, max(rates[k]) / 1e3) for k in legs))
    lines.append("cams1 / plain = %.4f, cams1024 / plain = %.4f (expected: within 5 %% of 1)" % (med["cams1"] / med["plain"], med["cams1024"] / med["plain"]))
    for d in (det, det1, detN):
        d.close()
    # the status quo: 256 cameras as 256 one-camera handles, one frame per call, against one 256-frame cameras batch
    n = 256
    cfg1 = ssd.default_config(W, H, max_frames_per_batch=1)
    handles = [ssd.Detector(cfg1, trans[i], 0) for i in range(n)]
    cfgB = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=DEPTH)
    detB = ssd.Detector(cfgB, ssd.GeometricTransformation(), 0)
    detB.set_cameras(trans[:n])
    idx = np.arange(n, dtype=np.uint16)
    fb = W * H * 12

    def tick_handles():
        for i, h in enumerate(handles):
            h.enqueue(buf.ptr + i * fb, 1)
        return [bytes(h.fetch(1)[0]) for h in handles]

    def tick_batch():
        detB.enqueue_cameras(buf.ptr, n, idx)
        return [bytes(r) for r in detB.fetch(n)]
    a, b = tick_handles(), tick_batch()
    lines.append("status quo, %d frames of %d cameras per tick: results equal byte for byte: %s" % (n, n, a == b))
    quo = {"handles": [], "batch": []}
    for r in range(rounds):
        for name, fn in (("handles", tick_handles), ("batch", tick_batch)):
            ssd.lib().ssd_device_sync(0)
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            quo[name].append(3 * n / (time.perf_counter() - t0))
    lines.append("median: 256 one-camera handles, one frame per call %.1f k frames/s; one 256-frame cameras batch %.1f k frames/s" %
                 (np.median(quo["handles"]) / 1e3, np.median(quo["batch"]) / 1e3))
    for h in handles:
        h.close()
    detB.close()
    buf.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 1 if bad or not same or a != b else 0


if __name__ == "__main__":
    sys.exit(main())
