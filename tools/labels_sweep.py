#!/usr/bin/env python3
"""tools/labels_sweep.py [N_BATCHES] [SEED] — randomised sweep of the per-pixel labels (k_labels) on the GPU box: random camera poses and
stair geometries as tools/fuzz.py draws them (yaw up to +-45 degrees, roll, noise, outliers, invalid pixels, 0-8 steps), four
resolutions, vertex or 16-bit depth input per batch, frames resident in device memory, debug records on.  Every frame: no label above
n_steps, all zero on THROW or n_steps == 0, and per emitted surface the count of its label and the fixed-point mean of its points' world z
equal the record's n_in_quad / ground_n_in_quad and mean_z / ground_mean_z and the result's height less world_z (world_z alone for a
ground without front edge, quirk Q6), bit for bit.
Prints a line per batch and one JSON line at the end; exit status 1 on any mismatch.  TEST INFRASTRUCTURE (uses tests/test_labels.py)."""
import importlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import oracle_binding as ob  # noqa: E402
from test_labels import per_surface, same_double  # noqa: E402

SIZES = [((640, 480), 128), ((1024, 768), 64), ((600, 450), 128), ((1920, 1080), 16)]


def check_frame(cal, xyz, lab, r, d):
    """None, or what differs"""
    if (r.status & ssd.ST_THROW) or r.n_steps == 0:
        return None if not lab.any() else "labels in a frame without surfaces"
    if int(lab.max()) > r.n_steps:
        return "label %d above n_steps %d" % (int(lab.max()), r.n_steps)
    ground = d.ground_ind >= 0
    steps = [k for k in range(d.first_valid_ind, d.n_plateaus) if d.plateaus[k].valid]
    for s, (cnt, mean) in enumerate(per_surface(cal, xyz, lab, r.n_steps)):
        if ground and s == 0:
            want_n, want_mean = d.ground_n_in_quad, d.ground_mean_z
        else:
            k = steps[s - (1 if ground else 0)]
            want_n, want_mean = d.plateaus[k].n_in_quad, d.plateaus[k].mean_z
        if cnt != want_n:
            return "surface %d: %d labelled, record %d" % (s, cnt, want_n)
        # the result's height: world_z + the mean, but world_z alone for a ground whose front edge was not found (quirk Q6: the
        # reference's "return {}", an all-zero ground) - its labels still mark the points the record counts
        height = cal.world_z + (0.0 if ground and s == 0 and not d.ground_front_valid else mean)
        if cnt and not (same_double(mean, want_mean) and same_double(height, r.steps[s].height)):
            return "surface %d: mean %r, record %r, height %r" % (s, mean, want_mean, r.steps[s].height)
    return None


def main():
    n_batches = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.default_rng(seed)
    oracle = ob.load_oracle()
    cores = min(len(os.sched_getaffinity(0)), 16)
    total = bad = thrown = depth_frames = 0
    hist, failures = {}, []
    for batch in range(n_batches):
        (W, H), F = SIZES[int(rng.integers(0, len(SIZES)))]
        cam_height, pitch, roll = float(rng.uniform(0.7, 1.5)), float(rng.uniform(35.0, 62.0)), float(rng.uniform(-4.0, 4.0))
        kws = [dict(n_steps=int(rng.integers(0, 9)), seed=int(rng.integers(1, 2**31)), cam_height=cam_height, pitch_deg=pitch,
                    roll_deg=roll, first_riser_y=float(rng.uniform(0.15, 0.7)), tread=float(rng.uniform(0.12, 0.4)),
                    rise=float(rng.uniform(0.08, 0.22)), stair_width=float(rng.uniform(0.4, 1.5)),
                    yaw_deg=float(rng.uniform(-45.0, 45.0)) if rng.random() < 0.5 else float(rng.uniform(-10.0, 10.0)),
                    sigma=float(rng.uniform(0.0, 0.004)), outlier_frac=float(rng.choice([0.0, 0.0, 0.01, 0.05, 0.15])),
                    invalid_frac=float(rng.choice([0.0, 0.0, 0.02, 0.2]))) for _ in range(F)]
        scenes = [ssd.make_scene(W, H, **kw) for kw in kws]
        trans = ssd.transformation_for_scene(scenes[0])
        cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=int(rng.choice([1, 3])))
        depth_in = rng.random() < 0.5
        det = ssd.Detector(cfg, trans, 0)
        det.set_debug(True, images=False)
        wh = W * H
        buf = ssd.DeviceBuffer(F * wh * (2 if depth_in else 12), 0)
        lbuf = ssd.DeviceBuffer(F * wh, 0)
        if depth_in:
            intr = ssd.intrinsics_for_scene(scenes[0])
            det.set_intrinsics(intr)
            ssd.synth_depth_device(scenes, buf.ptr, device=0)
            det.enqueue_depth_labels(buf.ptr, F, lbuf.ptr)
        else:
            ssd.synth_device(scenes, buf.ptr, device=0)
            det.enqueue_labels(buf.ptr, F, lbuf.ptr)
        res = det.fetch_list(F)
        recs = [det.debug(i) for i in range(F)]
        lab = lbuf.download(F * wh).reshape(F, wh)
        buf.free()
        lbuf.free()
        det.close()

        def host(i):
            if depth_in:
                return oracle.deproject(intr, ssd.synth_depth_host([scenes[i]])[0])
            return ssd.synth_host([scenes[i]])[0]      # bit-identical to the device generator (tested)

        def check(i):
            return i, check_frame(trans.constants, host(i), lab[i], res[i], recs[i])
        with ThreadPoolExecutor(cores) as pool:
            for i, err in pool.map(check, range(F)):
                total += 1
                depth_frames += 1 if depth_in else 0
                key = "throw" if res[i].status & ssd.ST_THROW else str(res[i].n_steps)
                hist[key] = hist.get(key, 0) + 1
                thrown += 1 if res[i].status & ssd.ST_THROW else 0
                if err:
                    bad += 1
                    failures.append({"batch": batch, "res": [W, H], "frame": i, "scene": kws[i], "cam": [cam_height, pitch, roll],
                                     "depth_input": bool(depth_in), "error": err[:300]})
        print("batch %d %dx%d x%d%s -> %d frames, %d mismatches so far" % (batch, W, H, F, " depth16" if depth_in else "", total, bad), flush=True)
    print(json.dumps({"frames": total, "depth_frames": depth_frames, "mismatches": bad, "would_have_thrown": thrown,
                      "steps_histogram": hist, "failures": failures[:20]}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
