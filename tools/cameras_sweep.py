#!/usr/bin/env python3
"""tools/cameras_sweep.py [N_BATCHES] [SEED] [OUT] - randomised sweep of cameras batches (ssd_enqueue_cameras) on the GPU box, in the
manner of tools/labels_sweep.py: every frame of a batch has a camera of its own (random height, pitch, roll; random stair geometry,
noise, outliers, invalid pixels, 0-8 steps), vertex or 16-bit depth input per batch (depth: its own field of view and depth unit
as well), VGA or XGA, one or three workspaces, single pass forced in half of the batches.  Every frame's result against the oracle
with THAT frame's calibration (oracle.process_lean; corners identical, heights to 1e-9 m, the serialized line).
Writes a line per batch and a JSON line with the frame count and the mismatches (0 expected) to OUT (default
profiles/cameras_sweep.txt); exit status 1 on any mismatch.  TEST INFRASTRUCTURE (uses tests/parity.py and the oracle)."""
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
import parity  # noqa: E402

SIZES = [((640, 480), 64), ((1024, 768), 32)]


def main():
    n_batches = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "cameras_sweep.txt")
    rng = np.random.default_rng(seed)
    oracle = ob.load_oracle()
    cores = min(len(os.sched_getaffinity(0)), 16)
    total = bad = depth_frames = 0
    lines, failures, hist = [], [], {}
    for batch in range(n_batches):
        (W, H), F = SIZES[int(rng.integers(0, len(SIZES)))]
        depth_in = bool(rng.random() < 0.5)
        kws = [dict(n_steps=int(rng.integers(0, 9)), seed=int(rng.integers(1, 2**31)), cam_height=float(rng.uniform(0.7, 1.5)),
                    pitch_deg=float(rng.uniform(35.0, 62.0)), roll_deg=float(rng.uniform(-4.0, 4.0)),
                    first_riser_y=float(rng.uniform(0.15, 0.7)), tread=float(rng.uniform(0.12, 0.4)), rise=float(rng.uniform(0.08, 0.22)),
                    stair_width=float(rng.uniform(0.4, 1.5)), yaw_deg=float(rng.uniform(-12.0, 12.0)), sigma=float(rng.uniform(0.0, 0.004)),
                    outlier_frac=float(rng.choice([0.0, 0.0, 0.01, 0.05])), invalid_frac=float(rng.choice([0.0, 0.0, 0.02])),
                    hfov_deg=float(rng.uniform(58.0, 72.0)) if depth_in else 70.0) for _ in range(F)]
        units = [float(rng.choice([0.00025, 0.0001, 0.0005])) for _ in range(F)]
        scs = [ssd.make_scene(W, H, **kw) for kw in kws]
        trans = [ssd.transformation_for_scene(sc) for sc in scs]
        intr = [ssd.intrinsics_for_scene(sc, depth_units=u) for sc, u in zip(scs, units)]
        cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=int(rng.choice([1, 3])))
        det = ssd.Detector(cfg, ssd.GeometricTransformation(), 0)       # the handle's own calibration: none of the cameras'
        det.set_cameras([(t, i) for t, i in zip(trans, intr)] if depth_in else trans)
        forced = bool(rng.random() < 0.5)
        det.single_pass(1 if forced else 0)
        perm = rng.permutation(F)                                       # frame k comes from camera perm[k]
        if depth_in:
            frames = np.stack([ssd.synth_depth_host([scs[j]], depth_units=units[j])[0] for j in perm])
        else:
            frames = np.stack([ssd.synth_host([scs[j]])[0] for j in perm])
        buf = ssd.DeviceBuffer(frames.nbytes, 0)
        buf.upload(frames)
        det.enqueue_cameras(buf.ptr, F, perm.astype(np.uint16), depth=depth_in)
        res = det.fetch_list(F)
        buf.free()
        det.close()
        ocfg = ob.to_oracle_config(cfg)

        def check(k):
            j = int(perm[k])
            xyz = oracle.deproject(intr[j], frames[k]) if depth_in else frames[k]
            try:
                parity.compare_results_only(ssd, oracle, res[k], oracle.process_lean(ocfg, ob.to_oracle_calibration(trans[j].constants), xyz))
                return k, None
            except parity.Mismatch as e:
                return k, str(e)
        with ThreadPoolExecutor(cores) as pool:
            for k, err in pool.map(check, range(F)):
                total += 1
                depth_frames += 1 if depth_in else 0
                key = "throw" if res[k].status & ssd.ST_THROW else str(res[k].n_steps)
                hist[key] = hist.get(key, 0) + 1
                if err:
                    bad += 1
                    failures.append({"batch": batch, "res": [W, H], "frame": k, "camera": int(perm[k]), "scene": kws[int(perm[k])],
                                     "depth_input": depth_in, "error": err[:300]})
        lines.append("batch %d %dx%d x%d%s%s -> %d frames, %d mismatches so far" % (batch, W, H, F, " depth16" if depth_in else "",
                                                                                 " single pass" if forced else "", total, bad))
        print(lines[-1], flush=True)
    summary = json.dumps({"frames": total, "depth_frames": depth_frames, "mismatches": bad, "steps_histogram": hist, "failures": failures[:20]})
    print(summary)
    with open(out_path, "w") as f:
        f.write("# tools/cameras_sweep.py %d %d: one camera per frame, every frame against the oracle with its own calibration\n" % (n_batches, seed))
        f.write("\n".join(lines) + "\n" + summary + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
