#!/usr/bin/env python3
"""tools/camera_surfaces_time.py [ROUNDS] [OUT] - the device time of the surface-moments pass of a cameras batch beside the
one-calibration pass on the same batch, on one box, in alternating legs (ssd_get_surface_moments_time_back: HIP events around the
memset and the kernel), after a half-second warm-up, with the bench scenes (scenes.batch_scenes), frames resident in device memory.
No time is fixed in advance: the yardstick is the one-calibration k_surface_moments, whose code this build leaves as its parent has
it (profiles/camera_surfaces_kernel_resources.txt), in the same run.  Legs at XGA x 256:
  plain     ssd_enqueue_surface_moments, the handle's one calibration
  cams1     ssd_enqueue_cameras_surface_moments with a table of ONE camera (the same calibration, so the same points): its records
            must equal the plain leg's byte for byte; what is left is the cost of fetching the frame's record
  camsN     ssd_enqueue_cameras_surface_moments with one camera per frame (each scene's own transformation_for_scene)
Writes profiles/camera_surfaces_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import scenes  # noqa: E402

W, H, F, STEPS = 1024, 768, 256, 6


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "camera_surfaces_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = [ssd.transformation_for_scene(sc) for sc in scs]
    cfg = ssd.default_config(W, H, max_frames_per_batch=F)
    rec = C.sizeof(ssd.FrameMoments)
    buf = ssd.DeviceBuffer(F * W * H * 12, 0)
    out = ssd.DeviceBuffer(F * rec, 0)
    ssd.synth_device(scs, buf.ptr, device=0)
    ssd.lib().ssd_device_sync(0)
    det = ssd.Detector(cfg, trans[0], 0)
    det1 = ssd.Detector(cfg, ssd.GeometricTransformation(), 0)
    det1.set_cameras([trans[0]])
    detN = ssd.Detector(cfg, ssd.GeometricTransformation(), 0)
    detN.set_cameras(trans)
    zeros, each = np.zeros(F, dtype=np.uint16), np.arange(F, dtype=np.uint16)
    legs = {"plain": (lambda: det.enqueue_surface_moments(buf.ptr, F, out.ptr), det),
            "cams1": (lambda: det1.enqueue_cameras_surface_moments(buf.ptr, F, zeros, out.ptr), det1),
            "camsN": (lambda: detN.enqueue_cameras_surface_moments(buf.ptr, F, each, out.ptr), detN)}
    lines = ["# tools/camera_surfaces_time.py %d: XGA x %d resident frames, the pass's device time (memset + kernel), %d timed enqueues per leg and round, legs alternated"
             % (rounds, F, STEPS)]
    c0 = time.perf_counter()
    while time.perf_counter() - c0 < 0.5:                                 # load until the device has been busy a while
        legs["plain"][0]()
        det.fetch(F)
    records = {}
    for name, (enq, d) in legs.items():
        d.set_timing(True)
        enq()
        d.fetch(F)
        records[name] = out.download(F * rec).tobytes()
    same = records["cams1"] == records["plain"]
    folded = sum(1 for m in (ssd.FrameMoments * F).from_buffer_copy(records["camsN"]) if m.ground == 1 and m.n_surfaces >= 1)
    lines.append("one-camera table == the one-calibration pass, byte for byte: %s; one camera per frame: %d of %d frames report a ground" % (same, folded, F))
    times = {k: [] for k in legs}
    for r in range(rounds):
        for name, (enq, d) in legs.items():
            for _ in range(STEPS):
                enq()
                d.fetch(F)
            per = [d.surface_moments_time_ms(b) for b in range(STEPS)]
            times[name].append(float(np.median(per)))
        lines.append("round %d: " % r + ", ".join("%s %.4f ms" % (k, v[-1]) for k, v in times.items()))
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines.append("median: " + ", ".join("%s %.4f ms (min %.4f, max %.4f)" % (k, med[k], min(times[k]), max(times[k])) for k in legs))
    lines.append("cams1 / plain = %.4f, camsN / plain = %.4f" % (med["cams1"] / med["plain"], med["camsN"] / med["plain"]))
    for d in (det, det1, detN):
        d.close()
    buf.free()
    out.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
