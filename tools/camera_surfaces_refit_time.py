#!/usr/bin/env python3
"""tools/camera_surfaces_refit_time.py [ROUNDS] [OUT] - what the cameras refit pass (k_surface_refit_cams) costs
beside its yardstick, the one-calibration pass (k_surface_refit, whose code is the parent commit's), on the same batch in the same
run: XGA x 256 frames resident in device memory (scenes.batch_scenes, the bench's), as vertices and as 16-bit depth, one workspace,
timing on.  Three handles share the frames: one created with the calibration, one with a camera table of ONE entry (every frame names
camera 0: the record's loads hit one line), one with a table of one camera PER FRAME (the same calibration 256 times: every block
fetches another record).  Each runs its whole enqueue once; a round is one refit pass per handle, gated at 2.5 rms by the first pass's
planes - so the legs alternate, after bench.py's half-second warm-up.  A pass's time (ssd_get_surface_refit_time) includes the memset
of the records in front of the kernel.  The three passes must give the same records.  The expectation is "about its sibling".
Writes profiles/camera_surfaces_refit_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
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
LEGS = ("k_surface_refit", "k_surface_refit_cams, 1 camera", "k_surface_refit_cams, %d cameras" % F)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 25
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "camera_surfaces_refit_time.txt")
    if rounds < 15:
        raise SystemExit("at least 15 rounds")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    wh, rec = W * H, C.sizeof(ssd.FrameMoments)
    lines = ["# tools/camera_surfaces_refit_time.py %d: XGA x %d resident frames, one workspace per handle, %d timed rounds; a round = one refit pass" % (rounds, F, rounds),
             "# per handle, one after the other (gates: 2.5 rms of the first pass).  ms per pass over %d frames, median (min .. max)" % F]
    for depth in (False, True):
        intr = ssd.intrinsics_for_scene(scs[0]) if depth else None
        cam = (trans, intr) if depth else trans
        dets = [ssd.Detector(cfg, trans, 0), ssd.Detector(cfg, ssd.GeometricTransformation(), 0), ssd.Detector(cfg, ssd.GeometricTransformation(), 0)]
        index = [None, [0] * F, list(range(F))]
        buf = ssd.DeviceBuffer(F * wh * (2 if depth else 12), 0)
        mom = ssd.DeviceBuffer(F * rec, 0)
        outs = [ssd.DeviceBuffer(F * rec, 0) for _ in dets]
        try:
            if depth:
                dets[0].set_intrinsics(intr)
                ssd.synth_depth_device(scs, buf.ptr, device=0)
            else:
                ssd.synth_device(scs, buf.ptr, device=0)
            ssd.lib().ssd_device_sync(0)
            dets[1].set_cameras([cam])
            dets[2].set_cameras([cam] * F)
            gates = None
            for det, idx in zip(dets, index):
                det.set_timing(True)
                if idx is None:
                    det.enqueue_surface_moments(buf.ptr, F, mom.ptr, depth=depth)
                else:
                    det.enqueue_cameras_surface_moments(buf.ptr, F, idx, mom.ptr, depth=depth)
                det.fetch(F)
                first = (ssd.FrameMoments * F).from_buffer_copy(np.ascontiguousarray(mom.download(F * rec)).tobytes())
                if gates is None:
                    ref, gates = bytes(first), (ssd.FrameGates * F)(*[ssd.surface_gates_from_moments(m, 200, 2.5, 0.0) for m in first])
                assert bytes(first) == ref, "the three handles' first passes agree"

            def one_round():
                took = []
                for det, idx, out in zip(dets, index, outs):
                    if idx is None:
                        det.enqueue_surface_refit(buf.ptr, F, gates, out.ptr, depth=depth)
                    else:
                        det.enqueue_cameras_surface_refit(buf.ptr, F, gates, out.ptr, depth=depth)
                    det.fetch_surface_refit()
                    took.append(det.surface_refit_time_ms())
                return took

            c0 = time.perf_counter()
            while time.perf_counter() - c0 < 0.5:                          # bench.py's warm-up: load until the device has been busy a while
                one_round()
            took = [one_round() for _ in range(rounds)]
            got = [out.download(F * rec).tobytes() for out in outs]
            assert got[0] == got[1] == got[2], "the three passes give the same records"
            tag = "depth16" if depth else "vertices"
            med = [statistics.median(t[k] for t in took) for k in range(3)]
            for k, leg in enumerate(LEGS):
                lines.append("%-8s %-34s %.3f (%.3f .. %.3f)" % (tag, leg, med[k], min(t[k] for t in took), max(t[k] for t in took)))
            lines.append("%-8s k_surface_refit_cams / k_surface_refit = %.3f (1 camera), %.3f (%d cameras)" % (tag, med[1] / med[0], med[2] / med[0], F))
        finally:
            for b in [buf, mom] + outs:
                b.free()
            for det in dets:
                det.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
