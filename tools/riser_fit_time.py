#!/usr/bin/env python3
"""tools/riser_fit_time.py [ROUNDS] [OUT] - what the riser moments cost on top of the riser pass, on one box, legs alternated, with the
bench scenes (scenes.batch_scenes), one XGA x 256 batch resident in device memory, as vertices and as 16-bit depth.  The device time of
the last stage (ssd_get_stage_times: `final` spans k_final and, behind it, the riser pass) is read in three settings per input:
  off      risers off: k_final alone
  risers   risers on, moments off: k_final + k_risers + k_riser_results (the parent's pass, its code object unchanged)
  moments  risers on, moments on: k_final + the records' memset + k_riser_moments + k_riser_results
so the riser pass is (risers - off) and the fused walk (moments - off); their ratio is what one fused walk costs over the count-only
walk.  The yardstick is the parent's pass on the same batch in the same run; nothing is fixed in advance.  Also checks that results
and risers are byte for byte the same with the moments on.  Writes profiles/riser_fit_time.txt (or OUT).
TEST INFRASTRUCTURE (uses tests/scenes.py)."""
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

W, H, F = 1024, 768, 256
SETTINGS = ("off", "risers", "moments")


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "riser_fit_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    intr = ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F)
    bufs = {"vertices": ssd.DeviceBuffer(F * W * H * 12, 0), "depth16": ssd.DeviceBuffer(F * W * H * 2, 0)}
    ssd.synth_device(scs, bufs["vertices"].ptr, device=0)
    ssd.synth_depth_device(scs, bufs["depth16"].ptr, device=0)
    ssd.lib().ssd_device_sync(0)
    det = ssd.Detector(cfg, trans, 0)
    det.set_intrinsics(intr)
    det.set_timing(True)

    def run(inp, setting):
        det.set_risers(setting != "off", tolerance=0.03, min_support=200)
        det.set_riser_moments(setting == "moments")
        (det.enqueue_depth if inp == "depth16" else det.enqueue)(bufs[inp].ptr, F)
        res = [bytes(r) for r in det.fetch_list(F)]
        ris = [bytes(r) for r in det.fetch_risers(F)] if setting != "off" else None
        return float(det.stage_times_ms(0)["final"]), res, ris

    lines = ["# tools/riser_fit_time.py %d: one XGA x %d batch resident in device memory, one workspace, tolerance 0.03 m; device time of the last"
             % (rounds, F), "# stage (k_final + the riser pass) per setting, ms; inputs and settings alternated"]
    c0 = time.perf_counter()
    while time.perf_counter() - c0 < 0.5:                                 # warm-up: load until the device has been busy a while
        run("vertices", "moments")
    same = True
    evidence = 0
    for inp in bufs:
        _, res_r, ris_r = run(inp, "risers")
        _, res_m, ris_m = run(inp, "moments")
        same = same and res_r == res_m and ris_r == ris_m
        mom = det.fetch_riser_moments(F)
        evidence = sum(int(m.s[k].m.n + m.s[k].n_far) for m in mom for k in range(m.n_surfaces))
        lines.append("%s: results and risers with the moments on == off, byte for byte: %s; %d evidence points in the batch, %.1f per frame"
                     % (inp, res_r == res_m and ris_r == ris_m, evidence, evidence / F))
    t = {(inp, s): [] for inp in bufs for s in SETTINGS}
    for r in range(rounds):
        for inp in bufs:
            for s in SETTINGS:
                t[(inp, s)].append(run(inp, s)[0])
        lines.append("round %d: " % r + "; ".join("%s " % inp + " ".join("%s %.4f" % (s, t[(inp, s)][-1]) for s in SETTINGS) for inp in bufs))
    for inp in bufs:
        med = {s: float(np.median(t[(inp, s)])) for s in SETTINGS}
        walk, fused = med["risers"] - med["off"], med["moments"] - med["off"]
        lines.append("%s median ms: off %.4f, risers %.4f, moments %.4f" % (inp, med["off"], med["risers"], med["moments"]))
        lines.append("%s_riser_pass_ms = %.4f" % (inp, walk))
        lines.append("%s_riser_pass_with_moments_ms = %.4f" % (inp, fused))
        lines.append("%s_ratio = %.3f" % (inp, fused / walk if walk > 0 else float("nan")))
    det.close()
    for b in bufs.values():
        b.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
