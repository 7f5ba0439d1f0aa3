#!/usr/bin/env python3
"""tools/depth_fill_accuracy.py [OUT] - what the depth fill (ssd_depth_fill_host) achieves behind the depth warp,
measured on the host statements and the oracle alone (the device is held to the host statement byte for byte, so no GPU is needed): the
recipes of tests/warp_model.py unchanged - the 3-step scene at 256 x 192, depth unit 0.00025 m, its poses, noise and seeds -, the default
rule, one pass.  A view that magnifies (pull_near_view) is counted in pixels that are not 0; everything else is compared with the clean
frame of the target pose over the pixels that are valid there: the share of them that are valid, of those the share more than 40 raw
units off, and the rms of the rest.  Then two passes, and the warped, filled and fused frame through the CPU oracle beside the unfilled
chain's.
Writes profiles/depth_fill_accuracy.txt (or OUT); tests/test_depth_fill.py holds the host statement to the conditions these figures meet.
TEST INFRASTRUCTURE (uses tests/fill_model.py, tests/warp_model.py and the CPU oracle)."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import fill_model as fm  # noqa: E402
import warp_model as wm  # noqa: E402
import oracle_binding  # noqa: E402


def two_passes():
    """the two recipes with the widest cracks once more, filled once and twice: [(label, once, twice)]"""
    fill = lambda f: ssd.depth_fill_host(np.ascontiguousarray(f))[0]                                               # noqa: E731
    src = wm.scene_src(ssd, wm.ACC_W, wm.ACC_H)
    w = ssd.depth_warp_host(wm.scene_frames(ssd, wm.ACC_W, wm.ACC_H)[0], wm.pull_near_view(ssd, src, 0.4), src)[0]
    rows = [("pull_near_view 0.4 m: non-zero %", "%.2f" % (100 * (fill(w) != 0).mean()), "%.2f" % (100 * (fill(fill(w)) != 0).mean()))]
    near = ssd.synth_depth_host([wm.pose_scene(ssd, fm.APPROACH[0]), wm.pose_scene(ssd, fm.APPROACH[1])])
    adst = ssd.intrinsics_for_scene(wm.pose_scene(ssd, fm.APPROACH[1]))
    w = ssd.depth_warp_host(near[0], wm.pose_view(ssd, fm.APPROACH[0], fm.APPROACH[1]), adst)[0]
    cell = lambda t: "%.2f %.3f %.2f" % (100 * t[0], 100 * t[1], t[2])                                             # noqa: E731
    rows.append(("30 cm approach: valid %, far %, rms", cell(wm.against(fill(w), near[1])), cell(wm.against(fill(fill(w)), near[1]))))
    return rows


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_fill_accuracy.txt")
    a = fm.accuracy_figures(ssd)
    lines = ["# tools/depth_fill_accuracy.py: %d x %d, 3 steps, the recipes of tests/warp_model.py; host statements only; the default rule"
             % (wm.ACC_W, wm.ACC_H),
             "# (min_pairs 1, cover 1, tol %d, slope 0), ONE pass behind ssd_depth_warp_host; 'valid, far, rms': against the clean frame of the"
             % fm.DEFAULT["tol"],
             "# target pose over its valid pixels - valid %%, of those > %d raw units off %%, rms of the rest in raw units" % wm.ACC_FAR,
             "# case | before the fill | filled once"]
    for label, before, after in fm.accuracy_rows(a):
        lines.append(" %-64s | %s | %s" % (label, " ".join(before), " ".join(after)))
    lines += ["# two passes (no condition): cracks wider than one pixel close from their rims inwards, a pixel per pass and side",
              "# case | filled once | filled twice"]
    for label, once, twice in two_passes():
        lines.append("twice: %-57s | %s | %s" % (label, once, twice))
    oracle = oracle_binding.load_oracle()
    plain = wm.detection_figures(ssd, oracle, a["base"])
    filled = wm.detection_figures(ssd, oracle, dict(a["base"], warped=a["filled"]))
    lines += ["# the oracle over the deprojected n = 5 fused frames, the target's calibration (no condition):",
              "clean_steps = %d   heights %s" % (plain["clean_steps"], " ".join("%.6f" % h for h in plain["clean_heights"])),
              "warped_fused_steps = %d   heights %s" % (plain["fused_steps"], " ".join("%.6f" % h for h in plain["fused_heights"])),
              "warped_fused_worst_height_difference_m = %.3e" % plain["worst"],
              "warped_filled_fused_steps = %d   heights %s" % (filled["fused_steps"], " ".join("%.6f" % h for h in filled["fused_heights"])),
              "warped_filled_fused_worst_height_difference_m = %.3e" % filled["worst"]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
