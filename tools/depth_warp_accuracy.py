#!/usr/bin/env python3
"""tools/depth_warp_accuracy.py [OUT] - what the depth warp (ssd_depth_warp_host) achieves, measured on the host
statements and the oracle alone (the device is held to the host statement byte for byte, so no GPU is needed): the 3-step scene at
256 x 192, depth unit 0.00025 m, seen from five poses (tests/warp_model.py: ACC_POSES - the target, then four that differ from it by up to
1 degree of pitch, 0.5 of roll, 2 cm of height and 3 cm along the floor), sigma 2 mm, 5 % outliers, 2 % invalid pixels, seeds 1000 .. 1004.
Everything is compared with the clean frame of the target pose, over the pixels that are valid there: the share of them that are valid,
of those the share more than 40 raw units off, and the rms of the rest.  Then the warped-and-fused frame through the CPU oracle beside
the target's clean frame.
Writes profiles/depth_warp_accuracy.txt (or OUT); tests/test_depth_warp.py holds the host statement to the conditions these figures meet.
TEST INFRASTRUCTURE (uses tests/warp_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import warp_model as wm  # noqa: E402
import oracle_binding  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_warp_accuracy.txt")
    a = wm.accuracy_figures(ssd)
    lines = ["# tools/depth_warp_accuracy.py: %d x %d, 3 steps, poses (pitch deg, roll deg, height m, along the floor m) %s;"
             % (wm.ACC_W, wm.ACC_H, " ".join(str(p) for p in wm.ACC_POSES)),
             "# host statements only; against the clean frame of the first pose, over its valid pixels",
             "# frame | valid, %% | of those > %d raw units off, %% | rms of the rest, raw units" % wm.ACC_FAR]
    row = lambda name, f: " %-58s | %s | %s | %s" % (name, "%.2f" % (100 * f[0]), "%.3f" % (100 * f[1]), "%.2f" % f[2])   # noqa: E731
    lines.append(row("single noisy frame of the target pose", a["single"]))
    lines.append(row("fuse of the five noisy frames as they are", a["unwarped"]))
    lines.append(row("warp each to the target view, then fuse", a["warped_fused"]))
    for k, f in enumerate(a["clean"]):
        lines.append(row("clean frame of pose %d warped" % (k + 1), f))
    for k, f in enumerate(a["clean_unwarped"]):
        lines.append(row("clean frame of pose %d as it is" % (k + 1), f))
    oracle = oracle_binding.load_oracle()
    d = wm.detection_figures(ssd, oracle, a)
    lines += ["# the oracle over the deprojected frames, the target's calibration (no condition):",
              "clean_steps = %d   heights %s" % (d["clean_steps"], " ".join("%.6f" % h for h in d["clean_heights"])),
              "warped_fused_steps = %d   heights %s" % (d["fused_steps"], " ".join("%.6f" % h for h in d["fused_heights"])),
              "warped_fused_worst_height_difference_m = %.3e" % d["worst"]]
    s = wm.solved_figures(ssd, oracle, a)
    d = s["detection"]
    lines += ["# the same with the views from ssd_stair_pose_solve's calibrations in place of the true poses (no condition): every pose's noisy",
              "# frame located against the map of the target's clean frame, three passes from the prior 'the camera has not moved'",
              "# (tests/warp_model.py, solved_views); status 0 = GF_OK; view error: rotation in degrees, translation in metres against the true view",
              "solved_status = %s   passes_ok = %s" % (" ".join(str(x) for x in s["status"]), " ".join(str(x) for x in s["passes"])),
              "solved_view_error = %s" % "  ".join("%.3f deg %.4f m" % e for e in s["view_error"]),
              "solved_warped_fused_pixels = valid %.2f %%  far %.3f %%  rms %.2f" % (100 * s["pixels"][0], 100 * s["pixels"][1], s["pixels"][2]),
              "solved_warped_fused_steps = %d   heights %s" % (d["fused_steps"], " ".join("%.6f" % h for h in d["fused_heights"])),
              "solved_warped_fused_worst_height_difference_m = %.3e" % d["worst"]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
