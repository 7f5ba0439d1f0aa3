#!/usr/bin/env python3
"""tools/depth_fuse_accuracy.py [OUT] - what the depth fusion (ssd_depth_fuse_host) achieves, measured on the host
statement and the oracle alone (the device is held to the host statement byte for byte, so no GPU is needed): the 3-step scene at
256 x 192, depth unit 0.00025 m, frames that differ in their noise alone (seeds 1000 ..), the default rule for n, against the frame
without noise.  (a) per pixel: the share of valid pixels more than 40 raw units off, the rms of the rest, the share of invalid pixels,
single frame -> fused; (b) the eight frames of the third row through the CPU oracle one by one and fused: step counts, and the worst
step height error against the clean frame's detection.
Writes profiles/depth_fuse_accuracy.txt (or OUT); tests/test_depth_fuse.py holds the host statement to the conditions these figures meet.
TEST INFRASTRUCTURE (uses tests/fuse_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import fuse_model as fm  # noqa: E402
import oracle_binding  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_fuse_accuracy.txt")
    lines = ["# tools/depth_fuse_accuracy.py: %d x %d, 3 steps, seeds 1000 .. 1000 + n - 1, default rule (min_valid = min_agree = (n + 1) / 2, tol 40);"
             % (fm.ACC_W, fm.ACC_H),
             "# host statement only.  Per row: single frame -> fused",
             "# sigma_mm outliers invalid  n | valid pixels > %d raw units off, %% | rms of the rest, raw units | invalid pixels, %% | fused few split |"
             " sum_abs_dev / sum_agree" % fm.ACC_FAR]
    for r in fm.accuracy_rows(ssd):
        s, f, st = r["single"], r["fused"], r["stats"]
        lines.append("%8.1f %8.2f %7.2f %2d | %6.3f -> %6.3f | %6.2f -> %5.2f | %6.2f -> %5.2f | %d %d %d | %.3f"
                     % (r["sigma"] * 1e3, r["outliers"], r["invalid"], r["n"], 100 * s[0], 100 * f[0], s[1], f[1], 100 * s[2], 100 * f[2],
                        st["n_fused"], st["n_few"], st["n_split"], st["sum_abs_dev"] / max(st["sum_agree"], 1)))
    d = fm.detection_figures(ssd, oracle_binding.load_oracle())
    lines += ["# the oracle over the deprojected frames of the third row (sigma 2 mm, 5 % outliers, 2 % invalid, n = 8):",
              "clean_steps = %d   heights %s" % (d["clean_steps"], " ".join("%.6f" % h for h in d["clean_heights"])),
              "single_steps = %s" % " ".join(str(n) for n in d["single_steps"]),
              "single_worst_height_error_m = %s" % " ".join("%.3e" % e for e in d["single_worst"]),
              "fused_steps = %d" % d["fused_steps"],
              "fused_worst_height_error_m = %.3e" % d["fused_worst"]]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
