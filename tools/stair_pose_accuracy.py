#!/usr/bin/env python3
"""tools/stair_pose_accuracy.py [OUT] - what the stair pose (ssd_stair_pose_host, ssd_stair_pose_add, ssd_stair_pose_solve; DESIGN.md
section 7q) recovers, measured on the host functions and the oracle alone (the device is held to the host sums bit for bit, so no GPU is
needed): the 3-step scene at 256 x 192 under tests/camera_drift_model.py's seeds and noises, against the median map of the oracle's
results.  (a) the fit from the TRUE prior - the map's own bias, its drawn edges against the faces; (b) the fits from priors off by 2 deg
of yaw, 3 cm along the going, 1 deg of pitch, 2 cm of height, each alone and all together, after 1, 2 and 3 chained passes, as distances
from (a)'s pose in the five components a straight staircase observes; and the scaled spectra SSD_SP_OBSERVABLE is taken from.
Writes profiles/stair_pose_accuracy.txt (or OUT); tests/test_stair_pose.py holds the code to the figures recorded there.
TEST INFRASTRUCTURE (uses tests/stair_pose_model.py and the CPU oracle)."""
import importlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import camera_drift_model as cd  # noqa: E402
import oracle_binding  # noqa: E402
import stair_pose_model as spm  # noqa: E402


def row(values):
    return " ".join("%.3e" % abs(v) for v in values)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else spm.ACCURACY_FILE
    r = spm.recipe(ssd, oracle_binding.load_oracle())
    lines = ["# tools/stair_pose_accuracy.py: %d x %d, 3 steps, %d frames (seed, sigma: %s) folded, the median map of the oracle's results;"
             % (spm.ground_model.W, spm.ground_model.H, len(cd.FRAMES), ", ".join("%d %g mm" % (s, g * 1e3) for s, g in cd.FRAMES)),
             "# rule margin %g band %g clear %g reach %g, min_points %d, %d chained passes; host functions only" % (spm.RULE + (spm.MIN_POINTS, spm.PASSES)),
             "# components: %s - |values|, against the pose named" % ", ".join(spm.COMPONENTS),
             "# (a) from the TRUE prior: %d points, rms %.3e m before the first pass, %.3e m behind the last" % (r["n"], r["rms"][0], r["rms"][1]),
             "#   (a)'s pose against the true calibration, the map's own bias: %s   (after one pass: %s)" % (row(r["bias"]), row(r["first_pass"])),
             "#   scaled spectrum lambda / lambda_max of its first pass: %s" % " ".join("%.3e" % v for v in r["spectrum_true"]),
             "# (b) offset priors, against (a)'s pose:"]
    worst = [0.0] * 5
    nearer = True
    for name, c in r["cases"].items():
        lines.append("#   %s: begins %s" % (name, row(c["begin"])))
        for k, (after, spec) in enumerate(zip(c["after"], c["spectra"])):
            lines.append("#     after pass %d (status %d, dof %d, %d points): %s   spectrum %s"
                         % (k + 1, c["status"][k], c["dof"][k], c["n"][k], row(after), " ".join("%.2e" % v for v in spec)))
        if len(c["after"]) == spm.PASSES:
            worst = [max(a, abs(b)) for a, b in zip(worst, c["after"][-1])]
            nearer = nearer and all(abs(e) < abs(b) for e, b in zip(c["after"][-1], c["begin"]))
        else:
            nearer = False
    lines.append("# every offset prior ends nearer to (a)'s pose than it began, in each observed component: %s" % ("yes" if nearer else "NO"))
    for name, v in zip(("pitch_rad", "roll_rad", "yaw_rad", "going_m", "height_m"), worst):
        lines.append("worst_end_%s = %.3e" % (name, v))
    for name, v in zip(("pitch_rad", "roll_rad", "yaw_rad", "going_m", "height_m"), r["bias"]):
        lines.append("bias_%s = %.3e" % (name, abs(v)))
    lo = r["unobserved_max"]
    lines.append("# the spectra above: the largest ratio of the direction a straight staircase does not observe, the smallest of one it does")
    lines.append("unobserved_max = %.3e" % lo)
    lines.append("observed_min = %.3e" % r["observed_min"])
    floor = max(lo, spm.ROUNDING)
    if lo < spm.ROUNDING:
        lines.append("# the unobserved ratio lies below the solve's rounding level 64 eps = %.3e (the median map's drawn edges are exactly parallel"
                     % spm.ROUNDING)
        lines.append("# here), which no eigenvalue is told from zero below: that level stands in for it in the geometric mean")
    lines.append("observable = %.1e" % math.sqrt(floor * r["observed_min"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
