#!/usr/bin/env python3
"""tools/ground_fit_accuracy.py [OUT] - how close the ground fit comes to the true pose, measured on the host functions
(ssd_ground_moments_host + ssd_ground_fit_solve; the device is held to them bit for bit, so no GPU is needed): the cases of
tests/ground_model.py (3-step scene at 256 x 192, sigma 1 mm and 3 mm, priors off by +-(3 deg, 2 deg, 4 cm)), three passes at the
default tolerances against ONE pass at the widest.  Writes profiles/ground_fit_accuracy.txt (or OUT); tests/test_ground_fit.py asserts
three times the worst figures recorded there.  TEST INFRASTRUCTURE (uses tests/ground_model.py)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import ground_model as gm  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else gm.ACCURACY_FILE
    lines = ["# tools/ground_fit_accuracy.py: %d x %d, 3 steps, tolerances %s against one pass at %g, min_points %d; host functions"
             % (gm.W, gm.H, "/".join("%g" % t for t in gm.TOLERANCES), gm.TOLERANCES[0], gm.MIN_POINTS),
             "# angle = between the fitted and the true floor normal (rad); height = |camera height error| (m)"]
    worst_a = worst_h = 0.0
    for name, cfg, frame, truth, prior in gm.accuracy_cases(ssd):
        three = gm.refine_host(ssd, cfg, frame, prior)
        one = gm.refine_host(ssd, cfg, frame, prior, tolerances=gm.TOLERANCES[:1])
        a3, h3 = gm.errors(three, truth)
        a1, h1 = gm.errors(one, truth)
        lines.append("# %s: three passes angle %.3e height %.3e (status %d, %d points, rms %.2e) | one pass angle %.3e height %.3e (%d points)"
                     % (name, a3, h3, three.status, three.m.n, three.rms, a1, h1, one.m.n))
        worst_a, worst_h = max(worst_a, a3), max(worst_h, h3)
    lines.append("worst_angle_rad = %.3e" % worst_a)
    lines.append("worst_height_m = %.3e" % worst_h)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
