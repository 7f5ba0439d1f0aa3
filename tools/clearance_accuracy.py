#!/usr/bin/env python3
"""tools/clearance_accuracy.py [OUT] - what the tread clearance rule finds on the 3-step scene, measured on the host functions (oracle ->
ssd_clearance_host -> ssd_clearance_solve; the device is held to the host sums byte for byte, so no GPU is needed): tests/clearance_model.py's
recipe at 256 x 192, sigma 1 mm and 3 mm, five seeds, the default rule.  Per case: the occupants of the clean frame (every one of them
false), the share of a 300-point patch pulled 10 % towards the camera that is found on its tread (tread 1, the top tread), its mean height
and the solved centroid's distance from the mean of the patch's own points.  Writes profiles/clearance_accuracy.txt (or OUT);
tests/test_clearance.py asserts the zero and the recorded shares less 0.03.
TEST INFRASTRUCTURE (uses tests/clearance_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import clearance_model as cm  # noqa: E402
import oracle_binding  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else cm.ACCURACY_FILE
    oracle = oracle_binding.load_oracle()
    rows = []
    worst = cm.accuracy(ssd, oracle, rows=rows)
    lines = ["# tools/clearance_accuracy.py: %d x %d, 3 steps, rule margin %g lo %g hi %g, min_support 50; host functions on the oracle's record" % ((cm.W, cm.H) + cm.RULE),
             "# per case: occupants of the clean frame | per patch: found on its tread of pulled (share), height_mean, |solved centroid - mean of the patch's points|"]
    lines += ["# " + r for r in rows]
    lines.append("false_occupants_clean = %d" % worst["false_occupants_clean"])
    lines.append("worst_share_tread1 = %.4f" % worst["worst_share_tread1"])
    lines.append("worst_share_top = %.4f" % worst["worst_share_top"])
    lines.append("worst_centroid_distance_m = %.5f" % worst["worst_centroid_distance_m"])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
