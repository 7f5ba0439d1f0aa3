#!/usr/bin/env python3
"""tools/depth_edges_accuracy.py [OUT] - what the depth edge filter (ssd_depth_edges_host) achieves, measured on the
host statement and the oracle alone (the device is held to the host statement byte for byte, so no GPU is needed).
(a) The default slope: the smallest of 0, 16, 32, 64, 128, 256 at which the noise-free depth frames of the scenes in tests/sweep_scenes.py
lose at most 0.1 % of the pixels that the oracle's labels assign to a reported surface; the loss at every candidate.
(b) 256 x 192, the 3-step scene, the default rule: the share of the mixed-pixel model's truth subset and of all its planted pixels that
goes, of the clean frame's pixels, of the stress configuration's outliers and inliers, and the occupants per surface from
ssd_clearance_host before -> after, on the scene with planted pixels and on the scene with a box on every surface.
Writes profiles/depth_edges_accuracy.txt (or OUT); tests/test_depth_edges.py computes the file again and asserts its directions.
TEST INFRASTRUCTURE (uses tests/edges_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import edges_model as em  # noqa: E402
import oracle_binding  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "depth_edges_accuracy.txt")
    text = "\n".join(em.accuracy_lines(ssd, oracle_binding.load_oracle())) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
