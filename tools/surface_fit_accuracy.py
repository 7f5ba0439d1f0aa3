#!/usr/bin/env python3
"""tools/surface_fit_accuracy.py [OUT] - how well the surface fit recovers the tilt of the reported surfaces, measured on the host
functions (oracle -> tests/test_labels.expected_labels -> ssd_surface_moments_host -> ssd_surface_fit_solve; the device is held to
the host sums bit for bit, so no GPU is needed): the cases of tests/surface_model.py (3-step scene at 256 x 192, sigma 1 mm and 3 mm,
the true calibration and calibrations pitched or rolled by a few tenths of a degree).  Every surface of the scene is level, so its
tilt under the calibration in use should be the angle between the true calibration's up vector and that calibration's.  Writes
profiles/surface_fit_accuracy.txt (or OUT); tests/test_surface_fit.py asserts three times the worst figure recorded there.
TEST INFRASTRUCTURE (uses tests/surface_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import oracle_binding  # noqa: E402
import surface_model as sm  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else sm.ACCURACY_FILE
    oracle = oracle_binding.load_oracle()
    lines = ["# tools/surface_fit_accuracy.py: %d x %d, 3 steps, min_points %d; host functions on the oracle's labels" % (sm.W, sm.H, sm.MIN_POINTS),
             "# per surface (0 = the ground): tilt (rad), |tilt - angle between the true and the used calibration's up vectors| (rad), rms (m), points"]
    worst = 0.0
    for name, cfg, frame, truth, cal in sm.accuracy_cases(ssd):
        want, res, rows = sm.tilt_errors(ssd, oracle, cfg, frame, truth, cal)
        lines.append("# %s: %d surfaces, angle between the up vectors %.3e" % (name, len(rows), want))
        for k, status, n, tilt, err, rms in rows:
            lines.append("#   surface %d: status %d, tilt %.3e, error %.3e, rms %.2e, %d points" % (k, status, tilt, err, rms, n))
            if status == ssd.GF_OK:
                worst = max(worst, err)
    lines.append("worst_tilt_error_rad = %.3e" % worst)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
