#!/usr/bin/env python3
"""tools/riser_fit_accuracy.py [OUT] - how well the riser fit recovers the faces of a staircase, measured on the host functions (oracle
-> tests/riser_model.riser_labels -> ssd_surface_moments_host -> ssd_riser_fit_solve; the device is held to the host sums bit for bit,
so no GPU is needed): the cases of tests/riser_model.py (the 3-step scene of tests/ground_model.py at 256 x 192, sigma 1 mm and 3 mm,
under the true calibration).  The scene's risers are vertical, parallel to the edges and one tread apart, so lean and skew should be 0
and going the scene's tread.  Writes profiles/riser_fit_accuracy.txt (or OUT); tests/test_riser_fit.py asserts three times each
figure recorded there.  TEST INFRASTRUCTURE (uses tests/riser_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import oracle_binding  # noqa: E402
import riser_model as rm  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else rm.ACCURACY_FILE
    oracle = oracle_binding.load_oracle()
    lines = ["# tools/riser_fit_accuracy.py: %d x %d, 3 steps, pose %s, tolerance %g m, min_points %d; host functions on the oracle's record"
             % (rm.W, rm.H, rm.gm.POSE, rm.TOL, rm.MIN_POINTS),
             "# per riser: lean (rad), skew (rad), rms (m), rise (m), going (m; 0: the next riser is not OK or there is none), points"]
    worst = [0.0, 0.0, 0.0]
    for name, cfg, frame, cal, sc in rm.accuracy_cases(ssd):
        status, lean, skew, going, pairs, rows = rm.accuracy_of(ssd, oracle, cfg, frame, cal, sc)
        lines.append("# %s: %d risers, %d OK, scene tread %.3f m, rise %.3f m" % (name, len(rows), sum(1 for s in status if s == ssd.GF_OK), sc.tread, sc.rise))
        for i, st, n, ln, sk, rms, rise, go in rows:
            lines.append("#   riser %d: status %d, lean %+.3e, skew %.3e, rms %.2e, rise %.4f, going %.4f, %d points" % (i, st, ln, sk, rms, rise, go, n))
        worst = [max(worst[0], lean), max(worst[1], skew), max(worst[2], going)]
    lines.append("worst_lean_rad = %.3e" % worst[0])
    lines.append("worst_skew_rad = %.3e" % worst[1])
    lines.append("worst_going_error_m = %.3e" % worst[2])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
