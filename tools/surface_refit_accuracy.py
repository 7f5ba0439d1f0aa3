#!/usr/bin/env python3
"""tools/surface_refit_accuracy.py [OUT] - what the trimmed surface refit does to the tilt error of the surface
fit, measured on the new host functions alone (oracle -> tests/test_labels.expected_labels -> ssd_surface_moments_host ->
ssd_surface_gates_from_moments -> ssd_surface_refit_moments_host -> ssd_surface_fit_solve; the device is held to the host sums bit
for bit, so no GPU is needed): the cases of tests/surface_model.accuracy_cases, per surface the tilt error and rms of the first fit
and of refit passes 1 and 2 at k_sigma 2.5 and 2.0 with gate_min 0, the points kept, and the worst of each column.  The yardstick is
the first fit of the same run; its column reproduces profiles/surface_fit_accuracy.txt.  Writes profiles/surface_refit_accuracy.txt
(or OUT); tests/test_surface_refit.py asserts against the figures recorded there.
TEST INFRASTRUCTURE (uses tests/refit_model.py, tests/surface_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import oracle_binding  # noqa: E402
import refit_model as rm  # noqa: E402
import surface_model as sm  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else rm.ACCURACY_FILE
    oracle = oracle_binding.load_oracle()
    cases = rm.accuracy_rows(ssd, oracle)
    cols = [(ks, p + 1) for ks in rm.K_SIGMAS for p in range(rm.PASSES)]
    lines = ["# tools/surface_refit_accuracy.py: %d x %d, 3 steps, min_points %d, gate_min 0; host functions on the oracle's labels" % (sm.W, sm.H, sm.MIN_POINTS),
             "# per surface (0 = the ground): |tilt - angle between the true and the used calibration's up vectors| (rad) / rms (m) / points,",
             "# of the first fit, then of refit pass 1 and 2 at k_sigma 2.5, then at k_sigma 2.0 (points = kept: m.n + n_far)"]
    for name, want, rows in cases:
        lines.append("# %s: %d surfaces, angle between the up vectors %.3e" % (name, len(rows), want))
        for k, r in enumerate(rows):
            cells = ["%.3e / %.2e / %d" % r["first"][:3]] + ["%.3e / %.2e / %d" % r[c][:3] for c in cols]
            bad = [rm.column_key(c) for c in ["first"] + cols if r[c][3] != ssd.GF_OK]
            lines.append("#   surface %d: %s%s" % (k, " | ".join(cells), "   status not OK: " + ", ".join(bad) if bad else ""))
    worst, share = rm.worst_columns(cases)
    for c in ["first"] + cols:
        lines.append("worst_tilt_error_rad_%s = %.3e" % (rm.column_key(c), worst[c]))
    for c in cols:
        lines.append("least_kept_share_%s = %.4f" % (rm.column_key(c), share[c]))
    for sigma in sm.SIGMAS:
        tag = "sigma %g mm" % (sigma * 1e3)
        mine = [(n, w, rows) for n, w, rows in cases if n.startswith(tag)]
        w, _ = rm.worst_columns(mine)
        lines.append("# %s alone: worst tilt error %s" % (tag, ", ".join("%s %.3e" % (rm.column_key(c), w[c]) for c in ["first"] + cols)))
        lines.append("# %s alone: the ground's rms, true calibration: %s" % (tag, ", ".join("%s %.2e" % (rm.column_key(c), mine[0][2][0][c][1]) for c in ["first"] + cols)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
