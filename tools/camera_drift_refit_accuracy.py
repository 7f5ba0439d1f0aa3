#!/usr/bin/env python3
"""tools/camera_drift_refit_accuracy.py [OUT] - what folding REFIT records does to the drift per camera, measured
on the host functions alone (oracle under the table entry -> tests/test_labels.expected_labels -> ssd_surface_moments_host ->
ssd_surface_gates_from_moments [-> ssd_camera_ground_gates] -> ssd_surface_refit_moments_host -> ssd_camera_drift_fold; the device is
held to the host sums bit for bit, so no GPU is needed): the entries and frames of tests/camera_drift_model.py, as
tools/camera_drift_accuracy.py takes them.  Columns: the fold of the first-pass records (the yardstick of the same run: it reproduces
profiles/camera_drift_accuracy.txt), the fold of one and of two refit passes at k_sigma 2.5 and 2.0 with per-frame gates, and the same
with the camera's folded floor plane as every frame's ground gate in front of the last pass.  The errors are taken against the scene
generator's true pose.  Writes profiles/camera_drift_refit_accuracy.txt (or OUT); tests/test_camera_surfaces_refit.py asserts against
the figures recorded there.
TEST INFRASTRUCTURE (uses tests/camera_refit_model.py, tests/camera_drift_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import camera_drift_model as cdm  # noqa: E402
import camera_refit_model as crm  # noqa: E402
import oracle_binding  # noqa: E402
import surface_model as sm  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else crm.ACCURACY_FILE
    oracle = oracle_binding.load_oracle()
    rows = crm.accuracy_rows(ssd, oracle)
    lines = ["# tools/camera_drift_refit_accuracy.py: %d x %d, 3 steps, %d frames per camera (seed, sigma: %s); gates: min_points %d, gate_min 0;"
             % (cdm.W, cdm.H, len(cdm.FRAMES), ", ".join("%d %g mm" % (s, g * 1e3) for s, g in cdm.FRAMES), sm.MIN_POINTS),
             "# fold: min_points %d; host functions on the oracle's labels" % cdm.MIN_POINTS,
             "# per table entry and column: the folded fit's errors against the true pose - tilt (rad) / height_delta (m) / normal (rad) -,",
             "# the ground points folded, their share of the first-pass fold's, and the least share of a FRAME's first-pass ground points kept",
             "# columns: first = the first-pass records; kK_passP = P refit passes at k_sigma K, per-frame gates; .._camera = the same with",
             "# ssd_camera_ground_gates (the fold of the records so far) in front of the last pass"]
    for name, row in rows:
        lines.append("# entry %s:" % name)
        for c in crm.COLUMNS:
            et, eh, ea, status, n, fold_share, share = row[c]
            lines.append("#   %-20s tilt %.3e, height %.3e, normal %.3e; %d points, kept share %.4f, least of a frame %.4f%s"
                         % (crm.column_key(c), et, eh, ea, n, fold_share, share, "" if status == ssd.GF_OK else "   status %d" % status))
    worst = crm.worst_columns(rows)
    for c in crm.COLUMNS:
        lines.append("worst_tilt_error_rad_%s = %.3e" % (crm.column_key(c), worst[c][0]))
    for c in crm.COLUMNS:
        lines.append("worst_height_error_m_%s = %.3e" % (crm.column_key(c), worst[c][1]))
    for c in crm.COLUMNS[1:]:
        lines.append("least_fold_kept_share_%s = %.4f" % (crm.column_key(c), worst[c][2]))
    for c in crm.COLUMNS[1:]:
        lines.append("least_frame_kept_share_%s = %.4f" % (crm.column_key(c), worst[c][3]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
