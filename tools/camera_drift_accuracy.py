#!/usr/bin/env python3
"""tools/camera_drift_accuracy.py [OUT] - how well the drift per camera (ssd_camera_drift_fold) recovers how far
a camera's mounting is from its table entry, measured on the host functions (oracle under the table entry ->
tests/test_labels.expected_labels -> ssd_surface_moments_host -> ssd_camera_drift_fold; the device is held to the host sums bit for
bit, so no GPU is needed): the entries of tests/camera_drift_model.py, four frames of the 3-step 256 x 192 scene each.  The errors are
taken against the scene generator's true pose.  Writes profiles/camera_drift_accuracy.txt (or OUT); tests/test_camera_surfaces.py
asserts three times the worst figures recorded there.
TEST INFRASTRUCTURE (uses tests/camera_drift_model.py and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import camera_drift_model as cdm  # noqa: E402
import oracle_binding  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else cdm.ACCURACY_FILE
    oracle = oracle_binding.load_oracle()
    lines = ["# tools/camera_drift_accuracy.py: %d x %d, 3 steps, %d frames per camera (seed, sigma: %s), min_points %d; host functions on the oracle's labels"
             % (cdm.W, cdm.H, len(cdm.FRAMES), ", ".join("%d %g mm" % (s, g * 1e3) for s, g in cdm.FRAMES), cdm.MIN_POINTS),
             "# per table entry: the folded fit's tilt (rad) and height_delta (m), their errors against the true pose, the fitted normal's angle to the true one,",
             "# and the worst single-frame figures of the same camera"]
    worst_tilt = worst_height = 0.0
    for name, offset in cdm.ENTRIES:
        truth, entry, moments = cdm.camera_case(ssd, oracle, offset)
        cams = [entry]
        d = ssd.camera_drift_fold(moments, [0] * len(moments), cams, min_points=cdm.MIN_POINTS)[0]
        single = [ssd.camera_drift_fold([m], [0], cams, min_points=cdm.MIN_POINTS)[0] for m in moments]
        et, eh, ea = cdm.drift_errors(d.fit, truth, entry)
        lines.append("# entry %s: %d of %d frames folded, %d ground points, status %d" % (name, d.frames_ground, d.frames, d.m.n, d.fit.status))
        lines.append("#   folded: tilt %.4e, height_delta %+.4e, rms %.2e; errors: tilt %.3e, height %.3e, normal %.3e"
                     % (d.fit.tilt, d.fit.height_delta, d.fit.rms, et, eh, ea))
        for (seed, sigma), s in zip(cdm.FRAMES, single):
            st, sh, sa = cdm.drift_errors(s.fit, truth, entry)
            lines.append("#   frame seed %d sigma %g mm: status %d, %d points; errors: tilt %.3e, height %.3e, normal %.3e"
                         % (seed, sigma * 1e3, s.fit.status, s.m.n, st, sh, sa))
        if d.fit.status == ssd.GF_OK:
            worst_tilt, worst_height = max(worst_tilt, et), max(worst_height, eh)
    lines.append("worst_tilt_error_rad = %.3e" % worst_tilt)
    lines.append("worst_height_error_m = %.3e" % worst_height)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
