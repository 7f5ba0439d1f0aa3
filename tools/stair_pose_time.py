#!/usr/bin/env python3
"""tools/stair_pose_time.py [ROUNDS] [OUT] - what the stair pose pass (k_stair_pose) costs beside its yardstick,
the ground fit's pass (k_ground_moments): a pure stream over the same bytes, on the same batch in the same run.  XGA x 256 frames
resident in device memory (scenes.batch_scenes, the bench's), as vertices and as 16-bit depth.
A round is three legs, so the legs alternate, after bench.py's half-second warm-up: the stair pose against ONE target that all 256 frames
name (the staircase the detector reports for frame 0), the stair pose against 16 targets dealt round-robin (the staircases of frames
0 .. 15), and the ground fit.  Each leg is timed with a host clock around the enqueue and the fetch that waits for it (a leg ends with
the copy of its records to the host: 3008 bytes per frame for the stair pose, 80 for the ground fit); the stair pose's own device events
(ssd_get_stair_pose_time) stand beside it.  The first and the last frame's records are checked against ssd_stair_pose_host.
Nothing is fixed in advance: the figures are what they are.
Writes profiles/stair_pose_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
import ctypes as C
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import scenes  # noqa: E402

W, H, F, TARGETS, TOL = 1024, 768, 256, 16, 0.03


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "stair_pose_time.txt")
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    intr = ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    rule = ssd.StairPoseRule()
    lines = ["# tools/stair_pose_time.py %d: XGA x %d resident frames, %d timed rounds; a round = the stair pose with 1 target for all frames, the"
             % (rounds, F, rounds),
             "# stair pose with %d targets dealt round-robin, the ground fit (tol %g) - rule %g / %g / %g / %g."
             % (TARGETS, TOL, rule.margin, rule.band, rule.clear, rule.reach),
             "# ms per pass over %d frames, host clock around enqueue and fetch, median (min .. max); [..]: the stair pose's own device events" % F]
    bad = 0
    for depth in (False, True):
        det = ssd.Detector(cfg, trans, 0)
        nbytes = F * W * H * (2 if depth else 12)
        buf = ssd.DeviceBuffer(nbytes, 0)
        try:
            if depth:
                det.set_intrinsics(intr)
                ssd.synth_depth_device(scs, buf.ptr, device=0)
            else:
                ssd.synth_device(scs, buf.ptr, device=0)
            ssd.lib().ssd_device_sync(0)
            det.set_timing(True)
            (det.enqueue_depth if depth else det.enqueue)(buf.ptr, F)
            res = det.fetch_list(F)
            targets = [ssd.stair_pose_target((trans, intr) if depth else trans, r) for r in res[:TARGETS]]
            dealt = [i % TARGETS for i in range(F)]

            def leg(fn, fetch):
                t0 = time.perf_counter()
                fn()
                fetch()
                return (time.perf_counter() - t0) * 1e3

            def one_round():
                a = leg(lambda: det.enqueue_stair_pose(buf.ptr, F, targets[:1], None, rule, depth=depth), lambda: det.fetch_stair_pose_moments(1))
                ea = det.stair_pose_time_ms()
                b = leg(lambda: det.enqueue_stair_pose(buf.ptr, F, targets, dealt, rule, depth=depth), lambda: det.fetch_stair_pose_moments(1))
                eb = det.stair_pose_time_ms()
                c = leg(lambda: det.enqueue_ground_fit(buf.ptr, F, TOL, depth=depth), lambda: det.fetch_ground_fit(1, min_points=1))
                return a, b, c, ea, eb

            c0 = time.perf_counter()
            while time.perf_counter() - c0 < 0.5:                          # bench.py's warm-up: load until the device has been busy a while
                one_round()
            took = [one_round() for _ in range(rounds)]
            tag = "depth16" if depth else "vertices"
            det.enqueue_stair_pose(buf.ptr, F, targets, dealt, rule, depth=depth)
            got = det.fetch_stair_pose_moments(F)
            classified = sum(int(m.treads.s[k].m.n + m.treads.s[k].n_far + m.risers.s[k].m.n + m.risers.s[k].n_far) for m in got for k in range(ssd.MAX_STEPS))
            for i in (0, F - 1):
                host = (ssd.synth_depth_host if depth else ssd.synth_host)([scs[i]])[0]
                same = bytes(got[i]) == bytes(ssd.stair_pose_host(cfg, targets[dealt[i]], host, rule, depth=depth))
                bad += 0 if same else 1
                lines.append("%-8s frame %d against target %d: equal to ssd_stair_pose_host: %s" % (tag, i, dealt[i], same))
            med = []
            for name, col, ev in (("k_stair_pose, 1 target", 0, 3), ("k_stair_pose, %d targets" % TARGETS, 1, 4), ("k_ground_moments", 2, None)):
                t = [x[col] for x in took]
                med.append(statistics.median(t))
                events = "" if ev is None else "   [%.3f (%.3f .. %.3f)]" % (statistics.median([x[ev] for x in took]), min(x[ev] for x in took),
                                                                             max(x[ev] for x in took))
                lines.append("%-8s %-26s %.3f (%.3f .. %.3f) = %.0f GB/s%s" % (tag, name, med[-1], min(t), max(t), nbytes / med[-1] / 1e6, events))
            lines.append("%-8s ratios of the medians: 1 target / k_ground_moments %.3f, %d targets / k_ground_moments %.3f; %d of %d points classified"
                         % (tag, med[0] / med[2], TARGETS, med[1] / med[2], classified, F * W * H))
        finally:
            buf.free()
            det.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
