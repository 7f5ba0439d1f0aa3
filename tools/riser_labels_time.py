#!/usr/bin/env python3
"""tools/riser_labels_time.py [ROUNDS] [OUT] - what the riser labels (k_riser_labels) cost on one resident XGA
batch of 256 frames (scenes.batch_scenes, one workspace), vertices and 16-bit depth, timing on, after bench.py's half-second warm-up,
legs alternating within a round, median (min .. max) of ROUNDS (15).

Three handles over the same frames, one enqueue with labels + fetch each per round, in turn:
  plain    labels, risers off                    - its `final` stage is k_final alone
  risers   labels + risers                       - the parent commit's code path; `final` = k_final + the riser pass
  marked   labels + risers + riser labels        - this build's
Reported per input: k_riser_labels' device time (ssd_get_riser_labels_time_back), the label pass of the same run
(ssd_get_labels_time_back on `risers` and on `marked`: the code object is the parent's), the riser pass (the `final` stage of `risers`
less that of `plain`), frames/s by wall time of `risers` against `marked`, and the ratios.  The masks of `marked` must split into the
masks of `risers` and counts that equal its riser records'.

Writes profiles/riser_labels_time.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/scenes.py)."""
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import scenes  # noqa: E402

W, H, F = 1024, 768, 256
TOL, SUPPORT = 0.03, 200
LEGS = ("plain", "risers", "marked")


def spread(v):
    return "%.4f (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def part(rounds, depth, lines):
    scs = scenes.batch_scenes(ssd, W, H, F)
    trans = ssd.transformation_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=F, batches_in_flight=1)
    wh = W * H
    dets = {}
    bufs = [ssd.DeviceBuffer(F * wh * (2 if depth else 12), 0), ssd.DeviceBuffer(F * wh, 0)]
    buf, lab = bufs
    try:
        for name in LEGS:
            det = dets[name] = ssd.Detector(cfg, trans, 0)
            if depth:
                det.set_intrinsics(ssd.intrinsics_for_scene(scs[0]))
            det.set_timing(True)
            if name != "plain":
                det.set_risers(True, tolerance=TOL, min_support=SUPPORT)
            if name == "marked":
                det.set_riser_labels(True)
        if depth:
            ssd.synth_depth_device(scs, buf.ptr, device=0)
        else:
            ssd.synth_device(scs, buf.ptr, device=0)
        ssd.lib().ssd_device_sync(0)

        def leg(name):
            det = dets[name]
            c0 = time.perf_counter()
            (det.enqueue_depth_labels if depth else det.enqueue_labels)(buf.ptr, F, lab.ptr)
            det.fetch(F)
            wall = time.perf_counter() - c0
            return dict(wall=wall, labels=det.labels_time_ms(), mark=det.riser_labels_time_ms(), final=det.stage_times_ms()["final"])

        def one_round():
            return {name: leg(name) for name in LEGS}

        # what the legs write, once: the marked masks split into the parent's masks and the riser records' counts
        leg("risers")
        base = lab.download(F * wh).copy()
        leg("marked")
        surfaces, risers = ssd.labels_split(lab.download(F * wh))
        assert np.array_equal(surfaces, base), "the surface labels moved"
        ris = dets["marked"].fetch_risers(F)
        counts = [np.bincount(risers[i * wh:(i + 1) * wh], minlength=ssd.MAX_RISERS + 1)[1:] for i in range(F)]
        assert all(int(counts[i][k]) == (ris[i].risers[k].n_points if k < ris[i].n_risers else 0) for i in range(F) for k in range(ssd.MAX_RISERS))
        marked_points = int(sum(int(c.sum()) for c in counts))

        c0 = time.perf_counter()
        while time.perf_counter() - c0 < 0.5:                                  # bench.py's warm-up: load until the device has been busy a while
            one_round()
        took = [one_round() for _ in range(rounds)]
        col = lambda name, key: [t[name][key] for t in took]
        mark, labels_r, labels_m = col("marked", "mark"), col("risers", "labels"), col("marked", "labels")
        riser_pass = [t["risers"]["final"] - t["plain"]["final"] for t in took]
        fps_r, fps_m = [F / t["risers"]["wall"] for t in took], [F / t["marked"]["wall"] for t in took]
        assert all(v == 0.0 for v in col("risers", "mark") + col("plain", "mark")), "a leg without riser labels marked something"
        kind = "16-bit depth" if depth else "vertices"
        lines.append("%-12s evidence points marked per batch            %d (%.0f per frame)" % (kind, marked_points, marked_points / F))
        lines.append("%-12s k_riser_labels (ssd_get_riser_labels_time_back)  %s ms" % (kind, spread(mark)))
        lines.append("%-12s k_labels, labels + risers                     %s ms" % (kind, spread(labels_r)))
        lines.append("%-12s k_labels, labels + risers + riser labels      %s ms" % (kind, spread(labels_m)))
        lines.append("%-12s riser pass (final with risers - final without) %s ms" % (kind, spread(riser_pass)))
        lines.append("%-12s frames/s, labels + risers                     %s" % (kind, spread([v / 1e3 for v in fps_r]) + " k"))
        lines.append("%-12s frames/s, labels + risers + riser labels      %s" % (kind, spread([v / 1e3 for v in fps_m]) + " k"))
        lines.append("%-12s k_riser_labels / k_labels = %.3f   k_riser_labels / riser pass = %.3f   frames/s marked / risers = %.4f"
                     % (kind, statistics.median(mark) / statistics.median(labels_r), statistics.median(mark) / statistics.median(riser_pass),
                        statistics.median(fps_m) / statistics.median(fps_r)))
    finally:
        for x in bufs:
            x.free()
        for det in dets.values():
            det.close()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "riser_labels_time.txt")
    lines = ["# tools/riser_labels_time.py %d: one resident XGA batch of %d frames, timing on, half a second of warm-up per input, the three legs" % (rounds, F),
             "# (labels; labels + risers; labels + risers + riser labels) alternating within a round, %d rounds; median (min .. max)" % rounds, ""]
    for depth in (False, True):
        part(rounds, depth, lines)
        lines.append("")
    text = "\n".join(lines)
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
