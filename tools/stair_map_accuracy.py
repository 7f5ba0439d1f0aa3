#!/usr/bin/env python3
"""tools/stair_map_accuracy.py [OUT] - what folding frames into a stair map does to the tread grid's answer,
through the host functions (ssd_tread_grid_host, ssd_tread_grid_add, ssd_stair_map_from_results, ssd_tread_grid_solve) and the CPU oracle
alone - the device is held to the host functions byte for byte, so no GPU is needed.
The 3-step scene at 256 x 192 under the clearance rule 0.03 / 0.03 / 0.5 and the tread grid recipe's cell.  Cases: 1, 2, 4 and 8 frames
of one camera (seeds 7, 8, .. with the noises of tests/camera_drift_model.py in turn) against the median map of their own oracle
results, and the three cameras of tests/test_gpu_stair_map.py together, one frame each.  Frame 0 of every set carries
clearance_model.patched's 300-point box on tread 1.  Per case and tread: the cells FREE / OCCUPIED / UNSEEN and the foothold of the
folded record under min_seen = min_occ = 3, and with both supports scaled by the number of frames folded; beside them frame 0's own
tread grid (its own oracle result, supports 3), which is what a caller had before.
Writes profiles/stair_map_accuracy.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/ and the CPU oracle)."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import camera_drift_model as cd  # noqa: E402
import clearance_model as cm  # noqa: E402
import ground_model as gm  # noqa: E402
import oracle_binding as ob  # noqa: E402
import tread_grid_model as tg  # noqa: E402
from test_labels import expected_labels  # noqa: E402

SUPPORT = tg.RECIPE_MIN_SEEN
POSES = [dict(), dict(pitch_deg=52.0), dict(cam_height=1.05, roll_deg=1.0)]
ACCURACY_FILE = os.path.join(ROOT, "profiles", "stair_map_accuracy.txt")


def detect(oracle, cfg, cal, frame):
    res = oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(cal), frame)[0]
    return res, cm.result_of_oracle(ssd, res)


def boxed(oracle, cfg, cal, frame):
    """the frame with the box on tread 1, and its own result"""
    res, fr = detect(oracle, cfg, cal, frame)
    f2 = cm.patched(cfg, cal, fr, frame, expected_labels(oracle, cfg, cal, res, frame), 1)[0]
    return f2, detect(oracle, cfg, cal, f2)[1]


def row(tag, f, k):
    s = f.s[k]
    return ("%-34s tread %d: free %3d occupied %2d unseen %2d | foothold %d (%d, %d, %d x %d) | tallest %.4f m"
            % (tag, k, s.n_free, s.n_occupied, s.n_unseen, s.foothold, s.col0, s.row0, s.cols, s.rows, s.tallest))


def case(lines, name, cfg, frames, cals, own, rule):
    """frames[i] under cals[i] with its own result own[i]; frame 0 carries the box"""
    n = len(frames)
    m, used = ssd.stair_map_from_results(own)
    folded = ssd.FrameTreadGrid()
    for f, cal in zip(frames, cals):
        ssd.tread_grid_add(ssd.tread_grid_host(cfg, cal, f, m.stairs, m.ground, rule), folded)
    before = ssd.tread_grid_solve(ssd.tread_grid_host(cfg, cals[0], frames[0], own[0], 1, rule), own[0], rule, SUPPORT, SUPPORT)
    plain = ssd.tread_grid_solve(folded, m.stairs, rule, SUPPORT, SUPPORT)
    scaled = ssd.tread_grid_solve(folded, m.stairs, rule, SUPPORT * n, SUPPORT * n)
    lines.append("# %s: %d frames, %d used for the median map (%d steps)" % (name, n, used, m.stairs.n_steps))
    for k in range(m.stairs.n_steps):
        lines.append("#   " + row("frame 0 alone, own result, %d / %d" % (SUPPORT, SUPPORT), before, k))
        lines.append("#   " + row("folded, supports %d / %d" % (SUPPORT, SUPPORT), plain, k))
        lines.append("#   " + row("folded, supports %d / %d" % (SUPPORT * n, SUPPORT * n), scaled, k))
    return before, plain, scaled


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else ACCURACY_FILE
    oracle = ob.load_oracle()
    cfg = ssd.default_config(cd.W, cd.H)
    rule = tg.rule_of(ssd, cm.RULE + (tg.RECIPE_CELL,))
    lines = ["# tools/stair_map_accuracy.py: %d x %d, 3 steps, rule margin %g lo %g hi %g, cell %g; the host functions on the oracle's records"
             % ((cd.W, cd.H) + cm.RULE + (tg.RECIPE_CELL,)),
             "# per case and tread: cells free / occupied / unseen, the foothold (col0, row0, cols x rows) and the tallest occupant of frame 0's own",
             "# tread grid, of the record folded over the case's frames against their median map, and of the same with the supports scaled"]
    summary = []
    for n in (1, 2, 4, 8):
        frames, own, cal = [], [], None
        for i in range(n):
            seed, sigma = 7 + i, cd.FRAMES[i % len(cd.FRAMES)][1]
            sc = gm.scene(ssd, "steps", seed=seed, sigma=sigma)
            cal = cal or ssd.transformation_for_scene(sc).constants
            frame = ssd.synth_host([sc])[0]
            if i == 0:
                frame, fr = boxed(oracle, cfg, cal, frame)
            else:
                fr = detect(oracle, cfg, cal, frame)[1]
            frames.append(frame)
            own.append(fr)
        before, plain, scaled = case(lines, "one camera", cfg, frames, [cal] * n, own, rule)
        summary.append(("one_camera_%d" % n, before, plain, scaled))
    frames, own, cals = [], [], []
    for c, kw in enumerate(POSES):
        sc = gm.scene(ssd, "steps", seed=7 + c, **kw)
        cal = ssd.transformation_for_scene(sc).constants
        frame = ssd.synth_host([sc])[0]
        if c == 0:
            frame, fr = boxed(oracle, cfg, cal, frame)
        else:
            fr = detect(oracle, cfg, cal, frame)[1]
        frames.append(frame)
        own.append(fr)
        cals.append(cal)
    summary.append(("three_cameras",) + case(lines, "three cameras", cfg, frames, cals, own, rule))
    lines.append("cell_m = %g" % tg.RECIPE_CELL)
    lines.append("support = %d" % SUPPORT)
    for name, before, plain, scaled in summary:
        lines.append("%s_unseen_tread_1 = %d alone, %d folded, %d folded with scaled supports"
                     % (name, before.s[1].n_unseen, plain.s[1].n_unseen, scaled.s[1].n_unseen))
        lines.append("%s_occupied_tread_1 = %d alone, %d folded, %d folded with scaled supports"
                     % (name, before.s[1].n_occupied, plain.s[1].n_occupied, scaled.s[1].n_occupied))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
