#!/usr/bin/env python3
"""tools/tread_grid_accuracy.py [OUT] - the tread grid's recipe under the oracle, through the numpy model of
tests/tread_grid_model.py alone (the host functions are held to the model cell by cell, the device to the host byte for byte, so no GPU
is needed): the 3-step scene at 256 x 192, sigma 1 mm, clearance rule 0.03 / 0.03 / 0.5, the model's cell size and supports; the clean
frame and the frame with a 300-point patch pulled 10 % towards the camera off tread 1, each under its own oracle result.  Per tread: the
cells FREE / OCCUPIED / UNSEEN, the best free rectangle and the tallest occupant; and the conditions tests/test_tread_grid.py asserts.
Writes profiles/tread_grid_accuracy.txt (or OUT).  TEST INFRASTRUCTURE (uses tests/tread_grid_model.py and the CPU oracle)."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ssd = importlib.import_module("stair-step-detector_amd")
import clearance_model as cm  # noqa: E402
import oracle_binding  # noqa: E402
import tread_grid_model as tg  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else tg.ACCURACY_FILE
    r = tg.recipe(ssd, oracle_binding.load_oracle())
    lines = ["# tools/tread_grid_accuracy.py: %d x %d, 3 steps, sigma 1 mm, seed 7, rule margin %g lo %g hi %g; the numpy model on the oracle's records"
             % ((cm.W, cm.H) + cm.RULE),
             "# per tread: cells free / occupied / unseen, best free rectangle (col0, row0, cols x rows), tallest occupant, points outside the grid"]
    for key in ("clean", "patched"):
        for k, s in enumerate(r[key]):
            g = r["grids_" + key][k]
            lines.append("# %-7s tread %d: free %3d occupied %2d unseen %2d | rectangle (%d, %d, %d x %d) | tallest %.4f m | outside: %d tread points, %d occupants"
                         % ((key, k, s["n_free"], s["n_occupied"], s["n_unseen"]) + tuple(s["rect"]) + (s["tallest"], g["n_seen_out"], g["n_occ_out"])))
    st, vac = r["patched"][1]["state"], r["vacated_cells"]
    lines.append("# patched tread 1, the states (0 out, 1 free, 2 occupied, 3 unseen), row 0 = the front edge:")
    lines += ["#   " + "".join(str(int(v)) for v in row) for row in st]
    lines.append("cell_m = %g" % tg.RECIPE_CELL)
    lines.append("min_seen = %d" % tg.RECIPE_MIN_SEEN)
    lines.append("min_occ = %d" % tg.RECIPE_MIN_OCC)
    lines.append("occupied_cells_clean = %d" % sum(s["n_occupied"] for s in r["clean"]))
    lines.append("occupied_cells_patched_tread = %d" % r["patched"][1]["n_occupied"])
    lines.append("unseen_cells_patched_tread = %d" % r["patched"][1]["n_unseen"])
    lines.append("cells_with_a_pulled_point = %d" % np.count_nonzero(r["pulled_cells"]))
    lines.append("vacated_cells = %d" % np.count_nonzero(vac))
    lines.append("vacated_cells_free = %d" % np.count_nonzero(vac & (st == tg.FREE)))
    lines.append("other_treads_unchanged = %d" % int(all(np.array_equal(r["patched"][k]["state"], r["clean"][k]["state"]) for k in (0, 2))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out_path, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
