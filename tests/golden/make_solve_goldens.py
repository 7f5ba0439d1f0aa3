#!/usr/bin/env python3
"""tests/golden/make_solve_goldens.py - writes tests/golden/solve_goldens.json: what the HOST solve (jacobi3 / plane_of_moments, behind
ssd_surface_gates_from_moments, ssd_surface_fit_solve and ssd_ground_fit_solve) returns for a set of integer moment records, every
double in hex.

What this pins: the host solve against itself across the move of its text from ssd_capi.hip into csrc/ssd_solve.h (DESIGN.md section
7i), where the device shares it: the file was written from the build of the commit BEFORE that move (named in the file), and
tests/test_solve_shared.py holds every later build to it bit for bit; tests/test_gpu_surface_gates.py holds k_surface_gates to the
same records.  Run it again only to ADD records, from a build whose host solve is known good - never to make a failing build pass.

Records (moments_frames): the surfaces of tests/surface_model.py's scenes (through the oracle's labels), and crafted ones - n below,
at and above min_points; collinear and coincident points; an isotropic scatter (equal diagonal, zero off-diagonal) and its partial
ties; one off-diagonal exactly 0; sums of either sign; scatter entries with more than 53 significant bits, among them values exactly
on and next to a rounding tie of the 128-bit-to-double conversion; perfectly flat surfaces (level and tilted) for gate_min 0 and > 0;
thin surfaces whose k_sigma * rms lies below gate_min.  Rules (RULES): min_points, k_sigma, gate_min.

Run from the repository root after building:
    python tests/golden/make_solve_goldens.py [COMMIT]
"""
import hashlib
import importlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(HERE, "solve_goldens.json")
RULES = [(200, 2.5, 0.0), (1, 16.0, 0.0), (200, 2.0, 2.0 ** -10)]
MAX_STEPS = 17


def hexd(v):
    return float(v).hex()


def sums_of(q):
    """integer points [N, 3] -> [n, s0, s1, s2, xx, xy, xz, yy, yz, zz, n_far = 0] in Python ints"""
    q = [[int(v) for v in p] for p in np.asarray(q).reshape(-1, 3)]
    out = [len(q), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    for x, y, z in q:
        out[1] += x; out[2] += y; out[3] += z
        out[4] += x * x; out[5] += x * y; out[6] += x * z; out[7] += y * y; out[8] += y * z; out[9] += z * z
    return out


def plane_points(rng, n, centre, span, slope=(0.0, 0.0), sigma=0.0):
    """n fixed-point points (2^-16 m) scattered over a rectangle of half-widths span about centre, on z = cz + slope . (x, y) + noise"""
    x = rng.uniform(-span[0], span[0], n)
    y = rng.uniform(-span[1], span[1], n)
    z = slope[0] * x + slope[1] * y + (rng.normal(0.0, sigma, n) if sigma else 0.0)
    p = np.stack([x + centre[0], y + centre[1], z + centre[2]], axis=1)
    return np.rint(p * 65536.0).astype(np.int64)


def tie_surface(rng, kind):
    """a record stated directly (no point set behind it): n = 2^12 and sums of 0 or +-1, so that N SS - S (x) S is ss * 2^12 (-+ 1): an
    odd 54-bit ss makes the entry a 66-bit number exactly ON a rounding tie of the conversion to double (ss = 1 mod 4 rounds down to
    even, 3 mod 4 up), a sum product of +-1 puts it one unit to either side of the tie.  zz and the couplings xz, yz carry the ties;
    xx and yy are 2^8 times larger, so the plane is OK and its normal and lambda_min move with the rounded bits."""
    def odd54(mod4):
        m = int(rng.integers(1 << 53, 1 << 54))
        return (m & ~3) | mod4
    big = [int(rng.integers(1 << 61, 1 << 62)) | 1 for _ in range(2)]
    zz = odd54(1 if kind & 1 else 3)
    xz = odd54(3 if kind & 2 else 1)
    yz = -odd54(1 if kind & 4 else 3)
    xy = int(rng.integers(1 << 56, 1 << 58)) * (-1 if kind & 8 else 1)
    s = [(0, 0, 0), (1, 1, 1), (1, -1, 1), (-1, 1, -1)][(kind >> 4) & 3]
    return [1 << 12, s[0], s[1], s[2], big[0], xy, xz, big[1], yz, zz, kind & 3]


def crafted():
    """[(name, [11 ints])] - every crafted surface"""
    rng = np.random.default_rng(20240607)
    out = []
    grid = np.array([[x * 4096, y * 4096, 65536 + ((x * 7 + y * 13) % 5 - 2) * 16] for x in range(-8, 9) for y in range(-6, 6)], dtype=np.int64)
    for n in (0, 1, 2, 3, 199, 200, 201):
        out.append(("grid, n = %d" % n, sums_of(grid[:n])))
    out.append(("collinear", sums_of([[i * 300 - 40000, i * 200 + 1000, 70000 + i * 100] for i in range(400)])))
    out.append(("collinear along x", sums_of([[i * 300 - 40000, 5000, 70000] for i in range(400)])))
    out.append(("coincident", sums_of([[12345, -2345, 80000]] * 300)))
    a, b = 3 << 40, 1 << 35
    for name, d in (("isotropic", (a, a, a)), ("tie mid = max, min z", (a, a, b)), ("tie mid = max, min x", (b, a, a)), ("tie mid = max, min y", (a, b, a)),
                    ("tie min = mid", (b, b, a)), ("descending diagonal", (a, 1 << 38, b)), ("ascending diagonal", (b, 1 << 38, a))):
        out.append((name + ", zero off-diagonal", [1024, 0, 0, 0, d[0], 0, 0, d[1], 0, d[2], 0]))
    sym = plane_points(rng, 600, (0.0, 0.3, 1.2), (0.4, 0.2), slope=(0.0, 0.05), sigma=0.002)
    sym = np.concatenate([sym, sym * np.array([-1, 1, 1])])                    # mirrored in x: s0 = xy = xz = 0 exactly
    out.append(("xy and xz exactly 0 (mirrored in x)", sums_of(sym)))
    for sx in (-1, 1):
        for sy in (-1, 1):
            out.append(("sums of sign %+d %+d" % (sx, sy), sums_of(plane_points(rng, 5000, (0.7 * sx, 0.5 * sy, 1.5), (0.3, 0.2), slope=(0.2 * sx, -0.1 * sy), sigma=0.003))))
    out.append(("negative z", sums_of(plane_points(rng, 3000, (0.1, -0.2, -2.0), (0.5, 0.3), slope=(0.1, 0.3), sigma=0.001))))
    out.append(("flat, level", sums_of([[x * 512, y * 512, 98304] for x in range(-20, 20) for y in range(10, 30)])))
    out.append(("flat, tilted (z = x / 4 + y / 2)", sums_of([[x * 512, y * 512, 98304 + x * 128 + y * 256] for x in range(-20, 20) for y in range(10, 30)])))
    out.append(("flat, steep (z = 3 x - 2 y)", sums_of([[x * 64, y * 64, 65536 + x * 192 - y * 128] for x in range(-30, 30) for y in range(-15, 15)])))
    for sigma in (0.00002, 0.0001, 0.0002, 0.001, 0.003, 0.01):
        out.append(("plane, sigma %g m" % sigma, sums_of(plane_points(rng, 20000, (0.2, 0.6, 2.5), (0.6, 0.15), slope=(0.02, 0.7), sigma=sigma))))
    out.append(("far and wide, 2^17 points", sums_of(plane_points(rng, 1 << 17, (3.0, -4.0, 12.0), (3.5, 3.5), slope=(-0.3, 0.4), sigma=0.004))))
    out.append(("thick: lambda_mid < 16 lambda_min", sums_of(plane_points(rng, 4000, (0.0, 0.0, 1.0), (0.3, 0.01), sigma=0.004))))
    out.append(("thick: lambda_mid about 16 lambda_min", sums_of(plane_points(rng, 4000, (0.0, 0.0, 1.0), (0.3, 0.02784), sigma=0.004))))
    for kind in range(64):
        out.append(("conversion tie, kind %d" % kind, tie_surface(rng, kind)))
    return out


def scene_frames(ssd):
    """the records of tests/surface_model.py's scenes, through the oracle's labels: [(name, n_surfaces, ground, [[11 ints]])]"""
    import oracle_binding
    import surface_model as sm
    oracle = oracle_binding.load_oracle()
    out = []
    for name, cfg, frame, truth, cal in sm.accuracy_cases(ssd):
        _, _, fm, _ = sm.oracle_planes(ssd, oracle, cfg, cal, frame)
        rows = [[int(r.m.n)] + [int(v) for v in r.m.s] + [int(v) for v in r.m.ss] + [int(r.n_far)] for r in fm.s[:fm.n_surfaces]]
        out.append(("scene: " + name, int(fm.n_surfaces), int(fm.ground), rows))
    return out


def moments_frames(ssd):
    frames = scene_frames(ssd)
    frames.append(("no surfaces", 0, 0, []))
    rows = crafted()
    for at in range(0, len(rows), MAX_STEPS):
        part = rows[at:at + MAX_STEPS]
        frames.append(("crafted: " + "; ".join(n for n, _ in part), len(part), (at // MAX_STEPS) & 1, [r for _, r in part]))
    return frames


def to_frame_moments(ssd, n_surfaces, ground, rows):
    fm = ssd.FrameMoments()
    fm.n_surfaces, fm.ground = n_surfaces, ground
    for k, r in enumerate(rows):
        m = fm.s[k].m
        m.n = r[0]
        m.s[:] = r[1:4]
        m.ss[:] = r[4:10]
        fm.s[k].n_far = r[10]
    return fm


def prior_calibration(ssd):
    import ground_model as gm
    return ssd.transformation_for_scene(gm.scene(ssd, "steps")).constants


def calibration_hex(c):
    return [hexd(v) for v in list(c.a) + list(c.b) + list(c.r2) + list(c.t2) + [c.world_z]]


def cal_digest(c):
    """a returned calibration as the first 16 hex digits of the SHA-256 of its bytes: bit for bit, at a fraction of the size"""
    return hashlib.sha256(bytes(c)).hexdigest()[:16]


def solve(ssd, fm, cal):
    """everything the three host functions return for one record, as plain JSON types.  Gates: the n_surfaces rows (the rows behind them
    are all zero, which the tests assert).  Fits per min_points, ascending; a surface's row under a smaller min_points is null where it
    equals its row under the largest."""
    n = fm.n_surfaces
    gates = []
    for mp, ks, gm_ in RULES:
        g = ssd.surface_gates_from_moments(fm, mp, ks, gm_)
        assert bytes(g)[8 + 40 * n:] == bytes(40 * (MAX_STEPS - n)) and (g.n_surfaces, g.reserved) == (n, 0)
        gates.append([[hexd(v) for v in list(x.n) + [x.dist, x.gate]] for x in g.g[:n]])
    fits, grounds = [], []
    for mp in sorted({r[0] for r in RULES}):
        f = ssd.surface_fit_solve(fm, cal, mp)
        assert (f.n_surfaces, f.ground) == (n, fm.ground)
        fits.append({"min_points": mp, "s": [[int(s.status), int(s.n), int(s.n_far)] + [hexd(v) for v in list(s.normal) + list(s.centroid) + [s.tilt, s.rms] + list(s.extent)]
                                             for s in f.s[:n]]})
        per = []
        for k in range(n):
            gf = ssd.ground_fit_solve(fm.s[k].m, cal, mp)
            per.append([int(gf.status)] + [hexd(v) for v in list(gf.normal) + [gf.dist, gf.rms, gf.tilt, gf.height_delta]] + [cal_digest(gf.cal)])
        grounds.append({"min_points": mp, "s": per})
    for group in (fits, grounds):
        for entry in group[:-1]:
            entry["s"] = [None if row == last else row for row, last in zip(entry["s"], group[-1]["s"])]
    return {"gates": gates, "surface_fit": fits, "ground_fit": grounds}


def main():
    ssd = importlib.import_module("stair-step-detector_amd")
    commit = sys.argv[1] if len(sys.argv) > 1 else subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True, capture_output=True,
                                                                    text=True).stdout.strip()
    cal = prior_calibration(ssd)
    records = []
    for name, n, ground, rows in moments_frames(ssd):
        fm = to_frame_moments(ssd, n, ground, rows)
        rec = {"name": name, "n_surfaces": n, "ground": ground, "s": rows}
        rec.update(solve(ssd, fm, cal))
        records.append(rec)
    doc = {"written_from_commit": commit,
           "what": "host solve of integer moment records: ssd_surface_gates_from_moments per rule, ssd_surface_fit_solve and ssd_ground_fit_solve "
                   "(each surface's sums as a ground record; the returned calibration as a SHA-256 prefix of its bytes) per min_points, against "
                   "`calibration`; doubles in hex; a null row = the row of the same surface under the largest min_points",
           "rules": [[mp, hexd(ks), hexd(gm_)] for mp, ks, gm_ in RULES],
           "calibration": calibration_hex(cal),
           "records": records}
    with open(OUT, "w") as f:                     # one record per line
        head = {k: v for k, v in doc.items() if k != "records"}
        f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"records":[\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in records))
        f.write("\n]}\n")
    print("%s: %d records, %d surfaces, %d bytes" % (OUT, len(records), sum(r["n_surfaces"] for r in records), os.path.getsize(OUT)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
