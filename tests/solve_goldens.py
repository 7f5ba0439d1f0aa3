"""tests/golden/solve_goldens.json read back for the tests (written by tests/golden/make_solve_goldens.py from the build of the commit
before the solve moved into csrc/ssd_solve.h): the integer moment records as FrameMoments, the rules, and what the host solve returned
for them.  TEST INFRASTRUCTURE; no GPU needed."""
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "solve_goldens.json")
_doc = None


def doc():
    global _doc
    if _doc is None:
        with open(PATH) as f:
            _doc = json.load(f)
    return _doc


def rules():
    """[(min_points, k_sigma, gate_min)]"""
    return [(int(mp), float.fromhex(ks), float.fromhex(gm)) for mp, ks, gm in doc()["rules"]]


def calibration(ssd):
    v = [float.fromhex(x) for x in doc()["calibration"]]
    c = ssd.Calibration()
    c.a[:], c.b[:], c.r2[:], c.t2[:], c.world_z = v[0:9], v[9:12], v[12:16], v[16:18], v[18]
    return c


def frame_moments(ssd, rec):
    """a golden record (or anything with n_surfaces, ground and rows of eleven integers) -> FrameMoments"""
    fm = ssd.FrameMoments()
    fm.n_surfaces, fm.ground = rec["n_surfaces"], rec["ground"]
    for k, r in enumerate(rec["s"]):
        m = fm.s[k].m
        m.n = r[0]
        m.s[:] = r[1:4]
        m.ss[:] = r[4:10]
        fm.s[k].n_far = r[10]
    return fm


def gates_of(ssd, rec, rule):
    """the golden FrameGates of a record under rule number `rule` (the file holds the n_surfaces rows; the rest is zero)"""
    g = ssd.FrameGates()
    g.n_surfaces = rec["n_surfaces"]
    for k, row in enumerate(rec["gates"][rule]):
        v = [float.fromhex(x) for x in row]
        g.g[k].n[:] = v[0:3]
        g.g[k].dist, g.g[k].gate = v[3], v[4]
    return g


def fits_of(rec, key):
    """rec["surface_fit"] or rec["ground_fit"] with the null rows filled in: [(min_points, [row per surface])]"""
    last = rec[key][-1]["s"]
    return [(e["min_points"], [l if r is None else r for r, l in zip(e["s"], last)]) for e in rec[key]]


def cal_digest(c):
    return hashlib.sha256(bytes(c)).hexdigest()[:16]
