"""What tests/test_gpu_follow_geometry.py and tests/test_chunk_plan.py share: tests/chunk_plan_main.cpp built with g++ and run (the plans
of csrc/ssd_chunks.h under the default tuning), the three block geometries the follow-on passes are held to, and the template frames a
large batch is made of.  TEST INFRASTRUCTURE; no GPU needed."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "stair-step-detector_amd", "csrc")
TILE = 1024


def build_chunk_plan(directory):
    """tests/chunk_plan_main.cpp -> the program's path in `directory`"""
    exe = os.path.join(str(directory), "chunk_plan_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "chunk_plan_main.cpp"), "-o", exe], check=True)
    return exe


def chunk_plans(exe, pairs):
    """the program on (nPoints, nframes) pairs -> (tile, bounds per kernel, {(nPoints, nframes): {"chunk", "hist", "raster", "inquad"}})"""
    args = [str(v) for pair in pairs for v in pair]
    lines = subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    tile, max_tiles, max_raster, max_inquad = (int(x) for x in lines[0].split())
    bounds = {"chunk": max_tiles * tile, "hist": max_tiles * tile, "raster": max_raster * tile, "inquad": max_inquad * tile}
    got = {}
    for line in lines[1:]:
        n, f, chunk, hist, raster, inquad = (int(x) for x in line.split())
        got[(n, f)] = {"chunk": chunk, "hist": hist, "raster": raster, "inquad": inquad}
    return tile, bounds, got


# ---- the geometries: (width, height, frames, tiles of `chunk`, tiles with one frame fewer), per input -------------------------------------
# A: the product's geometry (512 cells, both passes of the cell list full, 32 groups per wave, 24 whole chunks per frame).  B: the second
# list pass part-filled (272 cells), 17 chunks and a tail of 11 tiles per frame, chunk boundaries in the middle of a camera row.  C: a frame
# that is no whole number of cells (250 x 190: the last block holds 1420 points = 23 cells, the last cell 12 points).
GEOMETRY = {
    ("A", False): (1024, 768, 342, 32, 31), ("A", True): (1024, 768, 342, 32, 31),
    ("B", False): (640, 480, 465, 17, 16), ("B", True): (640, 480, 465, 17, 16),
    ("C", False): (250, 190, 884, 5, 4), ("C", True): (252, 191, 872, 5, 4),
}
SINGLE_PASS_MIN_POINTS = 64 * 1024 * 768          # csrc/ssd_launch.h: kSinglePassMinPoints (vertex input only)

# ---- the templates ---------------------------------------------------------------------------------------------------------------------------
# Staircases with visible risers (tests/test_gpu_surface_fit.py's "xga" pose: rolled by 30 degrees, steps of 7 cm, so camera rows cross
# from one surface to the next and a chunk holds several surfaces).  Template t sits at frames i with (7 i) % D == t, i.e. in the order
# 0, 7, 6, 5, 4, 3, 2, 1: the thrown frame (2), the all-zero frame (4) and the bare floor (6) sit between live ones, and the first and
# last frame of every geometry above (t = 0, and 3, 0, 5, 1 at 342, 465, 884, 872 frames) are live.
D = 8
KINDS = ("live", "occupant", "thrown", "many", "zero", "occupant", "floor", "live")
SMALL = ((250, 190), (252, 191))


# 640 x 480 runs with a world range that holds every point the camera sees: at the default range a fifth of a row's cells lie outside x and
# hold no wanted bin, and no chunk of 272 cells lists more than 256 - the second pass of the cell list would stay empty.  FIRST_PASS_CELLS:
# what the first pass of cell_list_build's fast path holds (csrc/ssd_k_cells.h)
FIRST_PASS_CELLS, CELL = 256, 64
WIDE_RANGE = {(640, 480): (-1.0, 1.0, 2.2)}


def pose_of(shape):
    """250 x 190 shows steps of 7 cm as two surfaces: the small shapes take tests/test_gpu_surface_fit.py's pose for them"""
    return dict(roll_deg=25.0) if shape in SMALL else dict(roll_deg=30.0, rise=0.07)


def scenes_of(shape):
    """make_scene keywords per template (None: the all-zero frame).  The thrown one and the many-step one were looked for per shape with
    the oracle, under the shape's pose and range; the small shapes report at most 5 of 8 built steps.  At 640 x 480 the many-step
    staircase is 3 m wide: it fills the frame, so that whole chunks of 272 cells hold a tread in every cell (Templates.dense_cells)"""
    throw = {(1024, 768): dict(yaw_deg=24.0, stair_width=0.8), (640, 480): dict(yaw_deg=30.0, stair_width=0.8)}.get(shape, dict(yaw_deg=30.0, stair_width=1.5))
    many = dict(tread=0.14, rise=0.12, first_riser_y=0.15) if shape in SMALL else dict(tread=0.12, first_riser_y=0.15)
    if shape in WIDE_RANGE:
        many.update(stair_width=3.0, outlier_frac=0.02)        # outliers: occupants in every part of the frame, for clearance
    noise = 0.5 if shape in SMALL else 1.0         # at 2 mm of noise the small shapes report two of the three steps
    return (
        dict(n_steps=3, seed=11, sigma=0.001),
        dict(n_steps=3, seed=12, sigma=0.0015),
        dict(n_steps=3, seed=100, sigma=0.002, **throw),
        dict(n_steps=8, seed=13, sigma=0.001, **many),
        None,
        dict(n_steps=3, seed=17, sigma=0.002 * noise),
        dict(n_steps=0, seed=5, sigma=0.001),
        dict(n_steps=3, seed=19, sigma=0.0025 * noise, outlier_frac=0.05 * noise * noise),
    )


def many_steps(shape):
    return 5 if shape in SMALL else 6


# template -> the surface its box stands on: the ground in front of the stairs and the top tread (a box of 10 cm on the middle tread of
# steps 7 cm high leaves hardly a point inside the tread's shrunk quadrilateral)
OCCUPANT_SURFACE = {1: 0, 5: -1}
# the cameras form: poses a little apart; template t is camera CAMERA_OF_TEMPLATE[t]'s (the thrown and the many-step one camera 0's: under
# the other poses they are neither), which is table entry TABLE_OF_CAMERA[camera]; UNUSED is nobody's
CAMERA_POSES = (dict(), dict(pitch_deg=52.0), dict(cam_height=1.05, roll_deg=31.0))
CAMERA_OF_TEMPLATE = (1, 2, 0, 0, 1, 2, 0, 1)
TABLE_OF_CAMERA, UNUSED = (2, 0, 3), 1


def which(nframes):
    """the template of every frame"""
    return [(7 * i) % D for i in range(nframes)]


class Templates:
    """the D template frames of one shape and input, and the oracle's word on them; made once and never written to.
    scenes[t]: the generated scene behind template t (the all-zero frame: the floor's, overwritten); frames[t]: float32 [H, W, 3] or
    uint16 [H, W]; pts[t]: the points they stand for; patched[t]: the frame is not its scene's (uploaded, not generated);
    camera[t]: whose frame it is (cameras form), cals / trans: per camera"""

    def __init__(self, ssd, oracle, w, h, depth, cameras=False):
        import clearance_model as cm
        import oracle_binding as ob
        from test_labels import expected_labels
        self.w, self.h, self.depth, self.cameras = w, h, depth, cameras
        self.shape = (w, h)
        self.camera = [CAMERA_OF_TEMPLATE[t] if cameras else 0 for t in range(D)]
        poses = [dict(pose_of(self.shape), **p) for p in CAMERA_POSES] if cameras else [pose_of(self.shape)]
        self.scenes, kws = [], scenes_of(self.shape)
        for t in range(D):
            kw = dict(poses[self.camera[t]], **(kws[t] if kws[t] is not None else kws[6]))
            if kw["n_steps"] == 0:
                kw.pop("rise", None)
            self.scenes.append(ssd.make_scene(w, h, **kw))
        views = [ssd.make_scene(w, h, n_steps=0, **{k: v for k, v in p.items() if k != "rise"}) for p in poses]
        self.trans = [ssd.transformation_for_scene(sc) for sc in views]
        self.cals = [t.constants for t in self.trans]
        self.intr = ssd.intrinsics_for_scene(views[0]) if depth else None
        self.cfg = ssd.default_config(w, h)
        if self.shape in WIDE_RANGE:
            self.cfg.x_min, self.cfg.x_max, self.cfg.y_max = WIDE_RANGE[self.shape]
        frames = list(ssd.synth_depth_host(self.scenes)) if depth else list(ssd.synth_host(self.scenes))
        self.generated = [f.copy() for f in frames]
        frames[4] = np.zeros_like(frames[4])
        self.patched = [t == 4 or t in OCCUPANT_SURFACE for t in range(D)]
        ocfg = ob.to_oracle_config(self.cfg)

        def points(f):
            return ssd.deproject_host(self.intr, f) if depth else f

        def record(t, p):
            return oracle.process(ocfg, ob.to_oracle_calibration(self.cals[self.camera[t]]), p)[0]

        for t, surface in OCCUPANT_SURFACE.items():
            p, cal = points(frames[t]), self.cals[self.camera[t]]
            rec = record(t, p)
            res = cm.result_of_oracle(ssd, rec)
            assert rec.n_steps >= 3 and not (rec.status & ob.ST_THROW), (t, rec.n_steps)
            f2, sel = cm.patched(self.cfg, cal, res, p, expected_labels(oracle, self.cfg, cal, rec, p), surface % rec.n_steps,
                                  n=80 if self.shape in SMALL else 300)
            if depth:
                f2 = frames[t].copy()
                f2[sel] = np.round(f2[sel] * 0.9).astype(np.uint16)
            frames[t] = f2
        self.frames = [np.ascontiguousarray(f) for f in frames]
        self.pts = [points(f) for f in self.frames]
        self.records = [record(t, p) for t, p in enumerate(self.pts)]
        self.thrown = [bool(r.status & ob.ST_THROW) for r in self.records]
        self.steps = [int(r.n_steps) for r in self.records]
        self.labels = [expected_labels(oracle, self.cfg, self.cals[self.camera[t]], r, p) for t, (r, p) in enumerate(zip(self.records, self.pts))]
        for a in self.frames + self.pts + self.labels + self.generated:
            a.setflags(write=False)

    def dense_cells(self, t, chunk_points, least=2):
        """per chunk of template t, the 64-point cells that hold a pixel labelled `least` or above (2: a tread above surface 0) by
        expected_labels: every such cell holds a wanted bin of the label, moment and refit passes, and - a tread of low steps lying in
        the band above the surface below it - of clearance"""
        lab, out = self.labels[t], []
        for at in range(0, lab.size, chunk_points):
            part = lab[at:at + chunk_points]
            part = np.concatenate([part, np.zeros(-part.size % CELL, dtype=part.dtype)]).reshape(-1, CELL)
            out.append(int(np.count_nonzero(part.max(axis=1) >= least)))
        return out

    def cal_of(self, t):
        return self.cals[self.camera[t]]

    def live(self, t):
        return not self.thrown[t] and self.steps[t] > 0

    def check_layout(self, nframes):
        """what the layout asks for, by the oracle alone: live staircases, a many-step frame, a bare floor, an all-zero frame, a thrown
        one where the shape gives one, and thrown and empty frames between live ones"""
        for t, kind in enumerate(KINDS):
            if kind in ("live", "occupant"):
                assert self.live(t) and self.steps[t] >= 3, (t, kind, self.steps[t])
            elif kind == "many":
                assert self.live(t) and self.steps[t] >= many_steps(self.shape), (t, self.steps[t])
            elif kind == "floor":
                assert not self.thrown[t] and self.steps[t] <= 1 and np.any(self.pts[t]), (t, self.steps[t])
            elif kind == "zero":
                assert not np.any(self.frames[t]) and self.steps[t] == 0
            elif kind == "thrown":
                assert self.thrown[t], t
        order = which(nframes)
        dead = [t for t in range(D) if not (self.live(t) and self.steps[t] >= 2)]
        assert order[0] not in dead and order[-1] not in dead
        for i in range(1, nframes - 1):
            assert order[i] not in dead or (order[i - 1] not in dead and order[i + 1] not in dead), i


_TEMPLATES = {}


def templates(ssd, oracle, w, h, depth, cameras=False):
    key = (w, h, depth, cameras)
    if key not in _TEMPLATES:
        _TEMPLATES[key] = Templates(ssd, oracle, w, h, depth, cameras)
    return _TEMPLATES[key]
