"""A handle's resources over its whole life (csrc/ssd_owned.h, csrc/ssd_handle.h): every lazily made buffer, event and stream enabled
and used on ONE handle - in one order and, on a fresh handle, in the reverse order -, with ssd_workspace_bytes after every step, the
buffers that grow, and handles made and closed in a row.  256 x 192, four frames per batch, one workspace and three.

What a step adds to workspace_bytes is what include/ssd_hip.h and DESIGN.md say it holds: device memory only for debug capture,
risers, riser moments, the ground fit, the camera table and the camera fold; device and pinned memory for the refit's gates; nothing
for timing events, the host feed's and the labels' staging buffers and streams, the per-batch pinned buffers, and the planes the
single-pass test hook makes."""
import ctypes as C

import numpy as np
import pytest

W, H, F = 256, 192, 4
NBATCH = 9                                          # frames of the largest host-fed batch: three slices of at most F
ORDER = [0, 1, 1, 0]                                # the cameras of a batch's frames
TOL, FOLD_MIN = 0.05, 1000


def _b(records):
    return [bytes(r) for r in records]


class World:
    """frames of one mounting (every scene shares the calibration), on the host and the first F of them on the device"""

    def __init__(self, ssd, device, width, height):
        self.ssd, self.device, self.W, self.H = ssd, device, width, height
        self.scenes = [ssd.make_scene(width, height, n_steps=3, seed=31 + i, sigma=0.001 + 0.0002 * i) for i in range(NBATCH)]
        self.trans = ssd.transformation_for_scene(self.scenes[0])
        assert all(bytes(ssd.transformation_for_scene(s).constants) == bytes(self.trans.constants) for s in self.scenes)
        self.intr = ssd.intrinsics_for_scene(self.scenes[0])
        self.xyz = np.ascontiguousarray(ssd.synth_host(self.scenes), dtype=np.float32)
        self.depth = np.ascontiguousarray(ssd.synth_depth_host(self.scenes), dtype=np.uint16) if width % 4 == 0 else None
        self.buf = ssd.DeviceBuffer(width * height * 12 * F, device)
        self.buf.upload(self.xyz[:F].reshape(-1).view(np.uint8))
        self.table = [(self.trans, self.intr), (self.trans, self.intr)]

    def detector(self, lanes):
        return self.ssd.Detector(self.ssd.default_config(self.W, self.H, max_frames_per_batch=F, batches_in_flight=lanes), self.trans, self.device)

    def close(self):
        self.buf.free()


@pytest.fixture(scope="module")
def world(ssd, gpu_device):
    w = World(ssd, gpu_device, W, H)
    yield w
    w.close()


@pytest.fixture(scope="module")
def camera_record_bytes(ssd, world):
    """one camera's device record, from two tables on a handle of one frame and one workspace: a table of n cameras without intrinsics
    holds n records and one index of 4 bytes per frame"""
    det = ssd.Detector(ssd.default_config(W, H, max_frames_per_batch=1), world.trans, world.device)
    base = det.workspace_bytes
    det.set_cameras([world.trans])
    one = det.workspace_bytes - base
    det.set_cameras([world.trans, world.trans])
    two = det.workspace_bytes - base
    det.close()
    assert one == (two - one) + 4 and two - one > 0
    return two - one


class Life:
    """one handle and what its workspace_bytes must be"""

    def __init__(self, world, lanes, camera_record_bytes):
        self.w, self.ssd, self.lanes, self.rec = world, world.ssd, lanes, camera_record_bytes
        self.det = world.detector(lanes)
        assert self.det.batches_in_flight == lanes
        self.bytes = self.det.workspace_bytes
        self.table = self.fold = False

    def did(self, share, what):
        self.bytes += share
        assert self.det.workspace_bytes == self.bytes, what

    def batch(self):
        self.det.enqueue(self.w.buf.ptr, F)
        return self.det.fetch_list(F)

    def set_table(self):
        share = 2 * self.rec + 2 * (W + H) * 4 + self.lanes * F * 4      # the records, each camera's maps, a frame index per workspace
        self.det.set_cameras(self.w.table)
        self.did(0 if self.table else share, "the camera table: once, however often it is set")
        self.table = True
        return share

    # ---- the steps: each enables something made on first use, uses it, and says what it may have added
    def captures(self):
        ssd, det, cfg = self.ssd, self.det, self.det.cfg
        words = H * ((W + 63) // 64)
        det.set_debug(True, images=True)
        self.did(F * C.sizeof(ssd.DebugFrame) + F * (cfg.max_step_plateaus + 1) * 2 * words * 8, "debug capture: the records and two images per slot")
        self.batch()
        assert det.debug(0).n_plateaus >= 0 and det.debug_image(0, -1, False).shape == (H, W)
        det.set_debug(False)
        det.set_timing(True)
        self.did(0, "timing: events only")
        self.batch()
        assert len(det.stage_times_ms()) == 7
        det.set_risers(True)
        self.did(F * C.sizeof(ssd.FrameRisers), "risers: their device records")
        self.batch()
        assert len(det.fetch_risers(F)) == F
        det.set_riser_moments(True)
        self.did(F * C.sizeof(ssd.FrameMoments), "riser moments: their device records")
        self.batch()
        assert len(det.fetch_riser_moments(F)) == F
        det.set_riser_moments(False)
        det.set_risers(False)
        self.did(0, "switching off keeps the buffers")

    def cameras(self):
        self.set_table()
        self.det.enqueue_cameras(self.w.buf.ptr, F, ORDER)
        assert len(self.det.fetch_list(F)) == F
        self.did(0, "a cameras batch allocates nothing counted")

    def host_labels(self):
        self.det.process_host_labels(self.w.xyz[:F])
        self.did(0, "the host feed's and the labels' staging: not counted")

    def host_moments(self):
        self.det.process_host_surfaces(self.w.xyz[:F], moments=True)
        self.did(0, "the moments' staging: not counted")

    def ground_fit(self):
        self.det.enqueue_ground_fit(self.w.buf.ptr, F, TOL)
        assert len(self.det.fetch_ground_fit(F)) == F
        self.did(F * (C.sizeof(self.ssd.GroundMoments) + 128), "the ground fit: device records and device priors")

    def refits(self):
        ssd, det = self.ssd, self.det
        gates = 2 * F * C.sizeof(ssd.FrameGates)
        det.process_host_surfaces_refit(self.w.xyz[:F], passes=1)
        self.did(0 if getattr(self, "gated", False) else gates, "host-gated refit: the gates on the device and pinned")
        self.gated = True
        assert det.surface_refit_time_ms() >= 0.0
        det.process_host_surfaces_refit(self.w.xyz[:F], passes=2, device_gates=True)
        self.did(0, "device-gated refit: the same gates")
        self.set_table()
        fold = ssd.MAX_CAMERAS * C.sizeof(ssd.CameraFold)
        det.camera_drift_resident(self.w.buf.ptr, F, ORDER, passes=2, fold_min_points=FOLD_MIN)
        self.did(0 if self.fold else fold, "folded refit: the fold buffer, once")
        self.fold = True
        det.camera_drift(self.w.xyz, ORDER * 2 + [0], passes=1, min_points=FOLD_MIN, device_fold=True)
        self.did(0, "the drift call: the same fold buffer")

    def forced_single_pass(self):
        self.det.single_pass(1)                    # 1024 % 256 == 0: the geometry allows it
        self.did(0, "the hook's planes are not counted")
        self.batch()
        assert self.det.single_pass_stats(F, scan_planes=False)["ran"]

    STEPS = ("captures", "cameras", "host_labels", "host_moments", "ground_fit", "refits", "forced_single_pass")

    def run(self, steps):
        for name in steps:
            getattr(self, name)()

    def give_back(self, base):
        share = 2 * self.rec + 2 * (W + H) * 4 + self.lanes * F * 4
        self.det.set_cameras([])
        self.did(-share, "an empty table gives the table's share back")
        self.det.set_single_pass(False)
        self.did(0, "planes that were not counted give nothing back")
        assert self.bytes > base

    def last_batch(self):
        """what a handle is compared by: a host-fed batch with its labels, one with its moment records, a resident one"""
        res, labels = self.det.process_host_labels(self.w.xyz[:F])
        res2, _, moments = self.det.process_host_surfaces(self.w.xyz[:F], moments=True)
        return _b(res), labels.tobytes(), _b(res2), _b(moments), _b(self.batch())


@pytest.fixture(scope="module")
def fresh(world, camera_record_bytes):
    """the last batch on handles that ran nothing else, by workspaces: computed once"""
    out = {}
    for lanes in (1, 3):
        life = Life(world, lanes, camera_record_bytes)
        out[lanes] = life.last_batch()
        life.det.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_everything_in_one_life(world, camera_record_bytes, fresh, lanes, order):
    life = Life(world, lanes, camera_record_bytes)
    base = life.bytes
    try:
        life.run(Life.STEPS if order == "forward" else Life.STEPS[::-1])
        life.give_back(base)
        got = life.last_batch()
        assert got[0] == fresh[lanes][0] and got[2] == fresh[lanes][2] and got[4] == fresh[lanes][4], "results"
        assert got[1] == fresh[lanes][1], "labels"
        assert got[3] == fresh[lanes][3], "moment records"
        assert fresh[1] == fresh[3]
    finally:
        life.det.close()


# ---- growth: 250 x 190 (no multiple of the tile, of a cell or of 64), and 252 x 191 for 16-bit depth, which the pipeline takes only at
# widths that are multiples of 4: there W * H * 2 % 16 == 8, so the ground fit's frames (16 bytes apart) need more than the pipeline's (8)
@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_buffers_grow_with_the_batch(ssd, gpu_device, lanes):
    w = World(ssd, gpu_device, 250, 190)
    try:
        det = w.detector(lanes)
        det.set_risers(True)
        det.set_riser_moments(True)
        small = _b(det.process_host(w.xyz[:3])), _b(det.fetch_risers(3)), _b(det.fetch_riser_moments(3))
        large = _b(det.process_host(w.xyz)), _b(det.fetch_risers(NBATCH)), _b(det.fetch_riser_moments(NBATCH))     # three slices; the pinned batch buffers grow
        fits = _b(det.process_host_ground_fit(w.xyz, TOL))
        det.close()
        for frames, want in ((w.xyz[:3], small), (w.xyz, large)):
            one = w.detector(lanes)
            one.set_risers(True)
            one.set_riser_moments(True)
            assert (_b(one.process_host(frames)), _b(one.fetch_risers(len(frames))), _b(one.fetch_riser_moments(len(frames)))) == want
            one.close()
        one = w.detector(lanes)
        assert _b(one.process_host_ground_fit(w.xyz, TOL)) == fits
        one.close()
    finally:
        w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_ingest_buffers_grow_from_the_pipeline_to_the_ground_fit(ssd, gpu_device, lanes):
    w = World(ssd, gpu_device, 252, 191)
    assert w.W * w.H * 2 % 16 == 8
    prior = [(w.trans, w.intr)]
    try:
        det = w.detector(lanes)
        det.set_intrinsics(w.intr)
        res = _b(det.process_depth_host(w.depth))                                          # slices of 4 frames, 8-byte frame stride
        fits = _b(det.process_host_ground_fit(w.depth, TOL, priors=prior, depth=True))     # 16-byte frame stride: larger slices
        again = _b(det.process_depth_host(w.depth))                                        # and the pipeline in the grown buffers
        det.close()
        assert again == res
        one = w.detector(lanes)
        assert _b(one.process_host_ground_fit(w.depth, TOL, priors=prior, depth=True)) == fits
        one.close()
        one = w.detector(lanes)
        one.set_intrinsics(w.intr)
        assert _b(one.process_depth_host(w.depth)) == res
        one.close()
    finally:
        w.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 3])
def test_create_and_close_in_a_row(world, camera_record_bytes, fresh, lanes):
    first = None
    for _ in range(3):
        life = Life(world, lanes, camera_record_bytes)
        life.run(Life.STEPS)
        plain = _b(life.batch())
        life.det.close()
        first = first or plain
        assert plain == first
    fourth = world.detector(lanes)
    fourth.enqueue(world.buf.ptr, F)
    assert _b(fourth.fetch_list(F)) == first == fresh[lanes][4]
    fourth.close()
