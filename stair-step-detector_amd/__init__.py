"""Host-side Python binding of libssd_hip.so (ctypes over the C ABI in include/ssd_hip.h).

The package name carries the reference's name and therefore a hyphen; import it with
``importlib.import_module("stair-step-detector_amd")``.

Mirrors the reference's interface for the per-frame path:

* ``GeometricTransformation(world_points, camera_points)``  -> reference transformation.h:102-126
* ``Pointcloud(window, trans).process(frame)``              -> reference pointcloud.h:32-42, pointcloud.cpp:608-626
* ``Stairs.serialize()``                                    -> reference stairs.cpp:55-70

There is no CPU implementation here: every compute call goes to the HIP library and fails
loudly (``SsdError``) when the library or a GPU is missing.  The CPU oracle lives under
``oracle/`` and is never imported by this package.
"""
import ctypes as C
import math
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SSD_HIP_LIB") or os.path.join(_HERE, "lib", "libssd_hip.so")   # override: sanitizer builds (tools/)

MAX_BINS = 128
MAX_PLATEAUS = 32
MAX_STEP_IMAGES = 16
MAX_PLANES = 24
POOL_PLANES_PER_FRAME = 10


def plane_pool_size(frames, points_per_frame):
    """planes a workspace holds for batches of up to `frames` frames (csrc/ssd_device.h: plane_pool_size)"""
    per = 16 if points_per_frame < 600000 else POOL_PLANES_PER_FRAME
    return max(frames * per + 2 * MAX_PLANES, min(frames, 8) * MAX_PLANES)
MAX_STEPS = MAX_STEP_IMAGES + 1
LABEL_RISER_BASE = 32                # SSD_LABEL_RISER_BASE: label LABEL_RISER_BASE + i = evidence of riser i (Detector.set_riser_labels)
MAX_SCANS = 128
MAX_EDGE_PTS = 256
LINE_CAP = 4096

ST_THROW, ST_OOB_PIXEL, ST_ASSERT, ST_OVERFLOW = 1, 2, 4, 8
STAGE_HIST, STAGE_PEAKS, STAGE_RASTER, STAGE_OUTLINE, STAGE_QUADS, STAGE_INQUAD, STAGE_FINAL = 1, 2, 4, 8, 16, 32, 64
STAGE_ALL = 127
STAGE_NAMES = ("hist", "peaks", "raster", "outline", "quads", "inquad", "final")
E_NODEVICE = -4
BATCHES_IN_FLIGHT_THROUGHPUT = 3     # SSD_BATCHES_IN_FLIGHT_THROUGHPUT


class SsdError(RuntimeError):
    pass


class Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("x_min", C.c_double), ("x_max", C.c_double), ("y_min", C.c_double), ("y_max", C.c_double),
                ("z_min", C.c_double), ("z_max", C.c_double),
                ("height_interval", C.c_double), ("min_height_above_ground", C.c_double), ("min_step_depth", C.c_double),
                ("max_frames_per_batch", C.c_int32), ("max_step_plateaus", C.c_int32),
                ("batches_in_flight", C.c_int32)]


class Calibration(C.Structure):
    _fields_ = [("a", C.c_double * 9), ("b", C.c_double * 3), ("r2", C.c_double * 4), ("t2", C.c_double * 2),
                ("world_z", C.c_double)]


class Riser(C.Structure):
    """ssd_riser (extension: vertical faces, include/ssd_hip.h)"""
    _fields_ = [("n_points", C.c_int32), ("detected", C.c_int32), ("height_bottom", C.c_double), ("height_top", C.c_double),
                ("left", C.c_double * 2), ("right", C.c_double * 2), ("mean_offset", C.c_double)]


class Step(C.Structure):
    _fields_ = [("height", C.c_double), ("quad", C.c_double * 8)]


class FrameResult(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("status", C.c_int32), ("steps", Step * MAX_STEPS)]


class FrameRisers(C.Structure):
    _fields_ = [("n_risers", C.c_int32), ("reserved", C.c_int32), ("risers", Riser * (MAX_STEPS - 1))]


class DebugPlateau(C.Structure):
    _fields_ = [("peak_bin", C.c_int32), ("bin_lo", C.c_int32), ("bin_hi", C.c_int32),
                ("eff_lo", C.c_int32), ("eff_hi", C.c_int32), ("n_points", C.c_int32),
                ("is_step", C.c_int32), ("outline_found", C.c_int32), ("valid", C.c_int32),
                ("n_scans_right", C.c_int32), ("n_scans_left", C.c_int32),
                ("scans_right", (C.c_int32 * 3) * MAX_SCANS), ("scans_left", (C.c_int32 * 3) * MAX_SCANS),
                ("n_edge_pts", C.c_int32 * 4), ("line", (C.c_int32 * 3) * 4),
                ("bounds", ((C.c_double * 2) * 2) * 4), ("base_line", C.c_double * 3),
                ("vedge_found", C.c_int32 * 2), ("n_vpts", C.c_int32 * 2),
                ("vpts", ((C.c_int32 * 2) * MAX_EDGE_PTS) * 2), ("best_pt", (C.c_int32 * 2) * 2),
                ("vline", (C.c_double * 3) * 2), ("corner_found", C.c_int32 * 4),
                ("quad_img", C.c_double * 8), ("quad_world", C.c_double * 8),
                ("quad_err", C.c_int32), ("n_in_quad", C.c_int32), ("sum_z_fix", C.c_int64), ("mean_z", C.c_double)]


class DebugFrame(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_nonzero", C.c_int32), ("n_inrange", C.c_int32), ("n_oob", C.c_int32),
                ("n_bins", C.c_int32), ("min_height", C.c_int32), ("min_img_y_extent", C.c_int32),
                ("hist", C.c_uint32 * MAX_BINS), ("n_peaks", C.c_int32), ("peaks", C.c_int32 * MAX_PLATEAUS),
                ("n_plateaus", C.c_int32), ("first_step", C.c_int32), ("ground_ind", C.c_int32),
                ("first_valid_ind", C.c_int32),
                ("ground_quad_world", C.c_double * 8), ("ground_quad_err", C.c_int32),
                ("ground_n_in_quad", C.c_int32), ("ground_mean_z", C.c_double),
                ("ground_front_valid", C.c_int32), ("ground_n_pts", C.c_int32),
                ("ground_pts", (C.c_int32 * 2) * MAX_SCANS), ("ground_line", C.c_int32 * 3),
                ("ground_front_img", C.c_double * 4),
                ("plateaus", DebugPlateau * MAX_PLATEAUS)]


class DeviceInfo(C.Structure):
    """ssd_device_info: which physical GPU a device index is, and the CPUs next to it"""
    _fields_ = [("pci_bus_id", C.c_char * 32), ("uuid", C.c_char * 40), ("numa_node", C.c_int32), ("n_local_cpus", C.c_int32),
                ("cpu_list", C.c_char * 256)]


class Intrinsics(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("ppx", C.c_float), ("ppy", C.c_float), ("depth_units", C.c_float)]


class Camera(C.Structure):
    """ssd_camera: one camera of a handle's table (Detector.set_cameras): its calibration and, for depth input, its intrinsics"""
    _fields_ = [("cal", Calibration), ("intr", Intrinsics), ("has_intrinsics", C.c_int32), ("reserved", C.c_int32)]


MAX_CAMERAS = 4096
INPUT_VERTICES, INPUT_DEPTH16 = 0, 1

GF_OK, GF_FEW, GF_DEGENERATE = 0, 1, 2
GF_PLANARITY = 16.0


class GroundMoments(C.Structure):
    """ssd_ground_moments: a frame's floor points as exact integer sums of q = rint(v * 65536) (ground fit)"""
    _fields_ = [("n", C.c_int64), ("s", C.c_int64 * 3), ("ss", C.c_int64 * 6)]


class GroundFit(C.Structure):
    """ssd_ground_fit: the moments, the fitted plane and the refined calibration (status != GF_OK: cal is the prior)"""
    _fields_ = [("m", GroundMoments), ("status", C.c_int32), ("reserved", C.c_int32), ("normal", C.c_double * 3), ("dist", C.c_double),
                ("rms", C.c_double), ("tilt", C.c_double), ("height_delta", C.c_double), ("cal", Calibration)]


class SurfaceMoments(C.Structure):
    """ssd_surface_moments: the ten sums of the points of one surface, and the labelled points at or beyond 16 m left out of them"""
    _fields_ = [("m", GroundMoments), ("n_far", C.c_int64)]


class FrameMoments(C.Structure):
    """ssd_frame_moments: a frame's surfaces (the order of its FrameResult) as exact integer moments (surface fit)"""
    _fields_ = [("n_surfaces", C.c_int32), ("ground", C.c_int32), ("s", SurfaceMoments * MAX_STEPS)]


class SurfaceFit(C.Structure):
    """ssd_surface_fit: one surface's plane in external world coordinates (status != GF_OK: the doubles are 0)"""
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("n_far", C.c_int64), ("normal", C.c_double * 3),
                ("centroid", C.c_double * 3), ("tilt", C.c_double), ("rms", C.c_double), ("extent", C.c_double * 2)]


class FrameSurfaces(C.Structure):
    """ssd_frame_surfaces: the fitted plane of every surface of a frame"""
    _fields_ = [("n_surfaces", C.c_int32), ("ground", C.c_int32), ("s", SurfaceFit * MAX_STEPS)]


class PlaneGate(C.Structure):
    """ssd_plane_gate: a plane in camera coordinates and a half-width; a point is kept iff |n . p - dist| <= gate (trimmed surface
    refit)"""
    _fields_ = [("n", C.c_double * 3), ("dist", C.c_double), ("gate", C.c_double)]


class FrameGates(C.Structure):
    """ssd_frame_gates: a frame's gates, one per surface (the order of its FrameMoments)"""
    _fields_ = [("n_surfaces", C.c_int32), ("reserved", C.c_int32), ("g", PlaneGate * MAX_STEPS)]


class ClearanceRule(C.Structure):
    """ssd_clearance_rule: how far inside a surface's sides (margin) and how high above it (lo, hi) an occupant lies, metres (tread
    clearance)"""
    _fields_ = [("margin", C.c_double), ("lo", C.c_double), ("hi", C.c_double)]

    def __init__(self, margin=0.03, lo=0.03, hi=0.5):
        super().__init__(float(margin), float(lo), float(hi))


CL_FREE, CL_OCCUPIED = 0, 1


class Clearance(C.Structure):
    """ssd_clearance: what stands on one surface, external world coordinates (status CL_FREE: the doubles are 0)"""
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("n_far", C.c_int64), ("centroid", C.c_double * 3),
                ("height_mean", C.c_double), ("height_rms", C.c_double), ("from_front", C.c_double), ("along_front", C.c_double),
                ("extent", C.c_double * 3)]


class FrameClearance(C.Structure):
    """ssd_frame_clearance: the occupants of every surface of a frame"""
    _fields_ = [("n_surfaces", C.c_int32), ("ground", C.c_int32), ("s", Clearance * MAX_STEPS)]


TG_COLS, TG_ROWS = 32, 8
TG_OUT, TG_FREE, TG_OCCUPIED, TG_UNSEEN = 0, 1, 2, 3


class TreadGridRule(C.Structure):
    """ssd_tread_grid_rule: the clearance rule that decides which points stand on which surface, and the side of a grid cell, metres
    (tread grid)"""
    _fields_ = [("clearance", ClearanceRule), ("cell", C.c_double)]

    def __init__(self, margin=0.03, lo=0.03, hi=0.5, cell=0.02):
        super().__init__(ClearanceRule(margin, lo, hi), float(cell))


class TreadGrid(C.Structure):
    """ssd_tread_grid: one surface's grid - per cell [row behind the front edge][column along it] the tread points seen, the occupants
    and the tallest occupant (units of 2^-16 m); the *_out fields hold what falls outside the grid"""
    _fields_ = [("n_seen_out", C.c_uint32), ("n_occ_out", C.c_uint32), ("top_out", C.c_int32), ("reserved", C.c_int32),
                ("seen", C.c_uint32 * TG_COLS * TG_ROWS), ("occ", C.c_uint32 * TG_COLS * TG_ROWS), ("top", C.c_int32 * TG_COLS * TG_ROWS)]


class FrameTreadGrid(C.Structure):
    """ssd_frame_tread_grid: the grids of every surface of a frame"""
    _fields_ = [("n_surfaces", C.c_int32), ("ground", C.c_int32), ("s", TreadGrid * MAX_STEPS)]


MAX_STAIR_MAPS = 64          # SSD_MAX_STAIR_MAPS
STAIR_MAP_NONE = 0xffff      # SSD_STAIR_MAP_NONE: a frame that names no map


class StairMap(C.Structure):
    """ssd_stair_map: a staircase the caller gives, in the external world the cameras share (stairs: a FrameResult, read as
    tread_grid_host reads a result), and the ground flag of its record's header"""
    _fields_ = [("stairs", FrameResult), ("ground", C.c_int32), ("reserved", C.c_int32)]


SP_OBSERVABLE = 3.5e-8       # SSD_SP_OBSERVABLE
SP_MARGIN, SP_BAND, SP_CLEAR, SP_REACH = 0.03, 0.03, 0.03, 0.04   # SSD_SP_*: the defaults of StairPoseRule


class StairPoseRule(C.Structure):
    """ssd_stair_pose_rule: how far inside a tread's sides (margin) and how near its height (band) a tread point lies, how far from the
    treads above and below (clear) and how near the plane under the front edge (reach) a riser point, metres (stair pose, DESIGN.md
    section 7q)"""
    _fields_ = [("margin", C.c_double), ("band", C.c_double), ("clear", C.c_double), ("reach", C.c_double)]

    def __init__(self, margin=SP_MARGIN, band=SP_BAND, clear=SP_CLEAR, reach=SP_REACH):
        super().__init__(float(margin), float(band), float(clear), float(reach))


class StairPoseTarget(C.Structure):
    """ssd_stair_pose_target: the prior the frames are read under and the staircase they are held against"""
    _fields_ = [("prior", Camera), ("map", StairMap)]


class StairPoseMoments(C.Structure):
    """ssd_stair_pose_moments: a frame's points on the map's treads (treads.s[k]) and risers (risers.s[i]: between steps i and i + 1)
    as exact integer moments"""
    _fields_ = [("treads", FrameMoments), ("risers", FrameMoments)]


class StairPose(C.Structure):
    """ssd_stair_pose: one Gauss-Newton step of the camera against the map and the calibration it gives (status != GF_OK: cal is the
    prior, the doubles are 0)"""
    _fields_ = [("status", C.c_int32), ("dof", C.c_int32), ("treads_used", C.c_uint32), ("risers_used", C.c_uint32), ("n", C.c_int64),
                ("n_far", C.c_int64), ("rotation", C.c_double * 3), ("translation", C.c_double * 3), ("centre", C.c_double * 3),
                ("eig", C.c_double * 6), ("rms_before", C.c_double), ("rms_after", C.c_double), ("cal", Calibration)]


FUSE_MAX_FRAMES, FUSE_TOL = 16, 40   # SSD_FUSE_MAX_FRAMES, SSD_FUSE_TOL


class FuseRule(C.Structure):
    """ssd_depth_fuse_rule: how many of a pixel's samples must be valid (min_valid) and agree with their median (min_agree), and how
    far from it, in raw units, a sample may lie to agree (tol)"""
    _fields_ = [("min_valid", C.c_int32), ("min_agree", C.c_int32), ("tol", C.c_int32), ("reserved", C.c_int32)]


class FuseStats(C.Structure):
    """ssd_depth_fuse_stats: a group's record - its pixels by class (they add up to the pixel count), the sum of the valid samples'
    count over all pixels, of the agreeing samples' count over the fused ones, and of their |sample - output| (raw units)"""
    _fields_ = [("n_fused", C.c_int64), ("n_empty", C.c_int64), ("n_few", C.c_int64), ("n_split", C.c_int64), ("sum_valid", C.c_int64),
                ("sum_agree", C.c_int64), ("sum_abs_dev", C.c_int64), ("reserved", C.c_int64)]


EDGE_KEPT, EDGE_EMPTY, EDGE_LONE, EDGE_BRIDGE, EDGE_SLOPE = 0, 1, 2, 3, 0   # SSD_EDGE_*


class EdgeRule(C.Structure):
    """ssd_depth_edge_rule: how many of a pixel's eight neighbours must be near it (min_support; 0: no LONE test), whether a pixel between
    two opposite neighbours in depth goes (bridge), and how far a neighbour may lie to be near: tol + ((d * slope) >> 12) raw units"""
    _fields_ = [("min_support", C.c_int32), ("bridge", C.c_int32), ("tol", C.c_int32), ("slope", C.c_int32)]


class EdgeStats(C.Structure):
    """ssd_depth_edge_stats: a frame's record - its pixels by class (they add up to the pixel count) and the sum of the near neighbours'
    count over the kept ones"""
    _fields_ = [("n_kept", C.c_int64), ("n_empty", C.c_int64), ("n_lone", C.c_int64), ("n_bridge", C.c_int64), ("sum_support", C.c_int64),
                ("reserved", C.c_int64 * 3)]


class WarpView(C.Structure):
    """ssd_depth_warp_view: source camera coordinates -> target camera coordinates (p_dst = r p_src + t, r row-major) and the SOURCE
    frame's intrinsics (depth warp)"""
    _fields_ = [("r", C.c_double * 9), ("t", C.c_double * 3), ("src", Intrinsics), ("reserved", C.c_int32 * 1)]


class WarpStats(C.Structure):
    """ssd_depth_warp_stats: a frame's record - its samples by class (they add up to the pixel count) and the output pixels that are
    not 0 (n_landed - n_filled samples shared a pixel with a nearer one)"""
    _fields_ = [("n_empty", C.c_int64), ("n_behind", C.c_int64), ("n_range", C.c_int64), ("n_outside", C.c_int64), ("n_landed", C.c_int64),
                ("n_filled", C.c_int64), ("reserved", C.c_int64 * 2)]


FILL_KEPT, FILL_EMPTY, FILL_FILLED, FILL_COVERED = 0, 1, 2, 3          # SSD_FILL_*


class FillRule(C.Structure):
    """ssd_depth_fill_rule: how many of a hole's four opposite neighbour pairs must agree for it to be filled (min_pairs), how many
    agreeing pairs must lie more than t in front of a valid pixel for it to be replaced (cover; 0: never), and how far apart a pair's
    two samples may lie to agree: t = tol + ((lo * slope) >> 12) raw units (depth fill)"""
    _fields_ = [("min_pairs", C.c_int32), ("cover", C.c_int32), ("tol", C.c_int32), ("slope", C.c_int32)]


class FillStats(C.Structure):
    """ssd_depth_fill_stats: a frame's record - its pixels by class (they add up to the pixel count), the pairs that made pixels FILLED
    or COVERED, and the spreads hi - lo of the pairs whose middle was written"""
    _fields_ = [("n_kept", C.c_int64), ("n_empty", C.c_int64), ("n_filled", C.c_int64), ("n_covered", C.c_int64), ("sum_pairs", C.c_int64),
                ("sum_spread", C.c_int64), ("reserved", C.c_int64 * 2)]


class Foothold(C.Structure):
    """ssd_foothold: one surface's cells (TG_OUT / TG_FREE / TG_OCCUPIED / TG_UNSEEN) and the best free rectangle on it"""
    _fields_ = [("state", C.c_uint8 * TG_COLS * TG_ROWS), ("n_free", C.c_int32), ("n_occupied", C.c_int32), ("n_unseen", C.c_int32),
                ("foothold", C.c_int32), ("col0", C.c_int32), ("row0", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32),
                ("tallest", C.c_double), ("centre", C.c_double * 2), ("size", C.c_double * 2)]


class FrameFootholds(C.Structure):
    """ssd_frame_footholds: the cells and the foothold of every surface of a frame"""
    _fields_ = [("n_surfaces", C.c_int32), ("ground", C.c_int32), ("s", Foothold * MAX_STEPS)]


MAX_RISERS = MAX_STEPS - 1


class RiserFit(C.Structure):
    """ssd_riser_fit: one riser's plane in external world coordinates (status != GF_OK: the doubles other than rise are 0)"""
    _fields_ = [("status", C.c_int32), ("reserved", C.c_int32), ("n", C.c_int64), ("n_far", C.c_int64), ("normal", C.c_double * 3),
                ("centroid", C.c_double * 3), ("lean", C.c_double), ("skew", C.c_double), ("rms", C.c_double), ("extent", C.c_double * 2),
                ("rise", C.c_double), ("going", C.c_double)]


class FrameRiserFits(C.Structure):
    """ssd_frame_riser_fits: the fitted plane, lean, skew and going of every riser of a frame (riser fit)"""
    _fields_ = [("n_risers", C.c_int32), ("reserved", C.c_int32), ("r", RiserFit * MAX_RISERS)]


class CameraDrift(C.Structure):
    """ssd_camera_drift: a camera's ground moments over the frames of a batch that name it, added exactly, and the ground fit of the
    sum against its table entry (fit.tilt, fit.height_delta: how far the mounting has moved)"""
    _fields_ = [("camera", C.c_int32), ("frames", C.c_int32), ("frames_ground", C.c_int32), ("frames_left", C.c_int32),
                ("m", GroundMoments), ("n_far", C.c_int64), ("fit", GroundFit)]


class CameraFold(C.Structure):
    """ssd_camera_fold: the head of ssd_camera_drift, field for field - what k_camera_fold makes on the device"""
    _fields_ = [("camera", C.c_int32), ("frames", C.c_int32), ("frames_ground", C.c_int32), ("frames_left", C.c_int32),
                ("m", GroundMoments), ("n_far", C.c_int64)]


class Scene(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("cam_height", C.c_double),
                ("axis_right", C.c_double * 3), ("axis_down", C.c_double * 3), ("axis_fwd", C.c_double * 3),
                ("n_steps", C.c_int32),
                ("first_riser_y", C.c_double), ("tread", C.c_double), ("rise", C.c_double),
                ("stair_width", C.c_double), ("landing", C.c_double),
                ("yaw_cos", C.c_double), ("yaw_sin", C.c_double),
                ("sigma", C.c_double),
                ("outlier_frac", C.c_double), ("outlier_min", C.c_double), ("outlier_max", C.c_double),
                ("invalid_frac", C.c_double), ("max_range", C.c_double),
                ("seed", C.c_uint64)]


# libssd_hip.so — the product ABI (include/ssd_hip.h)
EXPORTS = [
    "ssd_default_config", "ssd_calibration_from_points", "ssd_calibration_identity", "ssd_calibration_load",
    "ssd_create", "ssd_destroy", "ssd_last_error", "ssd_workspace_bytes",
    "ssd_process_host", "ssd_enqueue", "ssd_fetch", "ssd_enqueue_stages",
    "ssd_set_intrinsics", "ssd_process_depth_host", "ssd_enqueue_depth", "ssd_deproject_host",
    "ssd_fetch_back", "ssd_stream_wait", "ssd_batches_in_flight", "ssd_set_risers", "ssd_set_single_pass", "ssd_fetch_risers", "ssd_set_timing", "ssd_get_stage_times", "ssd_get_stage_times_back", "ssd_get_predict_time_back", "ssd_serialize",
    "ssd_set_debug", "ssd_get_debug", "ssd_get_debug_image",
    "ssd_device_count", "ssd_device_alloc", "ssd_device_free", "ssd_device_upload", "ssd_device_download",
    "ssd_device_sync", "ssd_host_alloc", "ssd_host_free", "ssd_device_info_get", "ssd_bind_thread_to_device",
    "ssd_pipeline_create", "ssd_pipeline_destroy", "ssd_pipeline_submit", "ssd_pipeline_submit_after", "ssd_pipeline_next", "ssd_pipeline_pending", "ssd_pipeline_set_timing", "ssd_pipeline_stage_times",
    "ssd_pipeline_last_error",
    "ssd_enqueue_labels", "ssd_enqueue_depth_labels", "ssd_process_host_labels", "ssd_process_depth_host_labels", "ssd_get_labels_time_back",
    "ssd_set_cameras", "ssd_camera_count", "ssd_enqueue_cameras", "ssd_process_host_cameras",
    "ssd_calibration_from_plane", "ssd_ground_moments_host", "ssd_ground_fit_solve", "ssd_enqueue_ground_fit", "ssd_fetch_ground_fit",
    "ssd_process_host_ground_fit",
    "ssd_enqueue_surface_moments", "ssd_enqueue_depth_surface_moments", "ssd_get_surface_moments_time_back", "ssd_surface_moments_host",
    "ssd_surface_fit_solve", "ssd_process_host_surfaces",
    "ssd_enqueue_cameras_surface_moments", "ssd_process_host_cameras_surfaces", "ssd_camera_drift_fold",
    "ssd_set_riser_moments", "ssd_fetch_riser_moments", "ssd_riser_fit_solve", "ssd_process_host_riser_fits",
    "ssd_process_host_cameras_riser_fits",
    "ssd_surface_gates_from_moments", "ssd_surface_refit_moments_host", "ssd_enqueue_surface_refit", "ssd_fetch_surface_refit",
    "ssd_get_surface_refit_time", "ssd_process_host_surfaces_refit",
    "ssd_enqueue_cameras_surface_refit", "ssd_process_host_cameras_surfaces_refit", "ssd_camera_ground_gates",
    "ssd_enqueue_surface_gates", "ssd_enqueue_surface_refit_device", "ssd_enqueue_cameras_surface_refit_device",
    "ssd_process_host_surfaces_refit_device", "ssd_process_host_cameras_surfaces_refit_device",
    "ssd_enqueue_camera_fold", "ssd_enqueue_camera_ground_gates", "ssd_enqueue_cameras_surface_refit_folded", "ssd_camera_drift_from_fold",
    "ssd_process_host_cameras_drift",
    "ssd_set_riser_labels", "ssd_get_riser_labels_time_back", "ssd_labels_split",
    "ssd_enqueue_clearance", "ssd_enqueue_cameras_clearance", "ssd_fetch_clearance", "ssd_get_clearance_time", "ssd_clearance_host",
    "ssd_clearance_solve", "ssd_process_host_clearance", "ssd_process_host_cameras_clearance",
    "ssd_enqueue_tread_grid", "ssd_enqueue_cameras_tread_grid", "ssd_fetch_tread_grid", "ssd_get_tread_grid_time", "ssd_tread_grid_host",
    "ssd_tread_grid_solve", "ssd_process_host_tread_grid", "ssd_process_host_cameras_tread_grid",
    "ssd_tread_grid_add", "ssd_stair_map_from_results", "ssd_enqueue_stair_map", "ssd_enqueue_cameras_stair_map", "ssd_fetch_stair_map",
    "ssd_get_stair_map_time", "ssd_process_host_stair_map", "ssd_process_host_cameras_stair_map",
    "ssd_stair_pose_host", "ssd_stair_pose_add", "ssd_stair_pose_solve", "ssd_enqueue_stair_pose", "ssd_fetch_stair_pose_moments",
    "ssd_fetch_stair_pose", "ssd_get_stair_pose_time", "ssd_process_host_stair_pose",
    "ssd_depth_fuse_default_rule", "ssd_depth_fuse_host", "ssd_enqueue_depth_fuse", "ssd_fetch_depth_fuse", "ssd_get_depth_fuse_time",
    "ssd_process_depth_host_fused",
    "ssd_depth_edge_default_rule", "ssd_depth_edges_host", "ssd_enqueue_depth_edges", "ssd_fetch_depth_edges", "ssd_get_depth_edges_time",
    "ssd_process_depth_host_edges",
    "ssd_depth_warp_view_between", "ssd_depth_warp_host", "ssd_enqueue_depth_warp", "ssd_fetch_depth_warp", "ssd_get_depth_warp_time",
    "ssd_process_depth_host_warp_fused",
    "ssd_depth_fill_default_rule", "ssd_depth_fill_host", "ssd_enqueue_depth_fill", "ssd_fetch_depth_fill", "ssd_get_depth_fill_time",
    "ssd_process_depth_host_fill", "ssd_process_depth_host_warp_fill_fused",
]
# libssd_source.so — the frame source standing in for the camera (include/ssd_source.h)
SOURCE_EXPORTS = [
    "ssd_synth_generate_host", "ssd_synth_generate_device", "ssd_synth_depth_host", "ssd_synth_depth_device",
    "ssd_synth_scene_to_camera", "ssd_source_default_scene", "ssd_source_write_calibration", "ssd_source_last_error",
]
# libssd_testhooks.so — test infrastructure (include/ssd_testhooks.h)
HOOK_EXPORTS = [
    "ssd_test_hypot_host", "ssd_test_hypot_device", "ssd_test_frame_state", "ssd_test_ground_image", "ssd_test_line_host", "ssd_test_intersect_host", "ssd_test_quad_device", "ssd_test_quad_host", "ssd_test_closing_host", "ssd_test_best_line_host", "ssd_test_grid_boxes_device", "ssd_test_sort_host",
    "ssd_test_sort_device", "ssd_test_stream_read", "ssd_test_empty_quadrilateral", "ssd_test_single_pass", "ssd_test_plane_pool", "ssd_test_single_pass_stats", "ssd_test_single_pass_frame", "ssd_test_single_pass_sample", "ssd_test_predict_table_host", "ssd_test_predict_sample_host", "ssd_test_prexy_host", "ssd_test_prez_host", "ssd_test_quad_edges_host", "ssd_test_quad_edges_device", "ssd_test_record_offset", "ssd_test_record_realloc", "ssd_test_record_realloc_sized", "ssd_test_record_release", "ssd_testhooks_last_error",
]
SOURCE_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libssd_source.so")
HOOKS_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libssd_testhooks.so")

_lib = None
_source_lib = None
_hooks_lib = None


def lib():
    """Loads libssd_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SsdError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(or make -C stair-step-detector_amd/csrc); there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    L.ssd_last_error.restype = C.c_char_p
    L.ssd_workspace_bytes.restype = sz
    L.ssd_workspace_bytes.argtypes = [vp]
    L.ssd_default_config.argtypes = [C.POINTER(Config), i32, i32]
    L.ssd_calibration_from_points.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(Calibration)]
    L.ssd_calibration_identity.argtypes = [C.POINTER(Calibration)]
    L.ssd_calibration_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Calibration), C.POINTER(C.c_int),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ssd_create.argtypes = [C.POINTER(Config), C.POINTER(Calibration), i32, C.POINTER(vp)]
    L.ssd_destroy.argtypes = [vp]
    L.ssd_process_host.argtypes = [vp, vp, i32, C.POINTER(FrameResult)]
    L.ssd_enqueue.argtypes = [vp, vp, sz, i32, vp]
    L.ssd_enqueue_stages.argtypes = [vp, vp, sz, i32, vp, i32]
    L.ssd_fetch.argtypes = [vp, C.POINTER(FrameResult), i32, vp]
    L.ssd_set_intrinsics.argtypes = [vp, C.POINTER(Intrinsics)]
    L.ssd_process_depth_host.argtypes = [vp, vp, i32, C.POINTER(FrameResult)]
    L.ssd_enqueue_depth.argtypes = [vp, vp, sz, i32, vp]
    L.ssd_deproject_host.argtypes = [C.POINTER(Intrinsics), i32, i32, vp, vp]
    L.ssd_set_timing.argtypes = [vp, i32]
    L.ssd_fetch_back.argtypes = [vp, C.POINTER(FrameResult), i32, i32]
    L.ssd_stream_wait.argtypes = [vp, i32, vp]
    L.ssd_batches_in_flight.argtypes = [vp]
    L.ssd_set_risers.argtypes = [vp, i32, C.c_double, i32]
    L.ssd_set_single_pass.argtypes = [vp, i32]
    L.ssd_fetch_risers.argtypes = [vp, C.POINTER(FrameRisers), i32, vp]
    L.ssd_get_stage_times.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_get_stage_times_back.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.ssd_get_predict_time_back.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.ssd_enqueue_labels.argtypes = [vp, vp, sz, i32, vp, vp, sz]
    L.ssd_enqueue_depth_labels.argtypes = [vp, vp, sz, i32, vp, vp, sz]
    L.ssd_process_host_labels.argtypes = [vp, vp, i32, C.POINTER(FrameResult), vp]
    L.ssd_process_depth_host_labels.argtypes = [vp, vp, i32, C.POINTER(FrameResult), vp]
    L.ssd_get_labels_time_back.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.ssd_set_cameras.argtypes = [vp, C.POINTER(Camera), i32]
    L.ssd_camera_count.argtypes = [vp]
    L.ssd_enqueue_cameras.argtypes = [vp, vp, sz, i32, vp, C.POINTER(C.c_uint16), i32, vp, sz]
    L.ssd_process_host_cameras.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(FrameResult), vp]
    L.ssd_calibration_from_plane.argtypes = [C.POINTER(C.c_double), C.c_double, C.POINTER(Calibration), C.POINTER(Calibration)]
    L.ssd_ground_moments_host.argtypes = [C.POINTER(Config), C.POINTER(Camera), i32, vp, C.c_double, C.POINTER(GroundMoments)]
    L.ssd_ground_fit_solve.argtypes = [C.POINTER(GroundMoments), C.POINTER(Calibration), i32, C.POINTER(GroundFit)]
    L.ssd_enqueue_ground_fit.argtypes = [vp, vp, sz, i32, vp, i32, C.POINTER(Camera), i32, C.c_double]
    L.ssd_fetch_ground_fit.argtypes = [vp, C.POINTER(GroundFit), i32, i32, vp]
    L.ssd_process_host_ground_fit.argtypes = [vp, vp, i32, i32, C.POINTER(Camera), i32, C.c_double, i32, C.POINTER(GroundFit)]
    L.ssd_enqueue_surface_moments.argtypes = [vp, vp, sz, i32, vp, vp]
    L.ssd_enqueue_depth_surface_moments.argtypes = [vp, vp, sz, i32, vp, vp]
    L.ssd_get_surface_moments_time_back.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.ssd_surface_moments_host.argtypes = [C.POINTER(Config), i32, C.POINTER(Intrinsics), vp, vp, i32, i32, C.POINTER(FrameMoments)]
    L.ssd_surface_fit_solve.argtypes = [C.POINTER(FrameMoments), C.POINTER(Calibration), i32, C.POINTER(FrameSurfaces)]
    L.ssd_process_host_surfaces.argtypes = [vp, vp, i32, i32, C.POINTER(FrameResult), C.POINTER(FrameMoments), i32, C.POINTER(FrameSurfaces)]
    L.ssd_enqueue_cameras_surface_moments.argtypes = [vp, vp, sz, i32, vp, C.POINTER(C.c_uint16), i32, vp]
    L.ssd_process_host_cameras_surfaces.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(FrameResult), C.POINTER(FrameMoments), i32,
                                                    C.POINTER(FrameSurfaces)]
    L.ssd_camera_drift_fold.argtypes = [C.POINTER(FrameMoments), C.POINTER(C.c_uint16), i32, C.POINTER(Camera), i32, i32, C.POINTER(CameraDrift)]
    L.ssd_surface_gates_from_moments.argtypes = [C.POINTER(FrameMoments), i32, C.c_double, C.c_double, C.POINTER(FrameGates)]
    L.ssd_surface_refit_moments_host.argtypes = [C.POINTER(Config), i32, C.POINTER(Intrinsics), vp, vp, C.POINTER(FrameGates), i32, i32,
                                                 C.POINTER(FrameMoments)]
    L.ssd_enqueue_surface_refit.argtypes = [vp, vp, sz, i32, vp, i32, C.POINTER(FrameGates), vp]
    L.ssd_fetch_surface_refit.argtypes = [vp, vp]
    L.ssd_get_surface_refit_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_process_host_surfaces_refit.argtypes = [vp, vp, i32, i32, C.POINTER(FrameResult), C.POINTER(FrameMoments), C.POINTER(FrameMoments), i32,
                                                  C.c_double, C.c_double, i32, C.POINTER(FrameSurfaces)]
    L.ssd_enqueue_cameras_surface_refit.argtypes = [vp, vp, sz, i32, vp, i32, C.POINTER(FrameGates), vp]
    L.ssd_process_host_cameras_surfaces_refit.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(FrameResult), C.POINTER(FrameMoments),
                                                          C.POINTER(FrameMoments), i32, C.c_double, C.c_double, i32, C.POINTER(FrameSurfaces)]
    L.ssd_enqueue_surface_gates.argtypes = [vp, vp, i32, vp, i32, C.c_double, C.c_double, vp]
    L.ssd_enqueue_surface_refit_device.argtypes = [vp, vp, sz, i32, vp, i32, vp, i32, C.c_double, C.c_double, vp]
    L.ssd_enqueue_cameras_surface_refit_device.argtypes = L.ssd_enqueue_surface_refit_device.argtypes
    L.ssd_process_host_surfaces_refit_device.argtypes = L.ssd_process_host_surfaces_refit.argtypes
    L.ssd_process_host_cameras_surfaces_refit_device.argtypes = L.ssd_process_host_cameras_surfaces_refit.argtypes
    L.ssd_camera_ground_gates.argtypes = [C.POINTER(FrameMoments), C.POINTER(C.c_uint16), i32, C.POINTER(CameraDrift), i32, C.c_double, C.c_double,
                                          C.POINTER(FrameGates)]
    L.ssd_enqueue_camera_fold.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.ssd_enqueue_camera_ground_gates.argtypes = [vp, vp, vp, i32, vp, i32, i32, C.c_double, C.c_double, vp, vp]
    L.ssd_enqueue_clearance.argtypes = [vp, vp, sz, i32, vp, i32, C.POINTER(ClearanceRule), vp, vp, sz]
    L.ssd_enqueue_cameras_clearance.argtypes = L.ssd_enqueue_clearance.argtypes
    L.ssd_fetch_clearance.argtypes = [vp, vp]
    L.ssd_get_clearance_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_clearance_host.argtypes = [C.POINTER(Config), C.POINTER(Calibration), i32, C.POINTER(Intrinsics), vp, C.POINTER(FrameResult), i32,
                                     C.POINTER(ClearanceRule), C.POINTER(FrameMoments), vp]
    L.ssd_clearance_solve.argtypes = [C.POINTER(FrameMoments), C.POINTER(FrameResult), C.POINTER(Calibration), i32, C.POINTER(FrameClearance)]
    L.ssd_process_host_clearance.argtypes = [vp, vp, i32, i32, C.POINTER(ClearanceRule), i32, C.POINTER(FrameResult), C.POINTER(FrameMoments), vp,
                                             C.POINTER(FrameClearance)]
    L.ssd_process_host_cameras_clearance.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(ClearanceRule), i32, C.POINTER(FrameResult),
                                                     C.POINTER(FrameMoments), vp, C.POINTER(FrameClearance)]
    L.ssd_enqueue_tread_grid.argtypes = [vp, vp, sz, i32, vp, i32, C.POINTER(TreadGridRule), vp]
    L.ssd_enqueue_cameras_tread_grid.argtypes = L.ssd_enqueue_tread_grid.argtypes
    L.ssd_fetch_tread_grid.argtypes = [vp, vp]
    L.ssd_get_tread_grid_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_tread_grid_host.argtypes = [C.POINTER(Config), C.POINTER(Calibration), i32, C.POINTER(Intrinsics), vp, C.POINTER(FrameResult), i32,
                                      C.POINTER(TreadGridRule), C.POINTER(FrameTreadGrid)]
    L.ssd_tread_grid_solve.argtypes = [C.POINTER(FrameTreadGrid), C.POINTER(FrameResult), C.POINTER(TreadGridRule), i32, i32, C.c_double, C.c_double,
                                       C.POINTER(FrameFootholds)]
    L.ssd_process_host_tread_grid.argtypes = [vp, vp, i32, i32, C.POINTER(TreadGridRule), i32, i32, C.c_double, C.c_double, C.POINTER(FrameResult),
                                              C.POINTER(FrameTreadGrid), C.POINTER(FrameFootholds)]
    L.ssd_process_host_cameras_tread_grid.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(TreadGridRule), i32, i32, C.c_double, C.c_double,
                                                      C.POINTER(FrameResult), C.POINTER(FrameTreadGrid), C.POINTER(FrameFootholds)]
    L.ssd_tread_grid_add.argtypes = [C.POINTER(FrameTreadGrid), C.POINTER(FrameTreadGrid)]
    L.ssd_stair_map_from_results.argtypes = [C.POINTER(FrameResult), i32, i32, C.POINTER(StairMap), C.POINTER(i32)]
    L.ssd_enqueue_stair_map.argtypes = [vp, vp, sz, i32, vp, i32, C.POINTER(StairMap), i32, C.POINTER(C.c_uint16), C.POINTER(TreadGridRule), i32, vp]
    L.ssd_enqueue_cameras_stair_map.argtypes = L.ssd_enqueue_stair_map.argtypes
    L.ssd_fetch_stair_map.argtypes = [vp, vp]
    L.ssd_get_stair_map_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_process_host_stair_map.argtypes = [vp, vp, i32, i32, C.POINTER(StairMap), i32, C.POINTER(C.c_uint16), C.POINTER(TreadGridRule), i32, i32,
                                             C.c_double, C.c_double, C.POINTER(FrameResult), C.POINTER(FrameTreadGrid), C.POINTER(FrameFootholds)]
    L.ssd_process_host_cameras_stair_map.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(StairMap), i32, C.POINTER(C.c_uint16),
                                                     C.POINTER(TreadGridRule), i32, i32, C.c_double, C.c_double, C.POINTER(FrameResult),
                                                     C.POINTER(FrameTreadGrid), C.POINTER(FrameFootholds)]
    L.ssd_stair_pose_host.argtypes = [C.POINTER(Config), C.POINTER(StairPoseTarget), i32, vp, C.POINTER(StairPoseRule), C.POINTER(StairPoseMoments)]
    L.ssd_stair_pose_add.argtypes = [C.POINTER(StairPoseMoments), C.POINTER(StairPoseMoments)]
    L.ssd_stair_pose_solve.argtypes = [C.POINTER(StairPoseMoments), C.POINTER(StairPoseTarget), i32, C.c_double, C.POINTER(StairPose)]
    L.ssd_enqueue_stair_pose.argtypes = [vp, vp, sz, i32, vp, i32, C.POINTER(StairPoseTarget), i32, C.POINTER(C.c_uint16), C.POINTER(StairPoseRule)]
    L.ssd_fetch_stair_pose_moments.argtypes = [vp, C.POINTER(StairPoseMoments), i32, vp]
    L.ssd_fetch_stair_pose.argtypes = [vp, C.POINTER(StairPose), i32, C.c_double, vp]
    L.ssd_get_stair_pose_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_depth_fuse_default_rule.argtypes = [i32, C.POINTER(FuseRule)]
    L.ssd_depth_fuse_host.argtypes = [i32, i32, vp, sz, i32, C.POINTER(FuseRule), vp, vp, C.POINTER(FuseStats)]
    L.ssd_enqueue_depth_fuse.argtypes = [vp, vp, sz, i32, vp, i32, i32, C.POINTER(FuseRule), vp, sz, vp, sz]
    L.ssd_fetch_depth_fuse.argtypes = [vp, C.POINTER(FuseStats), i32, vp]
    L.ssd_get_depth_fuse_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_process_depth_host_fused.argtypes = [vp, vp, i32, i32, C.POINTER(FuseRule), C.POINTER(FrameResult), vp, C.POINTER(FuseStats)]
    L.ssd_depth_edge_default_rule.argtypes = [C.POINTER(EdgeRule)]
    L.ssd_depth_edges_host.argtypes = [i32, i32, vp, C.POINTER(EdgeRule), vp, vp, C.POINTER(EdgeStats)]
    L.ssd_enqueue_depth_edges.argtypes = [vp, vp, sz, i32, vp, C.POINTER(EdgeRule), vp, sz, vp, sz]
    L.ssd_fetch_depth_edges.argtypes = [vp, C.POINTER(EdgeStats), i32, vp]
    L.ssd_get_depth_edges_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_process_depth_host_edges.argtypes = [vp, vp, i32, C.POINTER(EdgeRule), C.POINTER(FrameResult), vp, C.POINTER(EdgeStats)]
    L.ssd_depth_warp_view_between.argtypes = [C.POINTER(Camera), C.POINTER(Camera), C.POINTER(WarpView)]
    L.ssd_depth_warp_host.argtypes = [i32, i32, vp, C.POINTER(WarpView), C.POINTER(Intrinsics), vp, C.POINTER(WarpStats)]
    L.ssd_enqueue_depth_warp.argtypes = [vp, vp, sz, i32, vp, C.POINTER(WarpView), C.POINTER(Intrinsics), vp, sz]
    L.ssd_fetch_depth_warp.argtypes = [vp, C.POINTER(WarpStats), i32, vp]
    L.ssd_get_depth_warp_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_process_depth_host_warp_fused.argtypes = [vp, vp, i32, i32, C.POINTER(WarpView), C.POINTER(Intrinsics), C.POINTER(FuseRule),
                                                    C.POINTER(FrameResult), vp, C.POINTER(WarpStats), C.POINTER(FuseStats)]
    L.ssd_depth_fill_default_rule.argtypes = [C.POINTER(FillRule)]
    L.ssd_depth_fill_host.argtypes = [i32, i32, vp, C.POINTER(FillRule), vp, vp, C.POINTER(FillStats)]
    L.ssd_enqueue_depth_fill.argtypes = [vp, vp, sz, i32, vp, C.POINTER(FillRule), vp, sz, vp, sz]
    L.ssd_fetch_depth_fill.argtypes = [vp, C.POINTER(FillStats), i32, vp]
    L.ssd_get_depth_fill_time.argtypes = [vp, C.POINTER(C.c_float)]
    L.ssd_process_depth_host_fill.argtypes = [vp, vp, i32, C.POINTER(FillRule), C.POINTER(FrameResult), vp, C.POINTER(FillStats)]
    L.ssd_process_depth_host_warp_fill_fused.argtypes = [vp, vp, i32, i32, C.POINTER(WarpView), C.POINTER(Intrinsics), C.POINTER(FillRule),
                                                         C.POINTER(FuseRule), C.POINTER(FrameResult), vp, C.POINTER(WarpStats),
                                                         C.POINTER(FillStats), C.POINTER(FuseStats)]
    L.ssd_process_host_stair_pose.argtypes = [vp, vp, i32, i32, C.POINTER(StairPoseTarget), i32, C.POINTER(C.c_uint16), C.POINTER(StairPoseRule), i32,
                                              C.c_double, C.POINTER(StairPoseMoments), C.POINTER(StairPose)]
    L.ssd_enqueue_cameras_surface_refit_folded.argtypes = [vp, vp, sz, i32, vp, i32, vp, i32, C.c_double, C.c_double, i32, vp]
    L.ssd_camera_drift_from_fold.argtypes = [C.POINTER(CameraFold), C.POINTER(Camera), i32, i32, C.POINTER(CameraDrift)]
    L.ssd_process_host_cameras_drift.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(FrameResult), i32, C.c_double, C.c_double, i32, i32,
                                                 C.POINTER(CameraDrift)]
    L.ssd_set_riser_moments.argtypes = [vp, i32]
    L.ssd_fetch_riser_moments.argtypes = [vp, C.POINTER(FrameMoments), i32, vp]
    L.ssd_set_riser_labels.argtypes = [vp, i32]
    L.ssd_get_riser_labels_time_back.argtypes = [vp, i32, C.POINTER(C.c_float)]
    L.ssd_labels_split.argtypes = [vp, sz, vp, vp]
    L.ssd_riser_fit_solve.argtypes = [C.POINTER(FrameMoments), C.POINTER(FrameRisers), C.POINTER(Calibration), i32, C.POINTER(FrameRiserFits)]
    L.ssd_process_host_riser_fits.argtypes = [vp, vp, i32, i32, C.POINTER(FrameResult), C.POINTER(FrameRisers), C.POINTER(FrameMoments), i32,
                                              C.POINTER(FrameRiserFits)]
    L.ssd_process_host_cameras_riser_fits.argtypes = [vp, vp, i32, C.POINTER(C.c_uint16), i32, C.POINTER(FrameResult), C.POINTER(FrameRisers),
                                                      C.POINTER(FrameMoments), i32, C.POINTER(FrameRiserFits)]
    L.ssd_serialize.argtypes = [C.POINTER(FrameResult), C.c_char_p, sz]
    L.ssd_set_debug.argtypes = [vp, i32]
    L.ssd_get_debug.argtypes = [vp, i32, C.POINTER(DebugFrame)]
    L.ssd_get_debug_image.argtypes = [vp, i32, i32, i32, vp]
    L.ssd_device_alloc.argtypes = [i32, sz, C.POINTER(vp)]
    L.ssd_device_free.argtypes = [i32, vp]
    L.ssd_device_upload.argtypes = [i32, vp, vp, sz]
    L.ssd_device_download.argtypes = [i32, vp, vp, sz]
    L.ssd_device_sync.argtypes = [i32]
    L.ssd_host_alloc.argtypes = [sz, C.POINTER(vp)]
    L.ssd_device_info_get.argtypes = [i32, C.POINTER(DeviceInfo)]
    L.ssd_bind_thread_to_device.argtypes = [i32]
    L.ssd_host_free.argtypes = [vp]
    L.ssd_pipeline_create.argtypes = [C.POINTER(Config), C.POINTER(Calibration), i32, i32, C.POINTER(vp)]
    L.ssd_pipeline_destroy.argtypes = [vp]
    L.ssd_pipeline_submit.argtypes = [vp, vp, sz, i32]
    L.ssd_pipeline_submit_after.argtypes = [vp, vp, sz, i32, vp, i32]
    L.ssd_pipeline_next.argtypes = [vp, C.POINTER(FrameResult), i32, C.POINTER(i32)]
    L.ssd_pipeline_pending.argtypes = [vp]
    L.ssd_pipeline_set_timing.argtypes = [vp, i32]
    L.ssd_pipeline_stage_times.argtypes = [vp, vp]
    L.ssd_pipeline_last_error.restype = C.c_char_p
    _lib = L
    return L


def source_lib():
    """Loads libssd_source.so (the synthetic frame source: tests, bench, driver); raises if it has not been built."""
    global _source_lib
    if _source_lib is not None:
        return _source_lib
    if not os.path.exists(SOURCE_LIB_PATH):
        raise SsdError("%s is missing: build it with make -C stair-step-detector_amd/csrc" % SOURCE_LIB_PATH)
    L = C.CDLL(SOURCE_LIB_PATH)
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    L.ssd_source_last_error.restype = C.c_char_p
    L.ssd_synth_depth_host.argtypes = [C.POINTER(Scene), i32, C.c_float, vp]
    L.ssd_synth_depth_device.argtypes = [C.POINTER(Scene), i32, C.c_float, vp, sz, i32, vp]
    L.ssd_synth_generate_host.argtypes = [C.POINTER(Scene), i32, vp]
    L.ssd_synth_generate_device.argtypes = [C.POINTER(Scene), i32, vp, sz, i32, vp]
    L.ssd_synth_scene_to_camera.argtypes = [C.POINTER(Scene), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.ssd_source_default_scene.argtypes = [C.POINTER(Scene), i32, i32, i32, C.c_uint64]
    L.ssd_source_write_calibration.argtypes = [C.POINTER(Scene), C.POINTER(C.c_double), C.c_char_p]
    _source_lib = L
    return L


def hooks_lib():
    """Loads libssd_testhooks.so (test infrastructure, not part of the product ABI)."""
    global _hooks_lib
    if _hooks_lib is not None:
        return _hooks_lib
    if not os.path.exists(HOOKS_LIB_PATH):
        raise SsdError("%s is missing: build it with make -C stair-step-detector_amd/csrc" % HOOKS_LIB_PATH)
    lib()                                           # the hooks take handles of the product library
    L = C.CDLL(HOOKS_LIB_PATH)
    vp, i32 = C.c_void_p, C.c_int
    L.ssd_testhooks_last_error.restype = C.c_char_p
    L.ssd_test_hypot_host.restype = C.c_double
    L.ssd_test_hypot_host.argtypes = [C.c_double, C.c_double]
    L.ssd_test_hypot_device.argtypes = [i32, vp, vp, vp, i32]
    L.ssd_test_closing_host.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32]
    L.ssd_test_closing_host.restype = i32
    L.ssd_test_best_line_host.argtypes = [vp, i32, i32, vp]
    L.ssd_test_best_line_host.restype = i32
    L.ssd_test_quad_host.argtypes = [vp, vp, i32, vp, vp]
    L.ssd_test_quad_host.restype = i32
    L.ssd_test_frame_state.argtypes = [vp, i32, vp, C.c_size_t, vp]
    L.ssd_test_frame_state.restype = C.c_longlong
    L.ssd_test_ground_image.argtypes = [vp, i32, vp]
    L.ssd_test_empty_quadrilateral.argtypes = [vp, i32, i32]
    L.ssd_test_single_pass.argtypes = [vp, i32, i32]
    L.ssd_test_plane_pool.argtypes = [vp, i32]
    L.ssd_test_single_pass_stats.argtypes = [vp, i32, i32, vp]
    L.ssd_test_single_pass_frame.argtypes = [vp, i32, vp, vp]
    L.ssd_test_single_pass_sample.argtypes = [vp, i32, vp]
    L.ssd_test_predict_table_host.argtypes = [vp, i32, i32, i32, vp]
    L.ssd_test_predict_sample_host.argtypes = [C.c_ulonglong, i32, vp, vp, i32]
    L.ssd_test_prexy_host.argtypes = [vp, vp, vp, vp]
    L.ssd_test_prez_host.argtypes = [vp, vp, vp, C.c_double, i32, i32, vp]
    L.ssd_test_quad_edges_host.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.ssd_test_quad_edges_host.restype = i32
    L.ssd_test_quad_edges_device.argtypes = [i32, vp, i32, vp, vp]
    L.ssd_test_quad_edges_device.restype = i32
    L.ssd_test_record_offset.argtypes = [vp, C.c_size_t]
    L.ssd_test_record_realloc.argtypes = [vp]
    L.ssd_test_record_realloc.restype = C.c_ulonglong
    L.ssd_test_record_realloc_sized.argtypes = [vp, C.c_size_t, C.c_size_t]
    L.ssd_test_record_realloc_sized.restype = C.c_ulonglong
    L.ssd_test_line_host.argtypes = [vp, vp, vp]
    L.ssd_test_intersect_host.argtypes = [vp, vp, vp]
    L.ssd_test_sort_host.argtypes = [vp, i32, vp]
    L.ssd_test_sort_device.argtypes = [i32, vp, i32, vp]
    L.ssd_test_quad_device.argtypes = [i32, vp, vp, i32, vp, C.POINTER(C.c_int)]
    L.ssd_test_grid_boxes_device.argtypes = [i32, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp, i32, vp, C.POINTER(C.c_int)]
    L.ssd_test_stream_read.argtypes = [i32, vp, C.c_size_t, i32, vp, C.POINTER(C.c_float)]
    _hooks_lib = L
    return L


def _check(rc, which="hip"):
    if rc < 0:
        msg = {"hip": lambda: lib().ssd_last_error(), "source": lambda: source_lib().ssd_source_last_error(),
               "hooks": lambda: hooks_lib().ssd_testhooks_last_error()}[which]().decode()
        raise SsdError("libssd_%s error %d: %s" % (which, rc, msg))
    return rc


def _input_code(depth):
    """the `input` argument of the C entry points: 16-bit depth, or vertices"""
    return INPUT_DEPTH16 if depth else INPUT_VERTICES


def _time_ms(getter, *args):
    """a time getter of the C API (its last argument a float *) -> milliseconds"""
    ms = C.c_float(0.0)
    _check(getter(*args, C.byref(ms)))
    return float(ms.value)


def predict_table_host(sample, n_bins, min_height, sabotage=0):
    """test hook (host, no GPU): the single pass's bin -> plane table as csrc/ssd_predict.h states it; returns (uint8[MAX_BINS], planes)"""
    a = np.ascontiguousarray(sample, dtype=np.uint32)
    assert a.size == MAX_BINS
    out = np.zeros(MAX_BINS, dtype=np.uint8)
    n = _check(hooks_lib().ssd_test_predict_table_host(a.ctypes.data_as(C.c_void_p), n_bins, min_height, sabotage, out.ctypes.data_as(C.c_void_p)), "hooks")
    return out, n


def predict_sample_host(base_address, n_points):
    """test hook (host, no GPU): k_predict's sample of a vertex frame of n_points points whose first byte lies at base_address, as
    csrc/ssd_predict.h states it; returns (first, count), int32 arrays with an entry per group of lines: the sampled points of
    group g are first[g] .. first[g] + count[g] - 1"""
    groups = _check(hooks_lib().ssd_test_predict_sample_host(int(base_address), int(n_points), None, None, 0), "hooks")
    first, count = np.zeros(groups, dtype=np.int32), np.zeros(groups, dtype=np.int32)
    _check(hooks_lib().ssd_test_predict_sample_host(int(base_address), int(n_points), first.ctypes.data_as(C.c_void_p),
                                                    count.ctypes.data_as(C.c_void_p), groups), "hooks")
    return first, count


def device_info(device):
    """{'pci_bus_id', 'uuid', 'numa_node', 'n_local_cpus', 'cpu_list'} of a device index (ssd_device_info_get)"""
    info = DeviceInfo()
    _check(lib().ssd_device_info_get(device, C.byref(info)))
    return {"pci_bus_id": info.pci_bus_id.decode(), "uuid": info.uuid.decode(), "numa_node": int(info.numa_node),
            "n_local_cpus": int(info.n_local_cpus), "cpu_list": info.cpu_list.decode()}


def bind_thread_to_device(device):
    """the calling thread onto the CPUs of the device's NUMA node; returns how many (0 = the platform names none)"""
    n = lib().ssd_bind_thread_to_device(device)
    if n < 0:
        _check(n)
    return n


def device_count():
    return lib().ssd_device_count()


def default_config(width, height, max_frames_per_batch=64, max_step_plateaus=MAX_STEP_IMAGES, batches_in_flight=0):
    """batches_in_flight: workspaces of the handle (ssd_config); 0 = 1 = strict stream order; overlap is opt-in
    (BATCHES_IN_FLIGHT_THROUGHPUT = 3 for callers that enqueue ahead of their fetches and leave the frames alone meanwhile)"""
    cfg = Config()
    _check(lib().ssd_default_config(C.byref(cfg), width, height))
    cfg.max_frames_per_batch = max_frames_per_batch
    cfg.max_step_plateaus = max_step_plateaus
    cfg.batches_in_flight = batches_in_flight
    return cfg


# --------------------------------------------------------------------------- ground fit: host functions (no GPU needed)
def _as_camera(prior, intr=None):
    """a Camera from a Camera, GeometricTransformation, Calibration or (either, Intrinsics)"""
    if isinstance(prior, Camera):
        return prior
    if isinstance(prior, (tuple, list)):
        prior, intr = prior
    cam = Camera()
    cam.cal = prior.constants if isinstance(prior, GeometricTransformation) else prior
    if intr is not None:
        cam.intr = intr
        cam.has_intrinsics = 1
    return cam


def _camera_array(priors):
    """(ctypes array of Camera or None, count) from None, one prior or a list of priors"""
    if priors is None:
        return None, 0
    if not isinstance(priors, (list, tuple)) or (len(priors) == 2 and isinstance(priors[1], Intrinsics)):
        priors = [priors]
    arr = (Camera * max(1, len(priors)))()
    for i, p in enumerate(priors):
        arr[i] = _as_camera(p)
    return arr, len(priors)


def calibration_from_plane(normal, dist, prior):
    """ssd_calibration_from_plane: CameraToWorld from the floor's plane (unit normal away from the camera, camera height), the rest of
    the calibration copied from `prior` -> Calibration"""
    n0 = (C.c_double * 3)(*[float(v) for v in normal])
    p = prior.constants if isinstance(prior, GeometricTransformation) else prior
    out = Calibration()
    _check(lib().ssd_calibration_from_plane(n0, float(dist), C.byref(p), C.byref(out)))
    return out


def ground_moments_host(cfg, prior, frame, tol, depth=False):
    """ssd_ground_moments_host: one frame's floor points under `prior` (a Camera, or anything Detector.set_cameras takes) as exact
    integer moments -> GroundMoments.  frame: float32 [H, W, 3], or uint16 [H, W] with depth=True."""
    a = np.ascontiguousarray(frame, dtype=np.uint16 if depth else np.float32)
    if a.size != cfg.width * cfg.height * (1 if depth else 3):
        raise SsdError("ground_moments_host: the array is not one frame")
    cam = _as_camera(prior)
    out = GroundMoments()
    _check(lib().ssd_ground_moments_host(C.byref(cfg), C.byref(cam), _input_code(depth), a.ctypes.data_as(C.c_void_p),
                                         float(tol), C.byref(out)))
    return out


def ground_fit_solve(moments, prior, min_points=2000):
    """ssd_ground_fit_solve: moments -> plane -> refined calibration (GroundFit; status GF_OK / GF_FEW / GF_DEGENERATE)"""
    p = prior.constants if isinstance(prior, GeometricTransformation) else prior.cal if isinstance(prior, Camera) else prior
    out = GroundFit()
    _check(lib().ssd_ground_fit_solve(C.byref(moments), C.byref(p), int(min_points), C.byref(out)))
    return out


# --------------------------------------------------------------------------- surface fit: host functions (no GPU needed)
def surface_moments_host(cfg, frame, labels, n_surfaces, ground, intr=None):
    """ssd_surface_moments_host: one frame's per-surface sums from its labels (uint8 [H, W], label k + 1 = surface k) -> FrameMoments.
    frame: float32 [H, W, 3], or uint16 [H, W] with intr (an Intrinsics: 16-bit depth input)."""
    depth = intr is not None
    a = np.ascontiguousarray(frame, dtype=np.uint16 if depth else np.float32)
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    if a.size != cfg.width * cfg.height * (1 if depth else 3) or lab.size != cfg.width * cfg.height:
        raise SsdError("surface_moments_host: the arrays are not one frame")
    out = FrameMoments()
    _check(lib().ssd_surface_moments_host(C.byref(cfg), _input_code(depth), C.byref(intr) if depth else None,
                                          a.ctypes.data_as(C.c_void_p), lab.ctypes.data_as(C.c_void_p), int(n_surfaces), int(ground), C.byref(out)))
    return out


def labels_split(labels):
    """ssd_labels_split: a label mask with riser labels (Detector.set_riser_labels) -> (surfaces, risers), uint8 arrays of its shape:
    surfaces keeps the labels 0 .. MAX_STEPS, risers holds i + 1 where the label is LABEL_RISER_BASE + i; each is in the form
    surface_moments_host accepts.  A label in neither range raises SsdError."""
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    surfaces, risers = np.empty_like(lab), np.empty_like(lab)
    _check(lib().ssd_labels_split(lab.ctypes.data_as(C.c_void_p), lab.size, surfaces.ctypes.data_as(C.c_void_p), risers.ctypes.data_as(C.c_void_p)))
    return surfaces, risers


def surface_fit_solve(moments, cal, min_points=200):
    """ssd_surface_fit_solve: a frame's moments -> a plane per surface (FrameSurfaces; per surface GF_OK / GF_FEW / GF_DEGENERATE)"""
    c = cal.constants if isinstance(cal, GeometricTransformation) else cal.cal if isinstance(cal, Camera) else cal
    out = FrameSurfaces()
    _check(lib().ssd_surface_fit_solve(C.byref(moments), C.byref(c), int(min_points), C.byref(out)))
    return out


def surface_gates_from_moments(moments, min_points=200, k_sigma=2.5, gate_min=0.0):
    """ssd_surface_gates_from_moments: a frame's moments -> a gate per surface (FrameGates): the fitted plane in camera coordinates
    and max(k_sigma * rms, gate_min); gate 0 for a surface whose fit is not GF_OK"""
    out = FrameGates()
    _check(lib().ssd_surface_gates_from_moments(C.byref(moments) if moments is not None else None, int(min_points), float(k_sigma),
                                                float(gate_min), C.byref(out)))
    return out


def surface_refit_moments_host(cfg, frame, labels, gates, n_surfaces, ground, intr=None):
    """ssd_surface_refit_moments_host: surface_moments_host over the labelled points inside their surface's gate -> FrameMoments"""
    depth = intr is not None
    a = np.ascontiguousarray(frame, dtype=np.uint16 if depth else np.float32)
    lab = np.ascontiguousarray(labels, dtype=np.uint8)
    if a.size != cfg.width * cfg.height * (1 if depth else 3) or lab.size != cfg.width * cfg.height:
        raise SsdError("surface_refit_moments_host: the arrays are not one frame")
    out = FrameMoments()
    _check(lib().ssd_surface_refit_moments_host(C.byref(cfg), _input_code(depth), C.byref(intr) if depth else None,
                                                a.ctypes.data_as(C.c_void_p), lab.ctypes.data_as(C.c_void_p),
                                                C.byref(gates) if gates is not None else None, int(n_surfaces), int(ground), C.byref(out)))
    return out


def _calibration_of(cal):
    return cal.constants if isinstance(cal, GeometricTransformation) else cal.cal if isinstance(cal, Camera) else cal


def clearance_host(cfg, cal, frame, result, ground, rule=None, intr=None, mask=True):
    """ssd_clearance_host: one frame's occupants by the rule of DESIGN.md section 7m -> (FrameMoments, uint8 [H, W] mask with k + 1 on an
    occupant of surface k; None with mask=False).  frame: float32 [H, W, 3], or uint16 [H, W] with intr (16-bit depth input)."""
    depth = intr is not None
    a = np.ascontiguousarray(frame, dtype=np.uint16 if depth else np.float32)
    if a.size != cfg.width * cfg.height * (1 if depth else 3):
        raise SsdError("clearance_host: the array is not one frame")
    rule = ClearanceRule() if rule is None else rule
    c = _calibration_of(cal)
    out = FrameMoments()
    m = np.empty((cfg.height, cfg.width), dtype=np.uint8) if mask else None
    _check(lib().ssd_clearance_host(C.byref(cfg), C.byref(c), _input_code(depth), C.byref(intr) if depth else None,
                                    a.ctypes.data_as(C.c_void_p), C.byref(result), int(ground), C.byref(rule), C.byref(out),
                                    m.ctypes.data_as(C.c_void_p) if mask else None))
    return out, m


def clearance_solve(moments, result, cal, min_support=50):
    """ssd_clearance_solve: a frame's clearance moments -> what stands on each surface (FrameClearance; per surface CL_FREE / CL_OCCUPIED)"""
    c = _calibration_of(cal)
    out = FrameClearance()
    _check(lib().ssd_clearance_solve(C.byref(moments), C.byref(result), C.byref(c), int(min_support), C.byref(out)))
    return out


def tread_grid_host(cfg, cal, frame, result, ground, rule=None, intr=None):
    """ssd_tread_grid_host: one frame's grids by the rule of DESIGN.md section 7n -> FrameTreadGrid.  frame: float32 [H, W, 3], or
    uint16 [H, W] with intr (16-bit depth input)."""
    depth = intr is not None
    a = np.ascontiguousarray(frame, dtype=np.uint16 if depth else np.float32)
    if a.size != cfg.width * cfg.height * (1 if depth else 3):
        raise SsdError("tread_grid_host: the array is not one frame")
    rule = TreadGridRule() if rule is None else rule
    c = _calibration_of(cal)
    out = FrameTreadGrid()
    _check(lib().ssd_tread_grid_host(C.byref(cfg), C.byref(c), _input_code(depth), C.byref(intr) if depth else None,
                                     a.ctypes.data_as(C.c_void_p), C.byref(result), int(ground), C.byref(rule), C.byref(out)))
    return out


def tread_grid_solve(grid, result, rule=None, min_seen=1, min_occ=1, foot_along=0.0, foot_deep=0.0):
    """ssd_tread_grid_solve: a frame's grids -> every cell's state and the best free rectangle per surface (FrameFootholds)"""
    rule = TreadGridRule() if rule is None else rule
    out = FrameFootholds()
    _check(lib().ssd_tread_grid_solve(C.byref(grid), C.byref(result), C.byref(rule), int(min_seen), int(min_occ), float(foot_along),
                                      float(foot_deep), C.byref(out)))
    return out


def tread_grid_add(grid, acc):
    """ssd_tread_grid_add: the stair map's fold step - acc's header becomes grid's, grid's counts are added to acc's, acc's tops raised to
    grid's; SsdError (SSD_E_CAP) and acc untouched if a count would pass 2^32 - 1.  Returns acc."""
    _check(lib().ssd_tread_grid_add(C.byref(grid) if grid is not None else None, C.byref(acc) if acc is not None else None))
    return acc


def _stair_maps(maps):
    """one StairMap, a FrameResult (ground flag 1) or a sequence of either -> (StairMap array, count)"""
    if isinstance(maps, (StairMap, FrameResult)):
        maps = [maps]
    maps = list(maps)
    arr = (StairMap * max(len(maps), 1))()
    for i, m in enumerate(maps):
        if isinstance(m, FrameResult):
            C.memmove(C.byref(arr[i].stairs), C.byref(m), C.sizeof(FrameResult))
            arr[i].ground = 1
        else:
            C.memmove(C.byref(arr[i]), C.byref(m), C.sizeof(StairMap))
    return arr, len(maps)


def _map_index(map_of_frame, nframes):
    if map_of_frame is None:
        return None
    idx = np.ascontiguousarray(map_of_frame, dtype=np.uint16)
    if idx.ndim != 1 or idx.size != nframes or np.any(np.asarray(map_of_frame) != idx):
        raise SsdError("map_of_frame: one index 0..65535 per frame")
    return idx


def stair_map_from_results(results, ground=1):
    """ssd_stair_map_from_results: a reference staircase from a run of FrameResults - per step the lower median of the height and of each
    quadrilateral coordinate over the usable frames with the most frequent n_steps -> (StairMap, frames used)"""
    results = list(results)
    arr = (FrameResult * max(len(results), 1))(*results)
    out, used = StairMap(), C.c_int32(0)
    _check(lib().ssd_stair_map_from_results(arr, len(results), int(ground), C.byref(out), C.byref(used)))
    return out, int(used.value)


# --------------------------------------------------------------------------- stair pose: host functions (no GPU needed)
def stair_pose_target(prior, stair_map, intr=None):
    """a StairPoseTarget from a prior (a Camera, or anything Detector.set_cameras takes) and a StairMap or FrameResult (ground flag 1)"""
    if isinstance(prior, StairPoseTarget):
        return prior
    t = StairPoseTarget()
    t.prior = _as_camera(prior, intr)
    t.map = _stair_maps(stair_map)[0][0]
    return t


def _pose_targets(targets):
    """one StairPoseTarget, one (prior, map) pair or a sequence of either -> (StairPoseTarget array, count)"""
    if isinstance(targets, StairPoseTarget) or (isinstance(targets, tuple) and len(targets) == 2 and isinstance(targets[1], (StairMap, FrameResult))):
        targets = [targets]
    targets = [t if isinstance(t, StairPoseTarget) else stair_pose_target(*t) for t in targets]
    arr = (StairPoseTarget * max(len(targets), 1))()
    for i, t in enumerate(targets):
        C.memmove(C.byref(arr[i]), C.byref(t), C.sizeof(StairPoseTarget))
    return arr, len(targets)


def stair_pose_host(cfg, target, frame, rule=None, depth=False):
    """ssd_stair_pose_host: one frame's points on the target's treads and risers -> StairPoseMoments.  frame: float32 [H, W, 3], or
    uint16 [H, W] with depth=True (the target's prior then carries the intrinsics)."""
    a = np.ascontiguousarray(frame, dtype=np.uint16 if depth else np.float32)
    if a.size != cfg.width * cfg.height * (1 if depth else 3):
        raise SsdError("stair_pose_host: the array is not one frame")
    out = StairPoseMoments()
    rule = rule or StairPoseRule()
    _check(lib().ssd_stair_pose_host(C.byref(cfg), C.byref(target), _input_code(depth), a.ctypes.data_as(C.c_void_p), C.byref(rule), C.byref(out)))
    return out


def stair_pose_add(moments, acc):
    """ssd_stair_pose_add: the fold's step - acc's headers become moments', every sum is added; SsdError (SSD_E_CAP) and acc untouched
    if a sum would leave int64.  Returns acc."""
    _check(lib().ssd_stair_pose_add(C.byref(moments) if moments is not None else None, C.byref(acc) if acc is not None else None))
    return acc


def stair_pose_solve(moments, target, min_points=200, observable=SP_OBSERVABLE):
    """ssd_stair_pose_solve: a frame's record, or a fold of many, -> one Gauss-Newton step against the target's map (StairPose)"""
    out = StairPose()
    _check(lib().ssd_stair_pose_solve(C.byref(moments), C.byref(target), int(min_points), float(observable), C.byref(out)))
    return out


def depth_fuse_default_rule(n):
    """ssd_depth_fuse_default_rule: min_valid = min_agree = (n + 1) // 2, tol = FUSE_TOL"""
    rule = FuseRule()
    _check(lib().ssd_depth_fuse_default_rule(int(n), C.byref(rule)))
    return rule


def depth_fuse_host(frames, rule=None, support=False, stride_bytes=None):
    """ssd_depth_fuse_host: ONE group of depth frames, uint16 [n, H, W] (any strides along n that are a multiple of 2 bytes and hold a
    frame), -> (fused uint16 [H, W], FuseStats), with support=True (fused, FuseStats, support uint8 [H, W]).  rule None: the defaults"""
    a = frames if isinstance(frames, np.ndarray) else np.asarray(frames)
    if a.dtype != np.uint16 or a.ndim != 3 or not a[0].flags.c_contiguous:
        raise SsdError("depth_fuse_host: uint16 [n, H, W] with contiguous frames expected")
    n, H, W = a.shape
    stride = int(stride_bytes) if stride_bytes is not None else (a.strides[0] if n > 1 else H * W * 2)
    out, stats = np.zeros((H, W), np.uint16), FuseStats()
    sup = np.zeros((H, W), np.uint8) if support else None
    _check(lib().ssd_depth_fuse_host(W, H, a.ctypes.data_as(C.c_void_p), stride, n, None if rule is None else C.byref(rule),
                                     out.ctypes.data_as(C.c_void_p), None if sup is None else sup.ctypes.data_as(C.c_void_p), C.byref(stats)))
    return (out, stats, sup) if support else (out, stats)


def depth_edges_default_rule():
    """ssd_depth_edge_default_rule: min_support 2, bridge on, tol = FUSE_TOL, slope = EDGE_SLOPE"""
    rule = EdgeRule()
    _check(lib().ssd_depth_edge_default_rule(C.byref(rule)))
    return rule


def depth_edges_host(frame, rule=None, classes=False):
    """ssd_depth_edges_host: ONE depth frame, uint16 [H, W] -> (filtered uint16 [H, W], EdgeStats), with classes=True (filtered,
    EdgeStats, classes uint8 [H, W]: EDGE_KEPT / EDGE_EMPTY / EDGE_LONE / EDGE_BRIDGE).  rule None: the defaults"""
    a = np.ascontiguousarray(frame)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise SsdError("depth_edges_host: uint16 [H, W] expected")
    H, W = a.shape
    out, stats = np.zeros((H, W), np.uint16), EdgeStats()
    cls = np.zeros((H, W), np.uint8) if classes else None
    _check(lib().ssd_depth_edges_host(W, H, a.ctypes.data_as(C.c_void_p), None if rule is None else C.byref(rule), out.ctypes.data_as(C.c_void_p),
                                      None if cls is None else cls.ctypes.data_as(C.c_void_p), C.byref(stats)))
    return (out, stats, cls) if classes else (out, stats)


def depth_warp_view_between(src, dst):
    """ssd_depth_warp_view_between: two cameras (each a Camera or anything set_cameras takes; src with intrinsics) whose calibrations
    share one external world -> the WarpView from src's camera coordinates to dst's"""
    out = WarpView()
    _check(lib().ssd_depth_warp_view_between(None if src is None else C.byref(_as_camera(src)), None if dst is None else C.byref(_as_camera(dst)),
                                             C.byref(out)))
    return out


def _warp_views(views, n=None):
    """one WarpView, or a sequence of them -> a ctypes array (one is handed on as it is)"""
    if isinstance(views, C.Array) and views._type_ is WarpView and (n is None or len(views) == n):
        return views
    seq = [views] if isinstance(views, WarpView) else list(views)
    if n is not None and len(seq) != n:
        raise SsdError("depth warp: %d views for %d frames" % (len(seq), n))
    return (WarpView * max(len(seq), 1))(*seq)


def depth_warp_host(frame, view, dst):
    """ssd_depth_warp_host: ONE depth frame, uint16 [H, W], seen under view.src, as the target camera with the Intrinsics dst would
    have seen it -> (warped uint16 [H, W], WarpStats)"""
    a = np.ascontiguousarray(frame)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise SsdError("depth_warp_host: uint16 [H, W] expected")
    H, W = a.shape
    out, stats = np.zeros((H, W), np.uint16), WarpStats()
    _check(lib().ssd_depth_warp_host(W, H, a.ctypes.data_as(C.c_void_p), None if view is None else C.byref(view),
                                     None if dst is None else C.byref(dst), out.ctypes.data_as(C.c_void_p), C.byref(stats)))
    return out, stats


def depth_fill_default_rule():
    """ssd_depth_fill_default_rule: min_pairs 1, cover 1, tol = FUSE_TOL, slope 0"""
    rule = FillRule()
    _check(lib().ssd_depth_fill_default_rule(C.byref(rule)))
    return rule


def depth_fill_host(frame, rule=None, classes=False):
    """ssd_depth_fill_host: ONE depth frame, uint16 [H, W] -> (filled uint16 [H, W], FillStats), with classes=True (filled, FillStats,
    classes uint8 [H, W]: FILL_KEPT / FILL_EMPTY / FILL_FILLED / FILL_COVERED).  rule None: the defaults"""
    a = np.ascontiguousarray(frame)
    if a.dtype != np.uint16 or a.ndim != 2:
        raise SsdError("depth_fill_host: uint16 [H, W] expected")
    H, W = a.shape
    out, stats = np.zeros((H, W), np.uint16), FillStats()
    cls = np.zeros((H, W), np.uint8) if classes else None
    _check(lib().ssd_depth_fill_host(W, H, a.ctypes.data_as(C.c_void_p), None if rule is None else C.byref(rule), out.ctypes.data_as(C.c_void_p),
                                     None if cls is None else cls.ctypes.data_as(C.c_void_p), C.byref(stats)))
    return (out, stats, cls) if classes else (out, stats)


def riser_fit_solve(moments, risers, cal, min_points=100):
    """ssd_riser_fit_solve: a frame's riser moments (FrameMoments, record i = riser i) and its FrameRisers -> a plane per riser
    (FrameRiserFits; per riser GF_OK / GF_FEW / GF_DEGENERATE, lean, skew, rise and going)"""
    c = cal.constants if isinstance(cal, GeometricTransformation) else cal.cal if isinstance(cal, Camera) else cal
    out = FrameRiserFits()
    _check(lib().ssd_riser_fit_solve(C.byref(moments) if moments is not None else None, C.byref(risers) if risers is not None else None,
                                     C.byref(c) if c is not None else None, int(min_points), C.byref(out)))
    return out


def camera_drift_fold(moments, camera_of_frame, cameras, min_points=2000):
    """ssd_camera_drift_fold: per camera of `cameras` (a list of anything Detector.set_cameras takes), the ground moments of the frames
    that name it (moments: FrameMoments per frame, as the cameras surface-fit calls return them) added exactly, and the ground fit of
    the sum against that camera's calibration -> list of CameraDrift, one per camera"""
    n = len(moments)
    idx = np.ascontiguousarray(camera_of_frame, dtype=np.uint16)
    if idx.ndim != 1 or idx.size != n or np.any(np.asarray(camera_of_frame) != idx):
        raise SsdError("camera_of_frame: one index 0..65535 per frame")
    mom = moments if isinstance(moments, C.Array) and moments._type_ is FrameMoments else (FrameMoments * max(1, n))(*moments)
    cams = cameras if isinstance(cameras, C.Array) and cameras._type_ is Camera else _camera_array(list(cameras))[0]
    ncams = len(cameras)
    out = (CameraDrift * max(1, ncams))()
    _check(lib().ssd_camera_drift_fold(mom, idx.ctypes.data_as(C.POINTER(C.c_uint16)), n, cams, ncams, int(min_points), out))
    return [CameraDrift.from_buffer_copy(out[i]) for i in range(ncams)]


def camera_ground_gates(moments, camera_of_frame, drift, gates, k_sigma=2.5, gate_min=0.0):
    """ssd_camera_ground_gates: the ground gate (g[0]) of every frame with a ground whose camera's folded fit (drift: the list
    camera_drift_fold returns, one CameraDrift per camera) is GF_OK becomes that fit's plane with max(k_sigma * fit.rms, gate_min);
    gates: a FrameGates per frame, as surface_gates_from_moments made them -> the list of FrameGates, the others as given"""
    n = len(moments)
    idx = np.ascontiguousarray(camera_of_frame, dtype=np.uint16)
    if idx.ndim != 1 or idx.size != n or np.any(np.asarray(camera_of_frame) != idx):
        raise SsdError("camera_of_frame: one index 0..65535 per frame")
    if len(gates) != n:
        raise SsdError("camera_ground_gates: one FrameGates per frame")
    mom = moments if isinstance(moments, C.Array) and moments._type_ is FrameMoments else (FrameMoments * max(1, n))(*moments)
    ncams = len(drift)
    dr = drift if isinstance(drift, C.Array) and drift._type_ is CameraDrift else (CameraDrift * max(1, ncams))(*drift)
    arr = (FrameGates * max(1, n))(*gates)
    _check(lib().ssd_camera_ground_gates(mom, idx.ctypes.data_as(C.POINTER(C.c_uint16)), n, dr, ncams, float(k_sigma), float(gate_min), arr))
    return [FrameGates.from_buffer_copy(arr[i]) for i in range(n)]


def camera_drift_from_fold(fold, cameras, min_points=2000):
    """ssd_camera_drift_from_fold: CameraFold records (one per camera of `cameras`, as Detector.enqueue_camera_fold makes them on the
    device, or the heads of CameraDrift records) -> list of CameraDrift: the head copied, the ground fit of its sums against that
    camera's calibration.  Byte for byte camera_drift_fold over the records that made the fold"""
    ncams = len(cameras)
    if len(fold) != ncams:
        raise SsdError("camera_drift_from_fold: one CameraFold per camera")
    arr = fold if isinstance(fold, C.Array) and fold._type_ is CameraFold else (CameraFold * max(1, ncams))(*fold)
    cams = cameras if isinstance(cameras, C.Array) and cameras._type_ is Camera else _camera_array(list(cameras))[0]
    out = (CameraDrift * max(1, ncams))()
    _check(lib().ssd_camera_drift_from_fold(arr, cams, ncams, int(min_points), out))
    return [CameraDrift.from_buffer_copy(out[i]) for i in range(ncams)]


# --------------------------------------------------------------------------- reference-shaped classes
class GeometricTransformation:
    """reference transformation.h:102-126; constructor transformation.cpp:196-215."""

    def __init__(self, world_points=None, camera_points=None):
        self.constants = Calibration()
        if world_points is None:
            _check(lib().ssd_calibration_identity(C.byref(self.constants)))
        else:
            w = (C.c_double * 9)(*np.asarray(world_points, dtype=np.float64).reshape(9))
            c = (C.c_double * 9)(*np.asarray(camera_points, dtype=np.float64).reshape(9))
            _check(lib().ssd_calibration_from_points(w, c, C.byref(self.constants)))


class GeometricCalibration:
    """reference geometricCalibration.h:32-37: the offline half."""

    @staticmethod
    def load(directory="."):
        """GeometricCalibration::load() (geometricCalibration.cpp:185-203) -> (GeometricTransformation, loaded)."""
        t = GeometricTransformation()
        loaded = C.c_int(0)
        w, c = (C.c_double * 9)(), (C.c_double * 9)()
        _check(lib().ssd_calibration_load(os.path.join(directory, "calibration-triangle").encode(),
                                          os.path.join(directory, "calibration-points").encode(),
                                          C.byref(t.constants), C.byref(loaded), w, c))
        t.world_points = np.array(w).reshape(3, 3) if loaded.value else None
        t.camera_points = np.array(c).reshape(3, 3) if loaded.value else None
        return t, bool(loaded.value)


class Stairs:
    """reference stairs.h:30-39."""

    def __init__(self, result):
        self.result = result
        self.status = result.status
        self.stair_steps = [(result.steps[i].height, [(result.steps[i].quad[2 * k], result.steps[i].quad[2 * k + 1])
                                                      for k in range(4)]) for i in range(result.n_steps)]

    def serialize(self):
        buf = C.create_string_buffer(LINE_CAP)
        _check(lib().ssd_serialize(C.byref(self.result), buf, LINE_CAP))
        return buf.value.decode()


class Window:
    """reference window.h: the GL sink; has no effect on results."""

    def __init__(self, name=""):
        self.name = name


class Detector:
    """One handle = one device = one `Pointcloud` of the reference, plus the batch entry points."""

    def __init__(self, cfg, trans, device=0):
        self.cfg = cfg
        self.device = device
        self._h = C.c_void_p()
        cal = trans.constants if isinstance(trans, GeometricTransformation) else trans
        _check(lib().ssd_create(C.byref(cfg), C.byref(cal), device, C.byref(self._h)))
        self.frame_bytes = cfg.width * cfg.height * 12

    def close(self):
        if self._h:
            lib().ssd_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self):
        return lib().ssd_workspace_bytes(self._h)

    @property
    def batches_in_flight(self):
        """workspaces of the handle = batches it keeps in flight (ssd_config::batches_in_flight resolved)"""
        return lib().ssd_batches_in_flight(self._h)

    def stream_wait(self, back=0, stream=None):
        """makes `stream` wait for the batch `back` enqueues ago (ssd_stream_wait)"""
        _check(lib().ssd_stream_wait(self._h, back, C.c_void_p(stream or 0)))

    def _frames_arg(self, who, frames, depth):
        """the frames argument of a host-fed method (float32 [n, H, W, 3], or uint16 [n, H, W] with depth; a PinnedArray as it is)
        -> (contiguous array, n, the C `input` code)"""
        a = frames.array if isinstance(frames, PinnedArray) else np.ascontiguousarray(frames, dtype=np.uint16 if depth else np.float32)
        per = self.cfg.width * self.cfg.height * (1 if depth else 3)
        n = a.size // per
        if n < 1 or n * per != a.size:
            raise SsdError("%s: array does not hold whole frames" % who)
        return a, n, _input_code(depth)

    def process_host(self, xyz):
        """xyz: float32 array [n, H, W, 3] (or [H, W, 3]) on the host -> list of FrameResult."""
        a, n, _ = self._frames_arg("process_host", xyz, False)
        res = (FrameResult * n)()
        _check(lib().ssd_process_host(self._h, a.ctypes.data_as(C.c_void_p), n, res))
        return list(res)

    def set_intrinsics(self, intr):
        _check(lib().ssd_set_intrinsics(self._h, C.byref(intr)))
        self._intr = Intrinsics.from_buffer_copy(intr)

    def process_depth_host(self, depth):
        """depth: uint16 array [n, H, W] (or [H, W]) on the host -> list of FrameResult."""
        a = np.ascontiguousarray(depth, dtype=np.uint16)
        n = a.size // (self.cfg.width * self.cfg.height)
        res = (FrameResult * n)()
        _check(lib().ssd_process_depth_host(self._h, a.ctypes.data_as(C.c_void_p), n, res))
        return list(res)

    def enqueue_depth(self, d_ptr, nframes, stride_bytes=None, stream=None):
        _check(lib().ssd_enqueue_depth(self._h, C.c_void_p(d_ptr), stride_bytes or self.cfg.width * self.cfg.height * 2, nframes,
                                       C.c_void_p(stream or 0)))

    def enqueue(self, d_ptr, nframes, stride_bytes=None, stream=None, stages=STAGE_ALL):
        _check(lib().ssd_enqueue_stages(self._h, C.c_void_p(d_ptr), stride_bytes or self.frame_bytes, nframes,
                                        C.c_void_p(stream or 0), stages))

    def enqueue_labels(self, d_ptr, nframes, d_labels, label_stride=None, stride_bytes=None, stream=None):
        """ssd_enqueue plus per-pixel surface labels: frame i's W*H uint8 labels at d_labels + i*label_stride (default W*H),
        complete when fetch() of this batch returns (include/ssd_hip.h: label k + 1 = surface k of the result, 0 = none)"""
        _check(lib().ssd_enqueue_labels(self._h, C.c_void_p(d_ptr), stride_bytes or self.frame_bytes, nframes, C.c_void_p(stream or 0),
                                        C.c_void_p(d_labels), label_stride or self.cfg.width * self.cfg.height))

    def enqueue_depth_labels(self, d_ptr, nframes, d_labels, label_stride=None, stride_bytes=None, stream=None):
        """ssd_enqueue_depth plus per-pixel surface labels (as enqueue_labels)"""
        _check(lib().ssd_enqueue_depth_labels(self._h, C.c_void_p(d_ptr), stride_bytes or self.cfg.width * self.cfg.height * 2, nframes,
                                              C.c_void_p(stream or 0), C.c_void_p(d_labels), label_stride or self.cfg.width * self.cfg.height))

    def process_host_labels(self, xyz):
        """process_host plus labels: -> (list of FrameResult, uint8 array [n, H, W])"""
        a, n, _ = self._frames_arg("process_host_labels", xyz, False)
        res = (FrameResult * n)()
        labels = np.empty((n, self.cfg.height, self.cfg.width), dtype=np.uint8)
        _check(lib().ssd_process_host_labels(self._h, a.ctypes.data_as(C.c_void_p), n, res, labels.ctypes.data_as(C.c_void_p)))
        return list(res), labels

    def process_depth_host_labels(self, depth):
        """process_depth_host plus labels: -> (list of FrameResult, uint8 array [n, H, W])"""
        a, n, _ = self._frames_arg("process_depth_host_labels", depth, True)
        res = (FrameResult * n)()
        labels = np.empty((n, self.cfg.height, self.cfg.width), dtype=np.uint8)
        _check(lib().ssd_process_depth_host_labels(self._h, a.ctypes.data_as(C.c_void_p), n, res, labels.ctypes.data_as(C.c_void_p)))
        return list(res), labels

    # ---- per-frame calibration: batches of frames from many cameras (include/ssd_hip.h)
    def set_cameras(self, cameras):
        """The handle's camera table: a list of GeometricTransformation, Calibration, (either, Intrinsics) or Camera.  Waits for the
        batches in flight; an empty list frees the table."""
        arr = (Camera * max(1, len(cameras)))()
        for i, c in enumerate(cameras):
            if isinstance(c, Camera):
                arr[i] = c
                continue
            trans, intr = c if isinstance(c, (tuple, list)) else (c, None)
            arr[i].cal = trans.constants if isinstance(trans, GeometricTransformation) else trans
            if intr is not None:
                arr[i].intr = intr
                arr[i].has_intrinsics = 1
        _check(lib().ssd_set_cameras(self._h, arr, len(cameras)))
        self._cameras = [Camera.from_buffer_copy(arr[i]) for i in range(len(cameras))]      # what camera_drift folds against

    @property
    def camera_count(self):
        return lib().ssd_camera_count(self._h)

    @staticmethod
    def _camera_index(camera_of_frame, nframes):
        idx = np.ascontiguousarray(camera_of_frame, dtype=np.uint16)
        if idx.ndim != 1 or idx.size != nframes or np.any(np.asarray(camera_of_frame) != idx):
            raise SsdError("camera_of_frame: one index 0..65535 per frame")
        return idx

    def enqueue_cameras(self, d_ptr, nframes, camera_of_frame, depth=False, d_labels=None, label_stride=None, stride_bytes=None, stream=None):
        """ssd_enqueue_cameras: frame i is processed with camera camera_of_frame[i] of the table (the array is copied during the call);
        depth = 16-bit depth input; d_labels as enqueue_labels.  fetch() and the rest as after any enqueue."""
        idx = camera_of_frame if isinstance(camera_of_frame, np.ndarray) and camera_of_frame.dtype == np.uint16 and camera_of_frame.flags.c_contiguous \
            and camera_of_frame.ndim == 1 and camera_of_frame.size == nframes else self._camera_index(camera_of_frame, nframes)
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        _check(lib().ssd_enqueue_cameras(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                         idx.ctypes.data_as(C.POINTER(C.c_uint16)), _input_code(depth),
                                         C.c_void_p(d_labels or 0), (label_stride or self.cfg.width * self.cfg.height) if d_labels else 0))

    def process_host_cameras(self, frames, camera_of_frame, depth=False, labels=False):
        """frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True), one camera index per frame
        -> list of FrameResult, or (list, uint8 labels [n, H, W]) with labels=True"""
        a, n, inp = self._frames_arg("process_host_cameras", frames, depth)
        idx = self._camera_index(camera_of_frame, n)
        res = (FrameResult * n)()
        lab = np.empty((n, self.cfg.height, self.cfg.width), dtype=np.uint8) if labels else None
        _check(lib().ssd_process_host_cameras(self._h, a.ctypes.data_as(C.c_void_p), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)),
                                              inp, res, lab.ctypes.data_as(C.c_void_p) if labels else None))
        return (list(res), lab) if labels else list(res)

    def _fetch_records(self, fn, Type, n, stream, *args):
        """a record fetch of a stand-alone frame pass (fn(handle, out, n, *args, stream)) -> list of n Type (independent copies)"""
        out = (Type * n)()
        _check(fn(self._h, out, n, *args, C.c_void_p(stream or 0)))
        return [Type.from_buffer_copy(r) for r in out]

    def _depth_host_pre(self, who, depth, group, Stats, frames, stats, *args, first=None):
        """a host-fed depth pre-pass (ssd_<who>(handle, depth, total, *args, results, frames, [first's,] stats)): every `group` frames
        become one and that one is detected -> its FrameResults, with the staged frames (uint16 [k, H, W]) and / or its k Stats behind
        them.  first = (Type, wanted): a pre-pass of two passes, whose first leaves a record per INPUT frame - they go in front of the
        k Stats; a list of such pairs: a pre-pass of more passes, each but the last leaving a record per input frame, in that order"""
        a, total, _ = self._frames_arg(who, depth, True)
        k = total // group if group > 0 else 0
        res = (FrameResult * max(k, 1))()
        f = np.zeros((max(k, 1), self.cfg.height, self.cfg.width), np.uint16) if frames else None
        st = (Stats * max(k, 1))() if stats else None
        firsts = [] if not first else [first] if isinstance(first, tuple) else list(first)
        fsts = [(T * max(total, 1))() if wanted else None for T, wanted in firsts]
        _check(getattr(lib(), "ssd_" + who)(self._h, a.ctypes.data_as(C.c_void_p), total, *args, res,
                                            None if f is None else f.ctypes.data_as(C.c_void_p), *fsts, st))
        out = [list(res)[:k]]
        if frames:
            out.append(f[:k])
        for (T, _), fst in zip(firsts, fsts):
            if fst is not None:
                out.append([T.from_buffer_copy(fst[i]) for i in range(total)])
        if stats:
            out.append([Stats.from_buffer_copy(st[i]) for i in range(k)])
        return out[0] if len(out) == 1 else tuple(out)

    # ---- ground fit: a calibration refined from the floor in the frames (include/ssd_hip.h)
    def enqueue_ground_fit(self, d_ptr, nframes, tol, priors=None, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue_ground_fit: the floor moments of frames in device memory, on the caller's stream.  priors: None = the handle's
        calibration, one prior for all frames, or a list of one per frame (each a Camera or anything set_cameras takes)."""
        arr, n = _camera_array(priors)
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        _check(lib().ssd_enqueue_ground_fit(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                            _input_code(depth), arr, n, float(tol)))

    def fetch_ground_fit(self, nframes, min_points=2000, stream=None):
        """ssd_fetch_ground_fit: waits for the last enqueue_ground_fit -> list of GroundFit (independent copies)"""
        return self._fetch_records(lib().ssd_fetch_ground_fit, GroundFit, nframes, stream, int(min_points))

    def process_host_ground_fit(self, frames, tol, priors=None, depth=False, min_points=2000):
        """ssd_process_host_ground_fit: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True) -> list of GroundFit"""
        a, n, inp = self._frames_arg("process_host_ground_fit", frames, depth)
        arr, npriors = _camera_array(priors)
        out = (GroundFit * n)()
        _check(lib().ssd_process_host_ground_fit(self._h, a.ctypes.data_as(C.c_void_p), n, inp, arr, npriors,
                                                 float(tol), int(min_points), out))
        return [GroundFit.from_buffer_copy(r) for r in out]

    def refine_calibration(self, frames, depth=False, prior=None, tolerances=(0.08, 0.03, 0.012), min_points=2000):
        """One process_host_ground_fit per tolerance, each pass starting from the calibration the pass before gave that frame (riser feet
        inside a wide band bias its plane: the band shrinks).  prior: None = the handle's calibration, one prior, or one per frame.  A
        frame whose pass does not end GF_OK keeps its last good calibration and reports the failing status.  -> list of GroundFit"""
        cams = None if prior is None else _camera_array(prior)[0]
        fits = None
        for tol in tolerances:
            fits = self.process_host_ground_fit(frames, tol, priors=None if cams is None else list(cams), depth=depth, min_points=min_points)
            if cams is None or len(cams) != len(fits):
                first = cams[0] if cams is not None else None
                cams = (Camera * len(fits))()
                for i in range(len(fits)):
                    if first is not None:
                        cams[i] = first
                    elif depth:                      # the handle's own intrinsics (the first pass ran with them)
                        cams[i].intr = self._intr
                        cams[i].has_intrinsics = 1
            for i, f in enumerate(fits):
                cams[i].cal = f.cal                 # status != GF_OK: the pass's prior, i.e. the last good calibration
        return fits

    # ---- surface fit: plane, tilt and flatness of every reported surface (include/ssd_hip.h)
    def enqueue_surface_moments(self, d_ptr, nframes, d_moments, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue (depth=True: ssd_enqueue_depth) plus the frames' surface moments: frame i's FrameMoments at
        d_moments + i * sizeof(FrameMoments) in device memory, complete when fetch() of the batch returns"""
        fn = lib().ssd_enqueue_depth_surface_moments if depth else lib().ssd_enqueue_surface_moments
        frame = self.cfg.width * self.cfg.height * 2 if depth else self.frame_bytes
        _check(fn(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0), C.c_void_p(d_moments)))

    def process_host_surfaces(self, frames, depth=False, min_points=200, moments=False):
        """ssd_process_host_surfaces: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True)
        -> (list of FrameResult, list of FrameSurfaces), with moments=True also the list of FrameMoments"""
        a, n, inp = self._frames_arg("process_host_surfaces", frames, depth)
        res, mom, out = (FrameResult * n)(), (FrameMoments * n)(), (FrameSurfaces * n)()
        _check(lib().ssd_process_host_surfaces(self._h, a.ctypes.data_as(C.c_void_p), n, inp, res,
                                               mom if moments else None, int(min_points), out))
        return (list(res), list(out), list(mom)) if moments else (list(res), list(out))

    # ---- trimmed surface refit (include/ssd_hip.h)
    def enqueue_surface_refit(self, d_ptr, nframes, gates, d_moments, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue_surface_refit: the refit pass alone, behind the handle's last whole enqueue of the same frames: frame i's
        FrameMoments over the labelled points inside gates[i] (FrameGates per frame, host) at d_moments + i * sizeof(FrameMoments) in
        device memory; complete when fetch_surface_refit() returns"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        arr = None
        if gates is not None:
            arr = gates if isinstance(gates, C.Array) and gates._type_ is FrameGates else (FrameGates * max(1, len(gates)))(*gates)
            if len(arr) < nframes:
                raise SsdError("enqueue_surface_refit: fewer gates than frames")
        _check(lib().ssd_enqueue_surface_refit(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                               _input_code(depth), arr, C.c_void_p(d_moments)))

    def fetch_surface_refit(self, stream=None):
        """ssd_fetch_surface_refit: waits for the last enqueue_surface_refit"""
        _check(lib().ssd_fetch_surface_refit(self._h, C.c_void_p(stream or 0)))

    def surface_refit_time_ms(self):
        """Device time of the last refit pass (0.0: timing was off for it)"""
        return _time_ms(lib().ssd_get_surface_refit_time, self._h)

    def process_host_surfaces_refit(self, frames, depth=False, min_points=200, k_sigma=2.5, gate_min=0.0, passes=1, moments=False,
                                    device_gates=False):
        """ssd_process_host_surfaces_refit: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True)
        -> (list of FrameResult, list of FrameSurfaces of the last refit pass), with moments=True also the lists of FrameMoments of
        the first pass and of the last refit pass.  device_gates=True: ssd_process_host_surfaces_refit_device (the gates made on the
        device between the passes; the same outputs)"""
        a, n, inp = self._frames_arg("process_host_surfaces_refit", frames, depth)
        res, first, refit, out = (FrameResult * n)(), (FrameMoments * n)(), (FrameMoments * n)(), (FrameSurfaces * n)()
        fn = lib().ssd_process_host_surfaces_refit_device if device_gates else lib().ssd_process_host_surfaces_refit
        _check(fn(self._h, a.ctypes.data_as(C.c_void_p), n, inp, res, first if moments else None,
                  refit if moments else None, int(min_points), float(k_sigma), float(gate_min), int(passes), out))
        return (list(res), list(out), list(first), list(refit)) if moments else (list(res), list(out))

    # ---- tread clearance (include/ssd_hip.h)
    def enqueue_clearance(self, d_ptr, nframes, d_moments, rule=None, d_mask=None, mask_stride=None, depth=False, stride_bytes=None, stream=None,
                          cameras=False):
        """ssd_enqueue_clearance: the clearance pass alone, behind the handle's last whole enqueue of the same frames: frame i's
        FrameMoments over its occupants at d_moments + i * sizeof(FrameMoments) and, with d_mask, its W * H mask bytes at
        d_mask + i * mask_stride, both device memory; complete when fetch_clearance() returns"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        rule = ClearanceRule() if rule is None else rule
        fn = lib().ssd_enqueue_cameras_clearance if cameras else lib().ssd_enqueue_clearance
        _check(fn(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0), _input_code(depth),
                  C.byref(rule), C.c_void_p(d_moments), C.c_void_p(d_mask or 0), mask_stride or self.cfg.width * self.cfg.height))

    def enqueue_cameras_clearance(self, d_ptr, nframes, d_moments, rule=None, d_mask=None, mask_stride=None, depth=False, stride_bytes=None,
                                  stream=None):
        """ssd_enqueue_cameras_clearance: enqueue_clearance behind the handle's last whole CAMERAS enqueue of the same frames"""
        self.enqueue_clearance(d_ptr, nframes, d_moments, rule, d_mask, mask_stride, depth, stride_bytes, stream, cameras=True)

    def fetch_clearance(self, stream=None):
        """ssd_fetch_clearance: waits for the last enqueue_clearance"""
        _check(lib().ssd_fetch_clearance(self._h, C.c_void_p(stream or 0)))

    def clearance_time_ms(self):
        """Device time of the last clearance pass (0.0: timing was off for it)"""
        return _time_ms(lib().ssd_get_clearance_time, self._h)

    def process_host_clearance(self, frames, rule=None, min_support=50, depth=False, moments=False, mask=False, camera_of_frame=None):
        """ssd_process_host_clearance: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True)
        -> (list of FrameResult, list of FrameClearance), with moments=True also the list of FrameMoments, with mask=True also the
        masks (uint8 [n, H, W])"""
        a, n, inp = self._frames_arg("process_host_clearance", frames, depth)
        rule = ClearanceRule() if rule is None else rule
        res, mom, out = (FrameResult * n)(), (FrameMoments * n)(), (FrameClearance * n)()
        m = np.empty((n, self.cfg.height, self.cfg.width), dtype=np.uint8) if mask else None
        tail = (C.byref(rule), int(min_support), res, mom if moments else None, m.ctypes.data_as(C.c_void_p) if mask else None, out)
        if camera_of_frame is None:
            _check(lib().ssd_process_host_clearance(self._h, a.ctypes.data_as(C.c_void_p), n, inp, *tail))
        else:
            idx = self._camera_index(camera_of_frame, n)
            _check(lib().ssd_process_host_cameras_clearance(self._h, a.ctypes.data_as(C.c_void_p), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)), inp, *tail))
        ret = [list(res), list(out)]
        if moments:
            ret.append(list(mom))
        if mask:
            ret.append(m)
        return tuple(ret)

    def process_host_cameras_clearance(self, frames, camera_of_frame, rule=None, min_support=50, depth=False, moments=False, mask=False):
        """ssd_process_host_cameras_clearance: process_host_clearance with one camera index per frame"""
        return self.process_host_clearance(frames, rule, min_support, depth, moments, mask, camera_of_frame=camera_of_frame)

    # ---- tread grid (include/ssd_hip.h)
    def enqueue_tread_grid(self, d_ptr, nframes, d_grids, rule=None, depth=False, stride_bytes=None, stream=None, cameras=False):
        """ssd_enqueue_tread_grid: the tread grid pass alone, behind the handle's last whole enqueue of the same frames: frame i's
        FrameTreadGrid at d_grids + i * sizeof(FrameTreadGrid), device memory; complete when fetch_tread_grid() returns"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        rule = TreadGridRule() if rule is None else rule
        fn = lib().ssd_enqueue_cameras_tread_grid if cameras else lib().ssd_enqueue_tread_grid
        _check(fn(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0), _input_code(depth),
                  C.byref(rule), C.c_void_p(d_grids)))

    def enqueue_cameras_tread_grid(self, d_ptr, nframes, d_grids, rule=None, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue_cameras_tread_grid: enqueue_tread_grid behind the handle's last whole CAMERAS enqueue of the same frames"""
        self.enqueue_tread_grid(d_ptr, nframes, d_grids, rule, depth, stride_bytes, stream, cameras=True)

    def fetch_tread_grid(self, stream=None):
        """ssd_fetch_tread_grid: waits for the last enqueue_tread_grid"""
        _check(lib().ssd_fetch_tread_grid(self._h, C.c_void_p(stream or 0)))

    def tread_grid_time_ms(self):
        """Device time of the last tread grid pass (0.0: timing was off for it)"""
        return _time_ms(lib().ssd_get_tread_grid_time, self._h)

    def process_host_tread_grid(self, frames, rule=None, min_seen=1, min_occ=1, foot_along=0.0, foot_deep=0.0, depth=False, grids=False,
                                camera_of_frame=None):
        """ssd_process_host_tread_grid: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True)
        -> (list of FrameResult, list of FrameFootholds), with grids=True also the list of FrameTreadGrid"""
        a, n, inp = self._frames_arg("process_host_tread_grid", frames, depth)
        rule = TreadGridRule() if rule is None else rule
        res, out = (FrameResult * n)(), (FrameFootholds * n)()
        g = (FrameTreadGrid * n)() if grids else None
        tail = (C.byref(rule), int(min_seen), int(min_occ), float(foot_along), float(foot_deep), res, g, out)
        if camera_of_frame is None:
            _check(lib().ssd_process_host_tread_grid(self._h, a.ctypes.data_as(C.c_void_p), n, inp, *tail))
        else:
            idx = self._camera_index(camera_of_frame, n)
            _check(lib().ssd_process_host_cameras_tread_grid(self._h, a.ctypes.data_as(C.c_void_p), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)), inp, *tail))
        return (list(res), list(out), list(g)) if grids else (list(res), list(out))

    def process_host_cameras_tread_grid(self, frames, camera_of_frame, rule=None, min_seen=1, min_occ=1, foot_along=0.0, foot_deep=0.0, depth=False,
                                        grids=False):
        """ssd_process_host_cameras_tread_grid: process_host_tread_grid with one camera index per frame"""
        return self.process_host_tread_grid(frames, rule, min_seen, min_occ, foot_along, foot_deep, depth, grids, camera_of_frame=camera_of_frame)

    # ---- stair map (include/ssd_hip.h)
    def enqueue_stair_map(self, d_ptr, nframes, maps, d_grids, map_of_frame=None, rule=None, accumulate=False, depth=False, stride_bytes=None,
                          stream=None, cameras=False):
        """ssd_enqueue_stair_map: the tread grid's rule against the caller's staircases, behind the handle's last whole enqueue of the same
        frames: every frame i adds to the FrameTreadGrid of map map_of_frame[i] (None: map 0; STAIR_MAP_NONE: nothing) at d_grids +
        m * sizeof(FrameTreadGrid), device memory, zeroed first unless accumulate; complete when fetch_stair_map() returns.
        maps: StairMap, FrameResult or a sequence of them (host; copied during the call)"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        rule = TreadGridRule() if rule is None else rule
        arr, nmaps = _stair_maps(maps)
        idx = _map_index(map_of_frame, nframes)
        fn = lib().ssd_enqueue_cameras_stair_map if cameras else lib().ssd_enqueue_stair_map
        _check(fn(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0), _input_code(depth), arr, nmaps,
                  idx.ctypes.data_as(C.POINTER(C.c_uint16)) if idx is not None else None, C.byref(rule), 1 if accumulate else 0,
                  C.c_void_p(d_grids)))

    def enqueue_cameras_stair_map(self, d_ptr, nframes, maps, d_grids, map_of_frame=None, rule=None, accumulate=False, depth=False,
                                  stride_bytes=None, stream=None):
        """ssd_enqueue_cameras_stair_map: enqueue_stair_map behind the handle's last whole CAMERAS enqueue of the same frames"""
        self.enqueue_stair_map(d_ptr, nframes, maps, d_grids, map_of_frame, rule, accumulate, depth, stride_bytes, stream, cameras=True)

    def fetch_stair_map(self, stream=None):
        """ssd_fetch_stair_map: waits for the last enqueue_stair_map"""
        _check(lib().ssd_fetch_stair_map(self._h, C.c_void_p(stream or 0)))

    def stair_map_time_ms(self):
        """Device time of the last stair map pass (0.0: timing was off for it)"""
        return _time_ms(lib().ssd_get_stair_map_time, self._h)

    def process_host_stair_map(self, frames, maps, map_of_frame=None, rule=None, min_seen=1, min_occ=1, foot_along=0.0, foot_deep=0.0, depth=False,
                               camera_of_frame=None, grids=False):
        """ssd_process_host_stair_map: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True) folded into one
        record per map -> (list of FrameResult per frame, list of FrameFootholds per map), with grids=True also the FrameTreadGrid per map"""
        a, n, inp = self._frames_arg("process_host_stair_map", frames, depth)
        rule = TreadGridRule() if rule is None else rule
        arr, nmaps = _stair_maps(maps)
        idx = _map_index(map_of_frame, n)
        res, out = (FrameResult * n)(), (FrameFootholds * max(nmaps, 1))()
        g = (FrameTreadGrid * max(nmaps, 1))() if grids else None
        tail = (arr, nmaps, idx.ctypes.data_as(C.POINTER(C.c_uint16)) if idx is not None else None, C.byref(rule), int(min_seen), int(min_occ),
                float(foot_along), float(foot_deep), res, g, out)
        if camera_of_frame is None:
            _check(lib().ssd_process_host_stair_map(self._h, a.ctypes.data_as(C.c_void_p), n, inp, *tail))
        else:
            cam = self._camera_index(camera_of_frame, n)
            _check(lib().ssd_process_host_cameras_stair_map(self._h, a.ctypes.data_as(C.c_void_p), n, cam.ctypes.data_as(C.POINTER(C.c_uint16)), inp, *tail))
        return (list(res), list(out)[:nmaps], list(g)[:nmaps]) if grids else (list(res), list(out)[:nmaps])

    def process_host_cameras_stair_map(self, frames, camera_of_frame, maps, map_of_frame=None, rule=None, min_seen=1, min_occ=1, foot_along=0.0,
                                       foot_deep=0.0, depth=False, grids=False):
        """ssd_process_host_cameras_stair_map: process_host_stair_map with one camera index per frame"""
        return self.process_host_stair_map(frames, maps, map_of_frame, rule, min_seen, min_occ, foot_along, foot_deep, depth, camera_of_frame, grids)

    # ---- stair pose: a camera located against a stair map from its treads and risers (include/ssd_hip.h)
    def enqueue_stair_pose(self, d_ptr, nframes, targets, target_of_frame=None, rule=None, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue_stair_pose: every frame's points sorted onto its target's treads and risers, on the caller's stream.  targets: a
        StairPoseTarget, a (prior, map) pair or a sequence of either (host; copied during the call); target_of_frame: None = target 0, or
        one index per frame (STAIR_MAP_NONE: the frame adds nothing)."""
        arr, n = _pose_targets(targets)
        idx = _map_index(target_of_frame, nframes)
        rule = rule or StairPoseRule()
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        _check(lib().ssd_enqueue_stair_pose(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0), _input_code(depth),
                                            arr, n, None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(rule)))
        self._pose_targets = n

    def fetch_stair_pose_moments(self, nframes, stream=None):
        """ssd_fetch_stair_pose_moments: waits for the last enqueue_stair_pose -> list of StairPoseMoments (independent copies)"""
        return self._fetch_records(lib().ssd_fetch_stair_pose_moments, StairPoseMoments, nframes, stream)

    def fetch_stair_pose(self, min_points=200, observable=SP_OBSERVABLE, stream=None):
        """ssd_fetch_stair_pose: waits likewise; per target the fold of its frames' records, solved -> list of StairPose"""
        n = getattr(self, "_pose_targets", 0)                         # the last call's targets (process_host_stair_pose's slices are calls too)
        out = (StairPose * MAX_STAIR_MAPS)()
        _check(lib().ssd_fetch_stair_pose(self._h, out, int(min_points), float(observable), C.c_void_p(stream or 0)))
        return [StairPose.from_buffer_copy(out[i]) for i in range(n)]

    def stair_pose_time_ms(self):
        """the device time of the last stair pose pass, its zeroing and its records' copy included (0 unless set_timing was on)"""
        return _time_ms(lib().ssd_get_stair_pose_time, self._h)

    def process_host_stair_pose(self, frames, targets, target_of_frame=None, rule=None, min_points=200, observable=SP_OBSERVABLE, depth=False,
                                moments=False):
        """ssd_process_host_stair_pose: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True) -> list of StairPose,
        one per target (with moments=True: (that, list of StairPoseMoments, one per frame))"""
        a, n, inp = self._frames_arg("process_host_stair_pose", frames, depth)
        arr, nt = _pose_targets(targets)
        idx = _map_index(target_of_frame, n)
        rule = rule or StairPoseRule()
        out = (StairPose * max(nt, 1))()
        recs = (StairPoseMoments * n)() if moments else None
        _check(lib().ssd_process_host_stair_pose(self._h, a.ctypes.data_as(C.c_void_p), n, inp, arr, nt,
                                                 None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(rule), int(min_points),
                                                 float(observable), recs, out))
        self._pose_targets = nt
        poses = [StairPose.from_buffer_copy(out[i]) for i in range(nt)]
        return (poses, [StairPoseMoments.from_buffer_copy(r) for r in recs]) if moments else poses

    # ---- depth fusion: one trimmed-median frame from n frames of a still camera (include/ssd_hip.h)
    def enqueue_depth_fuse(self, d_ptr, nframes, n, d_out, hop=None, rule=None, d_support=None, stride_bytes=None, out_stride_bytes=None,
                           support_stride_bytes=None, stream=None):
        """ssd_enqueue_depth_fuse: groups of n of the nframes uint16 depth frames at d_ptr, hop frames apart (None: n, disjoint groups),
        fused on the caller's stream: frame g to d_out + g * out_stride_bytes, its support bytes (d_support None: none) likewise.
        -> the number of groups.  A depth-input enqueue on the same stream may read d_out with no host wait in between."""
        frame = self.cfg.width * self.cfg.height * 2
        hop = int(n) if hop is None else int(hop)
        _check(lib().ssd_enqueue_depth_fuse(self._h, C.c_void_p(d_ptr), stride_bytes or frame, int(nframes), C.c_void_p(stream or 0), int(n), hop,
                                            None if rule is None else C.byref(rule), C.c_void_p(d_out), out_stride_bytes or frame,
                                            C.c_void_p(d_support or 0), support_stride_bytes or frame // 2))
        return (int(nframes) - int(n)) // hop + 1

    def fetch_depth_fuse(self, ngroups, stream=None):
        """ssd_fetch_depth_fuse: waits for the last enqueue_depth_fuse -> list of FuseStats (independent copies), one per group"""
        return self._fetch_records(lib().ssd_fetch_depth_fuse, FuseStats, ngroups, stream)

    def depth_fuse_time_ms(self):
        """the device time of the last fusion pass, its zeroing and its records' copy included (0 unless set_timing was on)"""
        return _time_ms(lib().ssd_get_depth_fuse_time, self._h)

    def process_depth_host_fused(self, depth, n, rule=None, fused=False, stats=False):
        """ssd_process_depth_host_fused: depth frames on the host, uint16 [k * n, H, W]: every n of them fused on the device and the
        fused frame detected -> list of k FrameResult; with fused=True / stats=True a tuple with the fused frames (uint16 [k, H, W])
        and / or the list of k FuseStats behind it"""
        return self._depth_host_pre("process_depth_host_fused", depth, int(n), FuseStats, fused, stats, int(n), None if rule is None else C.byref(rule))

    # ---- depth edge filter: mixed and lone pixels out of one frame (include/ssd_hip.h)
    def enqueue_depth_edges(self, d_ptr, nframes, d_out, rule=None, d_cls=None, stride_bytes=None, out_stride_bytes=None, cls_stride_bytes=None,
                            stream=None):
        """ssd_enqueue_depth_edges: the nframes uint16 depth frames at d_ptr filtered on the caller's stream: frame i to d_out + i *
        out_stride_bytes, its class bytes (d_cls None: none) likewise.  -> nframes.  A depth-input enqueue on the same stream may read
        d_out with no host wait in between.  The output must not overlap the input."""
        frame = self.cfg.width * self.cfg.height * 2
        _check(lib().ssd_enqueue_depth_edges(self._h, C.c_void_p(d_ptr), stride_bytes or frame, int(nframes), C.c_void_p(stream or 0),
                                             None if rule is None else C.byref(rule), C.c_void_p(d_out), out_stride_bytes or frame,
                                             C.c_void_p(d_cls or 0), cls_stride_bytes or frame // 2))
        return int(nframes)

    def fetch_depth_edges(self, nframes, stream=None):
        """ssd_fetch_depth_edges: waits for the last enqueue_depth_edges -> list of EdgeStats (independent copies), one per frame"""
        return self._fetch_records(lib().ssd_fetch_depth_edges, EdgeStats, nframes, stream)

    def depth_edges_time_ms(self):
        """the device time of the last filter pass, its zeroing and its records' copy included (0 unless set_timing was on)"""
        return _time_ms(lib().ssd_get_depth_edges_time, self._h)

    depth_edges_time = depth_edges_time_ms                            # the name it was added under

    def process_depth_host_edges(self, depth, rule=None, filtered=False, stats=False):
        """ssd_process_depth_host_edges: depth frames on the host, uint16 [k, H, W]: every frame filtered on the device and the filtered
        frame detected -> list of k FrameResult; with filtered=True / stats=True a tuple with the filtered frames (uint16 [k, H, W])
        and / or the list of k EdgeStats behind it"""
        return self._depth_host_pre("process_depth_host_edges", depth, 1, EdgeStats, filtered, stats, None if rule is None else C.byref(rule))

    # ---- depth warp: the frame another pose would have seen (include/ssd_hip.h)
    def enqueue_depth_warp(self, d_ptr, nframes, views, dst, d_out, stride_bytes=None, out_stride_bytes=None, stream=None):
        """ssd_enqueue_depth_warp: the nframes uint16 depth frames at d_ptr, frame i warped under views[i] (a list of WarpView on the
        host, or one for a single frame) into the view with the Intrinsics dst, on the caller's stream: frame i to d_out + i *
        out_stride_bytes.  -> nframes.  enqueue_depth_fuse, enqueue_depth_edges or a depth-input enqueue on the same stream may read
        d_out with no host wait in between.  d_out and its stride are multiples of 4; the output must not overlap the input."""
        frame = self.cfg.width * self.cfg.height * 2
        arr = _warp_views(views, int(nframes))
        _check(lib().ssd_enqueue_depth_warp(self._h, C.c_void_p(d_ptr), stride_bytes or frame, int(nframes), C.c_void_p(stream or 0), arr,
                                            None if dst is None else C.byref(dst), C.c_void_p(d_out), out_stride_bytes or frame))
        return int(nframes)

    def fetch_depth_warp(self, nframes, stream=None):
        """ssd_fetch_depth_warp: waits for the last enqueue_depth_warp -> list of WarpStats (independent copies), one per frame"""
        return self._fetch_records(lib().ssd_fetch_depth_warp, WarpStats, nframes, stream)

    def depth_warp_time_ms(self):
        """the device time of the last warp pass, its zeroing and its records' copy included (0 unless set_timing was on)"""
        return _time_ms(lib().ssd_get_depth_warp_time, self._h)

    def process_depth_host_warp_fused(self, depth, n, views, dst, fuse_rule=None, fused=False, warp_stats=False, fuse_stats=False):
        """ssd_process_depth_host_warp_fused: depth frames of a moving camera on the host, uint16 [k * n, H, W]: frame i warped under
        views[i] into the view dst (the handle's intrinsics), every n warped frames fused and the fused frame detected -> list of k
        FrameResult; with fused=True / warp_stats=True / fuse_stats=True a tuple with the fused frames (uint16 [k, H, W]), the list of
        k * n WarpStats and / or the list of k FuseStats behind it, in this order"""
        total = len(depth)
        arr = _warp_views(views, total)
        return self._depth_host_pre("process_depth_host_warp_fused", depth, int(n), FuseStats, fused, fuse_stats, int(n), arr,
                                    None if dst is None else C.byref(dst), None if fuse_rule is None else C.byref(fuse_rule),
                                    first=(WarpStats, warp_stats))

    # ---- depth fill: holes and one-pixel see-through closed between agreeing samples (include/ssd_hip.h)
    def enqueue_depth_fill(self, d_ptr, nframes, d_out, rule=None, d_cls=None, stride_bytes=None, out_stride_bytes=None, cls_stride_bytes=None,
                           stream=None):
        """ssd_enqueue_depth_fill: the nframes uint16 depth frames at d_ptr filled on the caller's stream: frame i to d_out + i *
        out_stride_bytes, its class bytes (d_cls None: none) likewise.  -> nframes.  d_ptr may be what enqueue_depth_warp wrote on that
        stream, and enqueue_depth_fuse, enqueue_depth_edges or a depth-input enqueue on it may read d_out, with no host wait in
        between.  The output must not overlap the input."""
        frame = self.cfg.width * self.cfg.height * 2
        _check(lib().ssd_enqueue_depth_fill(self._h, C.c_void_p(d_ptr), stride_bytes or frame, int(nframes), C.c_void_p(stream or 0),
                                            None if rule is None else C.byref(rule), C.c_void_p(d_out), out_stride_bytes or frame,
                                            C.c_void_p(d_cls or 0), cls_stride_bytes or frame // 2))
        return int(nframes)

    def fetch_depth_fill(self, nframes, stream=None):
        """ssd_fetch_depth_fill: waits for the last enqueue_depth_fill -> list of FillStats (independent copies), one per frame"""
        return self._fetch_records(lib().ssd_fetch_depth_fill, FillStats, nframes, stream)

    def depth_fill_time_ms(self):
        """the device time of the last fill pass, its zeroing and its records' copy included (0 unless set_timing was on)"""
        return _time_ms(lib().ssd_get_depth_fill_time, self._h)

    def process_depth_host_fill(self, depth, rule=None, filled=False, stats=False):
        """ssd_process_depth_host_fill: depth frames on the host, uint16 [k, H, W]: every frame filled on the device and the filled
        frame detected -> list of k FrameResult; with filled=True / stats=True a tuple with the filled frames (uint16 [k, H, W]) and /
        or the list of k FillStats behind it"""
        return self._depth_host_pre("process_depth_host_fill", depth, 1, FillStats, filled, stats, None if rule is None else C.byref(rule))

    def process_depth_host_warp_fill_fused(self, depth, n, views, dst, fill_rule=None, fuse_rule=None, fused=False, warp_stats=False,
                                           fill_stats=False, fuse_stats=False):
        """ssd_process_depth_host_warp_fill_fused: process_depth_host_warp_fused with every warped frame filled before the fusion ->
        list of k FrameResult; with fused=True / warp_stats=True / fill_stats=True / fuse_stats=True a tuple with the fused frames
        (uint16 [k, H, W]), the list of k * n WarpStats, the list of k * n FillStats and / or the list of k FuseStats behind it, in this
        order"""
        total = len(depth)
        arr = _warp_views(views, total)
        return self._depth_host_pre("process_depth_host_warp_fill_fused", depth, int(n), FuseStats, fused, fuse_stats, int(n), arr,
                                    None if dst is None else C.byref(dst), None if fill_rule is None else C.byref(fill_rule),
                                    None if fuse_rule is None else C.byref(fuse_rule), first=[(WarpStats, warp_stats), (FillStats, fill_stats)])

    def locate_camera(self, frames, prior, stair_map, passes=3, rule=None, min_points=200, observable=SP_OBSERVABLE, depth=False):
        """process_host_stair_pose `passes` times over the same frames of ONE camera, each pass starting from the calibration the pass
        before gave (as refine_calibration chains the ground fit).  A pass that does not end GF_OK ends the chain: the last good
        calibration stays in .cal of the returned record, which reports the failing status.  -> (StairPose of the last pass run, the
        list of every pass's StairPose)"""
        cam = Camera.from_buffer_copy(_as_camera(prior))
        maps = _stair_maps(stair_map)[0][0]
        chain = []
        for _ in range(max(int(passes), 1)):
            pose = self.process_host_stair_pose(frames, stair_pose_target(cam, maps), None, rule, min_points, observable, depth)[0]
            chain.append(pose)
            if pose.status != GF_OK:
                break
            cam.cal = pose.cal
        return chain[-1], chain

    # ---- surface fit of cameras batches, drift per camera (include/ssd_hip.h)
    def enqueue_cameras_surface_moments(self, d_ptr, nframes, camera_of_frame, d_moments, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue_cameras_surface_moments: enqueue_cameras (no labels) plus frame i's FrameMoments, under camera
        camera_of_frame[i], at d_moments + i * sizeof(FrameMoments) in device memory; complete when fetch() of the batch returns"""
        idx = self._camera_index(camera_of_frame, nframes)
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        _check(lib().ssd_enqueue_cameras_surface_moments(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                                         idx.ctypes.data_as(C.POINTER(C.c_uint16)), _input_code(depth),
                                                         C.c_void_p(d_moments)))

    def process_host_cameras_surfaces(self, frames, camera_of_frame, depth=False, min_points=200, moments=False):
        """ssd_process_host_cameras_surfaces: frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True), one camera
        index per frame -> (list of FrameResult, list of FrameSurfaces), with moments=True also the list of FrameMoments"""
        a, n, inp = self._frames_arg("process_host_cameras_surfaces", frames, depth)
        idx = self._camera_index(camera_of_frame, n)
        res, mom, out = (FrameResult * n)(), (FrameMoments * n)(), (FrameSurfaces * n)()
        _check(lib().ssd_process_host_cameras_surfaces(self._h, a.ctypes.data_as(C.c_void_p), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                       inp, res, mom if moments else None, int(min_points), out))
        return (list(res), list(out), list(mom)) if moments else (list(res), list(out))

    def camera_drift(self, frames, camera_of_frame, depth=False, min_points=2000, passes=0, k_sigma=2.5, gate_min=0.0, device_gates=False,
                     device_fold=False):
        """process_host_cameras_surfaces, then camera_drift_fold of its moments against the handle's camera table
        -> (list of FrameResult, list of CameraDrift, one per camera of the table).  passes >= 1: the fold of the last refit pass's
        records of process_host_cameras_surfaces_refit(passes, k_sigma, gate_min, device_gates) instead of the first pass's.
        device_fold=True: ssd_process_host_cameras_drift - device gates and the fold on the device, slice by slice, no per-frame record on
        the host; the same outputs as device_gates=True, byte for byte"""
        if not getattr(self, "_cameras", None):
            raise SsdError("camera_drift: the handle has no camera table (set_cameras)")
        if device_fold:
            a, n, inp = self._frames_arg("camera_drift", frames, depth)
            idx = self._camera_index(camera_of_frame, n)
            ncams = len(self._cameras)
            res, out = (FrameResult * n)(), (CameraDrift * ncams)()
            _check(lib().ssd_process_host_cameras_drift(self._h, a.ctypes.data_as(C.c_void_p), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                        inp, res, 200, float(k_sigma), float(gate_min),
                                                        int(passes), int(min_points), out))
            return list(res), [CameraDrift.from_buffer_copy(out[i]) for i in range(ncams)]
        if passes:
            res, _, _, mom = self.process_host_cameras_surfaces_refit(frames, camera_of_frame, depth=depth, k_sigma=k_sigma, gate_min=gate_min,
                                                                      passes=passes, moments=True, device_gates=device_gates)
        else:
            res, _, mom = self.process_host_cameras_surfaces(frames, camera_of_frame, depth=depth, moments=True)
        return res, camera_drift_fold(mom, camera_of_frame, self._cameras, min_points=min_points)

    # ---- trimmed refit of cameras batches (include/ssd_hip.h)
    def enqueue_cameras_surface_refit(self, d_ptr, nframes, gates, d_moments, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue_cameras_surface_refit: enqueue_surface_refit behind the handle's last whole CAMERAS enqueue of the same frames:
        frame i under the camera that enqueue named for it and under gates[i]; complete when fetch_surface_refit() returns"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        arr = None
        if gates is not None:
            arr = gates if isinstance(gates, C.Array) and gates._type_ is FrameGates else (FrameGates * max(1, len(gates)))(*gates)
            if len(arr) < nframes:
                raise SsdError("enqueue_cameras_surface_refit: fewer gates than frames")
        _check(lib().ssd_enqueue_cameras_surface_refit(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                                       _input_code(depth), arr, C.c_void_p(d_moments)))

    def process_host_cameras_surfaces_refit(self, frames, camera_of_frame, depth=False, min_points=200, k_sigma=2.5, gate_min=0.0, passes=1,
                                            moments=False, device_gates=False):
        """ssd_process_host_cameras_surfaces_refit: process_host_surfaces_refit with one camera index per frame
        -> (list of FrameResult, list of FrameSurfaces of the last refit pass), with moments=True also the lists of FrameMoments of
        the first pass and of the last refit pass.  device_gates=True: ssd_process_host_cameras_surfaces_refit_device"""
        a, n, inp = self._frames_arg("process_host_cameras_surfaces_refit", frames, depth)
        idx = self._camera_index(camera_of_frame, n)
        res, first, refit, out = (FrameResult * n)(), (FrameMoments * n)(), (FrameMoments * n)(), (FrameSurfaces * n)()
        fn = lib().ssd_process_host_cameras_surfaces_refit_device if device_gates else lib().ssd_process_host_cameras_surfaces_refit
        _check(fn(self._h, a.ctypes.data_as(C.c_void_p), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)), inp, res,
                  first if moments else None, refit if moments else None, int(min_points), float(k_sigma), float(gate_min), int(passes), out))
        return (list(res), list(out), list(first), list(refit)) if moments else (list(res), list(out))

    # ---- surface gates on the device (include/ssd_hip.h)
    def enqueue_surface_gates(self, d_moments, nframes, d_gates, min_points=200, k_sigma=2.5, gate_min=0.0, stream=None):
        """ssd_enqueue_surface_gates: nframes FrameMoments in device memory -> nframes FrameGates in device memory (frame i's = what
        surface_gates_from_moments gives for record i, byte for byte), on `stream`, without synchronising"""
        _check(lib().ssd_enqueue_surface_gates(self._h, C.c_void_p(d_moments), nframes, C.c_void_p(stream or 0), int(min_points), float(k_sigma),
                                               float(gate_min), C.c_void_p(d_gates)))

    def enqueue_surface_refit_device(self, d_ptr, nframes, d_prev, d_moments, min_points=200, k_sigma=2.5, gate_min=0.0, depth=False,
                                     stride_bytes=None, stream=None):
        """ssd_enqueue_surface_refit_device: enqueue_surface_refit whose gates are made on the device from the nframes FrameMoments at
        d_prev (device memory: the first pass's records, or a refit pass's - d_prev == d_moments is allowed), no host copy, no wait"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        _check(lib().ssd_enqueue_surface_refit_device(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                                      _input_code(depth), C.c_void_p(d_prev), int(min_points),
                                                      float(k_sigma), float(gate_min), C.c_void_p(d_moments)))

    def enqueue_cameras_surface_refit_device(self, d_ptr, nframes, d_prev, d_moments, min_points=200, k_sigma=2.5, gate_min=0.0, depth=False,
                                             stride_bytes=None, stream=None):
        """ssd_enqueue_cameras_surface_refit_device: enqueue_surface_refit_device behind the handle's last whole CAMERAS enqueue"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        _check(lib().ssd_enqueue_cameras_surface_refit_device(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                                              _input_code(depth), C.c_void_p(d_prev), int(min_points),
                                                              float(k_sigma), float(gate_min), C.c_void_p(d_moments)))

    # ---- camera fold on the device (include/ssd_hip.h)
    def enqueue_camera_fold(self, d_moments, d_camera_of_frame, nframes, ncams, d_fold, accumulate=False, stream=None):
        """ssd_enqueue_camera_fold: nframes FrameMoments and one int32 camera index per frame, both in device memory -> ncams CameraFold
        in device memory (record c = the head of camera_drift_fold's record c, byte for byte; accumulate: on top of what d_fold holds),
        on `stream`, without synchronising"""
        _check(lib().ssd_enqueue_camera_fold(self._h, C.c_void_p(d_moments), C.c_void_p(d_camera_of_frame), int(nframes), int(ncams),
                                             1 if accumulate else 0, C.c_void_p(stream or 0), C.c_void_p(d_fold)))

    def enqueue_camera_ground_gates(self, d_moments, d_camera_of_frame, nframes, d_fold, ncams, d_gates, fold_min_points=2000, k_sigma=2.5,
                                    gate_min=0.0, stream=None):
        """ssd_enqueue_camera_ground_gates: camera_ground_gates on the device - g[0] of every frame with a ground whose camera's fold
        (d_fold, ncams CameraFold in device memory) solves GF_OK under fold_min_points becomes that plane with
        max(k_sigma * rms, gate_min); d_gates: nframes FrameGates in device memory, in/out"""
        _check(lib().ssd_enqueue_camera_ground_gates(self._h, C.c_void_p(d_moments), C.c_void_p(d_camera_of_frame), int(nframes), C.c_void_p(d_fold),
                                                     int(ncams), int(fold_min_points), float(k_sigma), float(gate_min), C.c_void_p(stream or 0),
                                                     C.c_void_p(d_gates)))

    def enqueue_cameras_surface_refit_folded(self, d_ptr, nframes, d_prev, d_moments, min_points=200, k_sigma=2.5, gate_min=0.0,
                                             fold_min_points=2000, depth=False, stride_bytes=None, stream=None):
        """ssd_enqueue_cameras_surface_refit_folded: enqueue_cameras_surface_refit_device with the camera's gate - the records at d_prev
        are also folded per camera on the device and every frame's ground gate becomes its camera's plane, no host copy, no wait"""
        frame = self.cfg.width * self.cfg.height * (2 if depth else 12)
        _check(lib().ssd_enqueue_cameras_surface_refit_folded(self._h, C.c_void_p(d_ptr), stride_bytes or frame, nframes, C.c_void_p(stream or 0),
                                                              _input_code(depth), C.c_void_p(d_prev), int(min_points),
                                                              float(k_sigma), float(gate_min), int(fold_min_points), C.c_void_p(d_moments)))

    def camera_drift_resident(self, d_ptr, nframes, camera_of_frame, depth=False, min_points=200, fold_min_points=2000, passes=2, k_sigma=2.5,
                              gate_min=0.0, camera_gate=True):
        """The drift watch on frames in device memory, no per-frame record on the host: enqueue_cameras_surface_moments, `passes`
        device-gated refits behind it - the last one with the camera's gate (enqueue_cameras_surface_refit_folded) when camera_gate -,
        the fold of the last records on the device, one fetch of the table's CameraFold records and camera_drift_from_fold
        -> (list of FrameResult, list of CameraDrift, one per camera of the table)"""
        if not getattr(self, "_cameras", None):
            raise SsdError("camera_drift_resident: the handle has no camera table (set_cameras)")
        idx = self._camera_index(camera_of_frame, nframes)
        ncams, dev, rec = len(self._cameras), self.device, C.sizeof(FrameMoments) * nframes
        bufs = []
        try:
            for nbytes in (rec, rec, 4 * nframes, C.sizeof(CameraFold) * ncams):
                p = C.c_void_p()
                _check(lib().ssd_device_alloc(dev, nbytes, C.byref(p)))
                bufs.append(p)
            d_first, d_refit, d_idx, d_fold = (b.value for b in bufs)
            idx32 = idx.astype(np.int32)
            _check(lib().ssd_device_upload(dev, C.c_void_p(d_idx), idx32.ctypes.data_as(C.c_void_p), idx32.nbytes))
            self.enqueue_cameras_surface_moments(d_ptr, nframes, idx, d_first, depth=depth)
            for p in range(passes):
                refit = self.enqueue_cameras_surface_refit_folded if camera_gate and p == passes - 1 else self.enqueue_cameras_surface_refit_device
                kw = dict(fold_min_points=fold_min_points) if camera_gate and p == passes - 1 else {}
                refit(d_ptr, nframes, d_first if p == 0 else d_refit, d_refit, min_points=min_points, k_sigma=k_sigma, gate_min=gate_min, depth=depth, **kw)
            res = self.fetch_list(nframes)
            if passes:
                self.fetch_surface_refit()          # the pass ran on its workspace's stream: the fold below goes behind it
            self.enqueue_camera_fold(d_refit if passes else d_first, d_idx, nframes, ncams, d_fold)
            fold = (CameraFold * ncams)()
            _check(lib().ssd_device_download(dev, fold, C.c_void_p(d_fold), C.sizeof(fold)))
            return res, camera_drift_from_fold(fold, self._cameras, min_points=fold_min_points)
        finally:
            lib().ssd_device_sync(dev)              # nothing enqueued above still reads the buffers
            for b in bufs:
                lib().ssd_device_free(dev, b)

    def surface_moments_time_ms(self, back=0):
        """Device time of the surface-moments pass of the enqueue `back` calls ago (0.0: it gathered none); timing must be on."""
        return _time_ms(lib().ssd_get_surface_moments_time_back, self._h, back)

    def labels_time_ms(self, back=0):
        """Device time of the label kernel of the enqueue `back` calls ago (0.0: it wrote no labels); timing must be on."""
        return _time_ms(lib().ssd_get_labels_time_back, self._h, back)

    def fetch(self, nframes, stream=None, back=0):
        """Waits for the last enqueue (back = 1: the one before it, so that the next batch can already be running) and
        returns its results (an indexable ctypes array of FrameResult; the buffer is reused by the next fetch of the
        same size)."""
        if getattr(self, "_res_n", 0) != nframes:
            self._res, self._res_n = (FrameResult * nframes)(), nframes
        _check(lib().ssd_fetch_back(self._h, self._res, nframes, back))
        return self._res

    def fetch_list(self, nframes, stream=None):
        """fetch() as a list of independent FrameResult copies."""
        return [FrameResult.from_buffer_copy(r) for r in self.fetch(nframes, stream)]

    def set_single_pass(self, on=True):
        """ssd_set_single_pass: off = the handle gives the planes' memory back and stays on two passes; on = the default again"""
        _check(lib().ssd_set_single_pass(self._h, 1 if on else 0))

    def set_risers(self, on=True, tolerance=0.03, min_support=200):
        """extension: also gather the evidence of the vertical faces (ssd_set_risers)"""
        _check(lib().ssd_set_risers(self._h, 1 if on else 0, tolerance, min_support))

    def fetch_risers(self, nframes, stream=None):
        """-> list of FrameRisers (independent copies) of the last enqueue / process_host batch"""
        arr = (FrameRisers * nframes)()
        _check(lib().ssd_fetch_risers(self._h, arr, nframes, C.c_void_p(stream or 0)))
        return [FrameRisers.from_buffer_copy(bytes(r)) for r in arr]

    # ---- riser fit: plane, lean and going of every vertical face (include/ssd_hip.h)
    def set_riser_moments(self, on=True):
        """ssd_set_riser_moments: while on (and risers are on) every riser pass also gathers each riser's exact integer moments"""
        _check(lib().ssd_set_riser_moments(self._h, 1 if on else 0))

    def set_riser_labels(self, on=True):
        """ssd_set_riser_labels: while on (and risers are on) every call that writes labels also writes LABEL_RISER_BASE + i into the
        byte of every evidence point of riser i"""
        _check(lib().ssd_set_riser_labels(self._h, 1 if on else 0))

    def riser_labels_time_ms(self, back=0):
        """Device time of the riser labels' kernel of the enqueue `back` calls ago (0.0: it marked nothing); timing must be on."""
        return _time_ms(lib().ssd_get_riser_labels_time_back, self._h, back)

    def fetch_riser_moments(self, nframes, stream=None):
        """-> list of FrameMoments (independent copies; record i = riser i) of the last enqueue / host batch"""
        arr = (FrameMoments * max(1, nframes))()
        _check(lib().ssd_fetch_riser_moments(self._h, arr, nframes, C.c_void_p(stream or 0)))
        return [FrameMoments.from_buffer_copy(arr[i]) for i in range(nframes)]

    def _host_riser_fits(self, who, frames, camera_of_frame, depth, min_points, moments):
        a, n, inp = self._frames_arg(who, frames, depth)
        res, ris, mom, out = (FrameResult * n)(), (FrameRisers * n)(), (FrameMoments * n)(), (FrameRiserFits * n)()
        if camera_of_frame is None:
            _check(lib().ssd_process_host_riser_fits(self._h, a.ctypes.data_as(C.c_void_p), n, inp, res, ris, mom if moments else None,
                                                     int(min_points), out))
        else:
            idx = self._camera_index(camera_of_frame, n)
            _check(lib().ssd_process_host_cameras_riser_fits(self._h, a.ctypes.data_as(C.c_void_p), n, idx.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                             inp, res, ris, mom if moments else None, int(min_points), out))
        return (list(res), list(ris), list(out), list(mom)) if moments else (list(res), list(ris), list(out))

    def process_host_riser_fits(self, frames, depth=False, min_points=100, moments=False):
        """ssd_process_host_riser_fits (risers must be on): frames on the host (float32 [n, H, W, 3], or uint16 [n, H, W] with depth=True)
        -> (list of FrameResult, list of FrameRisers, list of FrameRiserFits), with moments=True also the list of FrameMoments"""
        return self._host_riser_fits("process_host_riser_fits", frames, None, depth, min_points, moments)

    def process_host_cameras_riser_fits(self, frames, camera_of_frame, depth=False, min_points=100, moments=False):
        """ssd_process_host_cameras_riser_fits: the same for a cameras batch, one camera index per frame, each frame solved under its own
        camera's calibration"""
        return self._host_riser_fits("process_host_cameras_riser_fits", frames, camera_of_frame, depth, min_points, moments)

    def set_timing(self, on=True):
        _check(lib().ssd_set_timing(self._h, 1 if on else 0))

    def stage_times_ms(self, back=0):
        """Device time per stage of the enqueue `back` calls ago (HIP events on the kernels' stream)."""
        ms = (C.c_float * 7)()
        _check(lib().ssd_get_stage_times_back(self._h, back, ms))
        return dict(zip(STAGE_NAMES, [float(x) for x in ms]))

    def predict_time_ms(self, back=0):
        """Device time of k_predict, the kernel in front of the stages of a single-pass batch (0.0: the enqueue did not run it)."""
        return _time_ms(lib().ssd_get_predict_time_back, self._h, back)

    def set_debug(self, on=True, images=True):
        """debug capture: records + images (the whole ground image is rastered for it), or records only (images=False:
        the kernels run exactly as in production)"""
        _check(lib().ssd_set_debug(self._h, (1 if images else 2) if on else 0))

    def debug(self, frame=0):
        d = DebugFrame()
        _check(lib().ssd_get_debug(self._h, frame, C.byref(d)))
        return d

    def frame_state(self, frame):
        """test hook: raw device state of one frame after the last enqueue -> (bytes, layout dict)"""
        lay = (C.c_longlong * 8)()
        buf = C.create_string_buffer(1 << 16)
        n = _check(hooks_lib().ssd_test_frame_state(self._h, frame, buf, len(buf), lay), "hooks")
        names = ("size", "hist", "lut", "boxes", "plateaus", "quad_tests", "sum_z", "cnt")
        return buf.raw[:n], dict(zip(names, [int(x) for x in lay]))

    def empty_quadrilateral(self, frame, surface):
        """test hook: rewrites the sums of a surface (-1 = ground, else plateau index) as if its quadrilateral had accepted no point"""
        _check(hooks_lib().ssd_test_empty_quadrilateral(self._h, frame, surface), "hooks")

    def single_pass(self, mode, sabotage=0):
        """test hook: the single pass (K1 rasters the step plateaus itself) -1 = as the product decides, 0 = never, 1 = whenever the
        geometry allows; sabotage 1 / 2 = the predictor's planes in the wrong bins / none (every frame must fall back to k_raster)"""
        _check(hooks_lib().ssd_test_single_pass(self._h, mode, sabotage), "hooks")

    def plane_pool(self, planes=-1):
        """test hook: the planes k_predict may hand out per batch (-1: all the workspace holds); returns the pool's size"""
        return _check(hooks_lib().ssd_test_plane_pool(self._h, planes), "hooks")

    def single_pass_stats(self, frames, scan_planes=True):
        """test hook, of the last enqueue: {'ran': it ran the single pass, 'covered': frames whose step plateaus the planes covered,
        'with_steps': frames with step plateaus, 'planes': planes over all frames, 'dirty_words': words of the lane's plane images
        that are not zero (-1 with scan_planes=False: the images are not fetched)}"""
        counts = (C.c_longlong * 4)()
        ran = _check(hooks_lib().ssd_test_single_pass_stats(self._h, frames, 1 if scan_planes else 0, counts), "hooks")
        return dict(ran=bool(ran), covered=int(counts[0]), with_steps=int(counts[1]), planes=int(counts[2]), dirty_words=int(counts[3]))

    def single_pass_frame(self, frame):
        """test hook, one frame of the last enqueue: (plane of each height bin as a uint8 array, 255 = none; planes; covered; step plateaus)"""
        table = (C.c_uint8 * MAX_BINS)()
        info = (C.c_int32 * 3)()
        _check(hooks_lib().ssd_test_single_pass_frame(self._h, frame, table, info), "hooks")
        return np.frombuffer(bytes(table), dtype=np.uint8).copy(), int(info[0]), bool(info[1]), int(info[2])

    def single_pass_sample(self, frame):
        """test hook: the sample histogram k_predict made the frame's table of (uint32[MAX_BINS])"""
        out = np.zeros(MAX_BINS, dtype=np.uint32)
        _check(hooks_lib().ssd_test_single_pass_sample(self._h, frame, out.ctypes.data_as(C.c_void_p)), "hooks")
        return out

    def record_offset(self, offset_bytes):
        """tools hook: where the first workspace's cell records lie inside their allocation"""
        _check(hooks_lib().ssd_test_record_offset(self._h, offset_bytes), "hooks")

    def record_realloc(self, extra_bytes=0, offset_bytes=0):
        """tools hook: a newly allocated array for the first workspace's cell records (optionally inside a larger allocation);
        returns its device address"""
        return int(hooks_lib().ssd_test_record_realloc_sized(self._h, extra_bytes, offset_bytes))

    def ground_image_raw(self, frame):
        """test hook: the ground bit image as it lies in the last enqueue's workspace (height x width bytes)"""
        out = np.empty((self.cfg.height, self.cfg.width), dtype=np.uint8)
        _check(hooks_lib().ssd_test_ground_image(self._h, frame, out.ctypes.data_as(C.c_void_p)), "hooks")
        return out

    def debug_image(self, frame, step_slot, closed):
        out = np.empty((self.cfg.height, self.cfg.width), dtype=np.uint8)
        _check(lib().ssd_get_debug_image(self._h, frame, step_slot, 1 if closed else 0, out.ctypes.data_as(C.c_void_p)))
        return out


class Pipeline:
    """ssd_pipeline_*: `depth` handles on `depth` streams, batches dealt out round-robin, results in submission order."""

    def __init__(self, cfg, trans, device=0, depth=2):
        self.cfg, self.depth = cfg, depth
        self._p = C.c_void_p()
        cal = trans.constants if isinstance(trans, GeometricTransformation) else trans
        rc = lib().ssd_pipeline_create(C.byref(cfg), C.byref(cal), device, depth, C.byref(self._p))
        if rc < 0:
            raise SsdError("ssd_pipeline_create: %d: %s" % (rc, lib().ssd_pipeline_last_error().decode()))
        self._res = (FrameResult * cfg.max_frames_per_batch)()

    def submit(self, d_ptr, nframes, stride_bytes=None, after_stream=False):
        """after_stream: False = the frames are complete; None / an integer hipStream_t = order the batch behind that stream"""
        stride = stride_bytes or self.cfg.width * self.cfg.height * 12
        if after_stream is False:
            rc = lib().ssd_pipeline_submit(self._p, C.c_void_p(d_ptr), stride, nframes)
        else:
            rc = lib().ssd_pipeline_submit_after(self._p, C.c_void_p(d_ptr), stride, nframes, C.c_void_p(after_stream or 0), 1)
        if rc < 0:
            raise SsdError("ssd_pipeline_submit: %d: %s" % (rc, lib().ssd_pipeline_last_error().decode()))

    def pending(self):
        return lib().ssd_pipeline_pending(self._p)

    def next(self, copy=True):
        """-> the oldest unfetched batch's results: a list of independent FrameResult copies, or (copy=False) the frame count
        with the results left in self.results (reused by the next call)"""
        n = C.c_int(0)
        rc = lib().ssd_pipeline_next(self._p, self._res, len(self._res), C.byref(n))
        if rc < 0:
            raise SsdError("ssd_pipeline_next: %d: %s" % (rc, lib().ssd_pipeline_last_error().decode()))
        if not copy:
            return n.value
        return [FrameResult.from_buffer_copy(self._res[i]) for i in range(n.value)]

    @property
    def results(self):
        return self._res

    def set_timing(self, on=True):
        rc = lib().ssd_pipeline_set_timing(self._p, 1 if on else 0)
        if rc < 0:
            raise SsdError("ssd_pipeline_set_timing: %d: %s" % (rc, lib().ssd_pipeline_last_error().decode()))

    def stage_times_ms(self):
        """Device time per stage of the batch next() returned last (call right after next())."""
        ms = (C.c_float * 7)()
        rc = lib().ssd_pipeline_stage_times(self._p, ms)
        if rc < 0:
            raise SsdError("ssd_pipeline_stage_times: %d: %s" % (rc, lib().ssd_pipeline_last_error().decode()))
        return dict(zip(STAGE_NAMES, [float(v) for v in ms]))

    def close(self):
        if self._p:
            lib().ssd_pipeline_destroy(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pointcloud:
    """reference pointcloud.h:32-42: ``Pointcloud(window, trans).process(frame)`` prints one line."""

    def __init__(self, window, trans, device=0):
        self._window, self._trans, self._device = window, trans, device
        self._det = None

    def detect(self, frame):
        a = np.asarray(frame, dtype=np.float32)
        h, w = a.shape[0], a.shape[1]
        if self._det is None or (self._det.cfg.width, self._det.cfg.height) != (w, h):
            self._det = Detector(default_config(w, h, max_frames_per_batch=1), self._trans, self._device)
        st = Stairs(self._det.process_host(a)[0])
        if st.status & ST_THROW:
            raise ValueError("Quadrilateral is not usable (reference quadrilateralTest.cpp:283-372 throws)")
        return st

    def process(self, frame):
        print(self.detect(frame).serialize(), flush=True)


# --------------------------------------------------------------------------- synthetic frame source
def stream_read_ms(d_ptr, nbytes, reps=5, device=0, stream=None):
    """Average milliseconds of a plain read stream over nbytes at d_ptr (measurement hook, libssd_testhooks.so)."""
    ms = C.c_float(0.0)
    _check(hooks_lib().ssd_test_stream_read(device, C.c_void_p(d_ptr), nbytes, reps, C.c_void_p(stream), C.byref(ms)), "hooks")
    return float(ms.value)


def line_host(pq):
    """test hook: the kernels' line through two points -> (abc as doubles, abc as int32 from the truncated coordinates)"""
    a = np.ascontiguousarray(pq, dtype=np.float64).reshape(4)
    d, i = np.zeros(3), np.zeros(3, dtype=np.int32)
    _check(hooks_lib().ssd_test_line_host(a.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p)), "hooks")
    return d, i


def intersect_host(l, o):
    """test hook: the kernels' Line<double>::intersection -> (found, x, y)"""
    a, b, xy = np.ascontiguousarray(l, dtype=np.float64), np.ascontiguousarray(o, dtype=np.float64), np.zeros(2)
    rc = _check(hooks_lib().ssd_test_intersect_host(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p)), "hooks")
    return bool(rc), float(xy[0]), float(xy[1])


def sort_perm(dist, device=None):
    """test hook: libstdc++'s std::sort restated (csrc/ssd_sort.h), on the host (device=None) or on a GPU"""
    d = np.ascontiguousarray(dist, dtype=np.float64)
    perm = np.zeros(len(d), dtype=np.int32)
    if device is None:
        _check(hooks_lib().ssd_test_sort_host(d.ctypes.data_as(C.c_void_p), len(d), perm.ctypes.data_as(C.c_void_p)), "hooks")
    else:
        _check(hooks_lib().ssd_test_sort_device(device, d.ctypes.data_as(C.c_void_p), len(d), perm.ctypes.data_as(C.c_void_p)), "hooks")
    return perm


def quad_test_device(quad, pts, device=0):
    """test hook: the kernels' QuadrilateralTest on one quadrilateral -> (err code, uint8 inside[n])"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(len(p), dtype=np.uint8)
    err = C.c_int(0)
    _check(hooks_lib().ssd_test_quad_device(device, q.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), len(p),
                                            out.ctypes.data_as(C.c_void_p), C.byref(err)), "hooks")
    return err.value, out


def closing_host(img, x0, x_step, y_from=0, band_rows=16, want_closed=True):
    """test hook: the kernels' closing compiled for the host -> (closed uint8 image or None, first[], last[]) for the pixel
    columns x0, x0 + x_step, .. (rows y_from..)"""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = a.shape
    n = (w - 1 - x0) // x_step + 1 if w > x0 else 0
    closed = np.zeros_like(a) if want_closed else None
    first = np.zeros(max(n, 1), dtype=np.int32)
    last = np.zeros(max(n, 1), dtype=np.int32)
    _check(hooks_lib().ssd_test_closing_host(a.ctypes.data_as(C.c_void_p), w, h, x0, x_step, y_from, band_rows,
                                             closed.ctypes.data_as(C.c_void_p) if want_closed else None,
                                             first.ctypes.data_as(C.c_void_p), last.ctypes.data_as(C.c_void_p), n), "hooks")
    return closed, first[:n], last[:n]


def best_line_host(pts, form):
    """test hook: BestLine with the kernels' residual code compiled for the host -> (a, b, c)"""
    p = np.ascontiguousarray(pts, dtype=np.int32).reshape(-1, 2)
    out = np.zeros(3, dtype=np.int32)
    _check(hooks_lib().ssd_test_best_line_host(p.ctypes.data_as(C.c_void_p), len(p), form, out.ctypes.data_as(C.c_void_p)), "hooks")
    return tuple(int(v) for v in out)


def quad_test_host(quad, pts):
    """test hook: the same QuadrilateralTest code compiled for the host (no GPU) -> (err code, uint8 inside[n])"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(len(p), dtype=np.uint8)
    err = C.c_int(0)
    _check(hooks_lib().ssd_test_quad_host(q.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), len(p),
                                          out.ctypes.data_as(C.c_void_p), C.byref(err)), "hooks")
    return err.value, out


def grid_boxes_device(quad, x_min, y_min, box_x, box_y, boxes, device=0):
    """test hook: k_inquad's "box of K1's grid wholly inside the quadrilateral" -> (usable, uint8 inside[n])"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    out = np.zeros(len(b), dtype=np.uint8)
    usable = C.c_int(0)
    _check(hooks_lib().ssd_test_grid_boxes_device(device, q.ctypes.data_as(C.c_void_p), x_min, y_min, box_x, box_y,
                                                  b.ctypes.data_as(C.c_void_p), len(b), out.ctypes.data_as(C.c_void_p),
                                                  C.byref(usable)), "hooks")
    return usable.value, out


def make_scene(width, height, n_steps=3, seed=12345, cam_height=1.0, pitch_deg=50.0, roll_deg=0.0,
               first_riser_y=0.45, tread=0.28, rise=0.17, stair_width=0.8, landing=1.0, yaw_deg=0.0,
               sigma=0.001, outlier_frac=0.0, outlier_min=0.3, outlier_max=3.0, invalid_frac=0.0,
               max_range=9.0, hfov_deg=70.0, vfov_deg=55.0):
    """L515-shaped pinhole looking down at a staircase (SURVEY.md section 8(d) recipe)."""
    s = Scene()
    s.width, s.height = width, height
    s.fx = (width / 2.0) / math.tan(math.radians(hfov_deg / 2.0))
    s.fy = (height / 2.0) / math.tan(math.radians(vfov_deg / 2.0))
    s.cx, s.cy = (width - 1) / 2.0, (height - 1) / 2.0
    s.cam_height = cam_height
    p, r = math.radians(pitch_deg), math.radians(roll_deg)
    fwd = np.array([0.0, math.cos(p), -math.sin(p)])
    right0 = np.array([1.0, 0.0, 0.0])
    down0 = np.cross(fwd, right0)
    right = math.cos(r) * right0 + math.sin(r) * down0
    down = np.cross(fwd, right)
    s.axis_right[:] = list(right)
    s.axis_down[:] = list(down)
    s.axis_fwd[:] = list(fwd)
    s.n_steps = n_steps
    s.first_riser_y, s.tread, s.rise, s.stair_width, s.landing = first_riser_y, tread, rise, stair_width, landing
    s.yaw_cos, s.yaw_sin = math.cos(math.radians(yaw_deg)), math.sin(math.radians(yaw_deg))
    s.sigma = sigma
    s.outlier_frac, s.outlier_min, s.outlier_max = outlier_frac, outlier_min, outlier_max
    s.invalid_frac, s.max_range = invalid_frac, max_range
    s.seed = seed
    return s


def scene_array(scenes):
    arr = (Scene * len(scenes))()
    for i, s in enumerate(scenes):
        C.memmove(C.byref(arr[i]), C.byref(s), C.sizeof(Scene))
    return arr


def synth_host(scenes):
    """-> float32 [n, H, W, 3]; runs on the host, no GPU needed; bit-identical to the device generator."""
    arr = scene_array(scenes)
    h, w = scenes[0].height, scenes[0].width
    out = np.empty((len(scenes), h, w, 3), dtype=np.float32)
    _check(source_lib().ssd_synth_generate_host(arr, len(scenes), out.ctypes.data_as(C.c_void_p)), "source")
    return out


def intrinsics_for_scene(scene, depth_units=0.00025):
    """rs2_intrinsics of the synthetic camera (L515 depth unit: 0.25 mm)."""
    i = Intrinsics()
    i.fx, i.fy, i.ppx, i.ppy, i.depth_units = scene.fx, scene.fy, scene.cx, scene.cy, depth_units
    return i


def synth_depth_host(scenes, depth_units=0.00025):
    """-> uint16 [n, H, W]: the scenes as 16-bit depth frames; host, bit-identical to the device generator."""
    arr = scene_array(scenes)
    out = np.empty((len(scenes), scenes[0].height, scenes[0].width), dtype=np.uint16)
    _check(source_lib().ssd_synth_depth_host(arr, len(scenes), depth_units, out.ctypes.data_as(C.c_void_p)), "source")
    return out


def synth_depth_device(scenes, d_ptr, depth_units=0.00025, stride_bytes=None, device=0, stream=None):
    arr = scene_array(scenes)
    stride = stride_bytes or scenes[0].width * scenes[0].height * 2
    _check(source_lib().ssd_synth_depth_device(arr, len(scenes), depth_units, C.c_void_p(d_ptr), stride, device, C.c_void_p(stream or 0)), "source")


def deproject_host(intr, depth):
    """rs2::pointcloud::calculate restated (host): uint16 [H, W] -> float32 [H, W, 3]."""
    a = np.ascontiguousarray(depth, dtype=np.uint16)
    out = np.empty(a.shape + (3,), dtype=np.float32)
    _check(lib().ssd_deproject_host(C.byref(intr), a.shape[1], a.shape[0], a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def synth_device(scenes, d_ptr, stride_bytes=None, device=0, stream=None):
    arr = scene_array(scenes)
    stride = stride_bytes or scenes[0].width * scenes[0].height * 12
    _check(source_lib().ssd_synth_generate_device(arr, len(scenes), C.c_void_p(d_ptr), stride, device, C.c_void_p(stream or 0)), "source")


CALIBRATION_MARKS = ((-0.35, 0.9, 0.0), (0.35, 0.9, 0.0), (0.2, 0.35, 0.0))


def calibration_points(scene, marks=CALIBRATION_MARKS, world_offset=(0.0, 0.0, 0.004)):
    """Three ground marks: (external-world points, camera points) as the calibration files would hold them."""
    world, cam = [], []
    for m in marks:
        p = (C.c_double * 3)(*m)
        o = (C.c_double * 3)()
        _check(source_lib().ssd_synth_scene_to_camera(C.byref(scene), p, o), "source")
        cam.append([o[0], o[1], o[2]])
        world.append([m[0] + world_offset[0], m[1] + world_offset[1], m[2] + world_offset[2]])
    return np.array(world), np.array(cam)


def transformation_for_scene(scene):
    world, cam = calibration_points(scene)
    return GeometricTransformation(world, cam)


def prez_host(x_min, x_max, y_min, y_max, z_min, z_max, a, b, height_interval=0.01, width=1024, height=768):
    """test hook: the constants of K1's single-precision z row / bin and candidate pixel (csrc/ssd_prexy.h: make_pre_z, make_pre_pixel)"""
    rng = (C.c_double * 6)(x_min, x_max, y_min, y_max, z_min, z_max)
    aa = (C.c_double * 9)(*[float(v) for v in np.asarray(a, dtype=np.float64).reshape(9)])
    bb = (C.c_double * 3)(*[float(v) for v in np.asarray(b, dtype=np.float64).reshape(3)])
    out = (C.c_float * 16)()
    _check(hooks_lib().ssd_test_prez_host(rng, aa, bb, float(height_interval), int(width), int(height), out), "hooks")
    o = np.array(list(out), dtype=np.float32)
    return dict(zc=o[:4], z_neg_k=o[4], z_h0=o[5], z_top=o[6], z_check_top=bool(o[7]), f_w=o[8], f_half_w=o[9], f_neg_h=o[10], f_half_h=o[11],
                px_neg_k=o[12], px_h0=o[13], recip=float(o[14]))


def quad_edges_host(quad, x_min, x_max, y_min, y_max, z_min, z_max, a, b, pts_xyz):
    """test hook: k_inquad's single-precision edge tests of one quadrilateral (csrc/ssd_quadtest.h: build_quad_edges) on camera points ->
    dict(err, gx, gy, g2, m, d_k, d_e0, cls = int8[n] (+1 / -1 / 0), world_xy = float64[n, 2], in_range_xy = uint8[n])"""
    q = np.ascontiguousarray(quad, dtype=np.float64).reshape(8)
    rng = (C.c_double * 6)(x_min, x_max, y_min, y_max, z_min, z_max)
    aa = (C.c_double * 9)(*[float(v) for v in np.asarray(a, dtype=np.float64).reshape(9)])
    bb = (C.c_double * 3)(*[float(v) for v in np.asarray(b, dtype=np.float64).reshape(3)])
    p = np.ascontiguousarray(pts_xyz, dtype=np.float32).reshape(-1, 3)
    consts = (C.c_float * 15)()
    cls = np.zeros(len(p), dtype=np.int8)
    wxy = np.zeros((len(p), 2), dtype=np.float64)
    inr = np.zeros(len(p), dtype=np.uint8)
    err = C.c_int(0)
    _check(hooks_lib().ssd_test_quad_edges_host(q.ctypes.data_as(C.c_void_p), rng, aa, bb, p.ctypes.data_as(C.c_void_p), len(p), consts,
                                               cls.ctypes.data_as(C.c_void_p), wxy.ctypes.data_as(C.c_void_p), inr.ctypes.data_as(C.c_void_p),
                                               C.byref(err)), "hooks")
    o = np.array(list(consts), dtype=np.float32)
    return dict(err=err.value, gx=o[0:4], gy=o[4:8], g2=o[8:12], m=o[12], d_k=o[13], d_e0=o[14], cls=cls, world_xy=wxy, in_range_xy=inr)


def quad_edges_device(quads, x_min, x_max, y_min, y_max, device=0):
    """test hook: k_inquad's edge table as the device builds it in k_quads' three steps, for n quadrilaterals -> float32[n, 13] (gx, gy, g2, m)"""
    q = np.ascontiguousarray(quads, dtype=np.float64).reshape(-1, 8)
    rng = (C.c_double * 4)(x_min, x_max, y_min, y_max)
    out = np.zeros((len(q), 13), dtype=np.float32)
    _check(hooks_lib().ssd_test_quad_edges_device(device, q.ctypes.data_as(C.c_void_p), len(q), rng, out.ctypes.data_as(C.c_void_p)), "hooks")
    return out


def prexy_host(x_min, x_max, y_min, y_max, z_min, z_max, a, b):
    """test hook: the constants of K1's single-precision pre-filter (csrc/ssd_prexy.h) for a measuring range and a calibration:
    dict(c = 4 x 2 float32 coefficients, lo, hi, max_input, box_lo, box_hi, check_input)"""
    rng = (C.c_double * 6)(x_min, x_max, y_min, y_max, z_min, z_max)
    aa = (C.c_double * 9)(*[float(v) for v in np.asarray(a, dtype=np.float64).reshape(9)])
    bb = (C.c_double * 3)(*[float(v) for v in np.asarray(b, dtype=np.float64).reshape(3)])
    out = (C.c_float * 14)()
    _check(hooks_lib().ssd_test_prexy_host(rng, aa, bb, out), "hooks")
    o = np.array(list(out), dtype=np.float32)
    return dict(c=o[:8].reshape(4, 2), lo=o[8], hi=o[9], max_input=o[10], box_lo=o[11], box_hi=o[12], check_input=bool(o[13]))


class PinnedArray:
    """A numpy array over page-locked host memory (ssd_host_alloc): ssd_process_host copies it by DMA without staging."""

    def __init__(self, shape, dtype):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        _check(lib().ssd_host_alloc(self.nbytes, C.byref(p)))
        self.ptr = p.value
        self.array = np.frombuffer((C.c_uint8 * self.nbytes).from_address(self.ptr), dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().ssd_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    """hipMalloc'd bytes through the C ABI (for hosts without torch)."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = device, nbytes
        p = C.c_void_p()
        _check(lib().ssd_device_alloc(device, nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, array, offset=0):
        a = np.ascontiguousarray(array)
        _check(lib().ssd_device_upload(self.device, C.c_void_p(self.ptr + offset), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def download(self, nbytes, offset=0, dtype=np.uint8):
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        _check(lib().ssd_device_download(self.device, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr + offset), nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().ssd_device_free(self.device, C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
