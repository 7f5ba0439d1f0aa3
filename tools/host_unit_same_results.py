#!/usr/bin/env python3
"""tools/host_unit_same_results.py A.so B.so - the handle-free entry points of two builds of libssd_hip.so (csrc/ssd_host.cpp: the
configuration, the calibrations, the host statements, the solvers and folds, the label split, the serializer) give the same bytes.

One child process per library (SSD_HIP_LIB), each calling every such entry point on fixed inputs - the 96 x 72 three-step staircase of
tools/stair_pose_sanitize.cpp as vertices and as 16-bit depth, and the records the host statements make of it - and at least one
refusal per entry point; a line per call: its name, the return code, a digest of every byte it wrote, and for a refusal the text of
ssd_last_error.  The two lists must be equal.  Needs no device (nothing here opens one) and loads nothing but the library.
Exit status 0 and "verdict: identical" when they are."""
import ctypes as C
import hashlib
import importlib
import math
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 72


def staircase(ssd, truth):
    """the frame of tools/stair_pose_sanitize.cpp: (vertices float32 [H*W, 3], depth uint16 [H*W], labels uint8 [H*W]: tread k -> k + 1)"""
    import numpy as np
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    s = (v + 0.5) / H * 5.0
    part = s.astype(np.int64)
    f = s - part
    wx = -0.38 + 0.76 * u / (W - 1)
    tread = part % 2 == 0
    wy = np.where(tread, 0.2 + 0.3 * (part // 2) + 0.04 + 0.22 * f, 0.2 + 0.3 * ((part + 1) // 2))
    wz = np.where(tread, 0.16 * (part // 2), 0.16 * (part // 2) + 0.05 + 0.06 * f)
    a, b = np.array(truth.a[:]).reshape(3, 3), np.array(truth.b[:])
    w = np.stack([wx - b[0], wy - b[1], wz - b[2]], axis=-1)
    xyz = np.stack([a[0, j] * w[..., 0] + a[1, j] * w[..., 1] + a[2, j] * w[..., 2] for j in range(3)], axis=-1)
    xyz = np.ascontiguousarray(xyz.reshape(-1, 3).astype(np.float32))
    depth = np.rint(xyz[:, 2] / np.float32(0.00025)).astype(np.uint16)
    depth[0], depth[1] = 0, 65535
    labels = np.where(tread, part // 2 + 1, 0).astype(np.uint8).reshape(-1)
    return xyz, np.ascontiguousarray(depth), np.ascontiguousarray(labels)


def child():
    import numpy as np
    sys.path.insert(0, ROOT)
    ssd = importlib.import_module("stair-step-detector_amd")
    L = ssd.lib()
    lines = []

    def digest(*outs):
        h = hashlib.sha256()
        for o in outs:
            h.update(o.tobytes() if isinstance(o, np.ndarray) else bytes(o))
        return h.hexdigest()[:24]

    def call(name, rc, *outs):
        text = " | " + L.ssd_last_error().decode() if rc < 0 else ""
        lines.append("%-44s rc %4d  %s%s" % (name, rc, digest(*outs), text))
        return rc

    def ptr(a):
        return a.ctypes.data if a is not None else None

    # the configuration and the calibrations
    cfg = ssd.Config()
    call("default_config", L.ssd_default_config(cfg, W, H), cfg)
    call("default_config: width 0", L.ssd_default_config(cfg, 0, H))
    ident, truth = ssd.Calibration(), ssd.Calibration()
    call("calibration_identity", L.ssd_calibration_identity(ident), ident)
    call("calibration_identity: null", L.ssd_calibration_identity(None))
    pitch = 50.0 * math.pi / 180.0
    n0 = (C.c_double * 3)(0.0, math.sin(pitch), math.cos(pitch))
    call("calibration_from_plane", L.ssd_calibration_from_plane(n0, 1.0, ident, truth), truth)
    call("calibration_from_plane: null prior", L.ssd_calibration_from_plane(n0, 1.0, None, truth))
    other = ssd.Calibration()
    call("calibration_from_plane: n0 = 0", L.ssd_calibration_from_plane((C.c_double * 3)(0.0, 0.0, 0.0), 1.0, ident, other), other)
    wpts = (C.c_double * 9)(-0.35, 0.9, 0.0, 0.35, 0.9, 0.0, 0.2, 0.35, 0.0)
    cpts = (C.c_double * 9)(-0.35, 0.31, 1.22, 0.35, 0.31, 1.22, 0.2, 0.73, 0.87)
    fromp = ssd.Calibration()
    call("calibration_from_points", L.ssd_calibration_from_points(wpts, cpts, fromp), fromp)
    call("calibration_from_points: null", L.ssd_calibration_from_points(None, cpts, fromp))
    same = (C.c_double * 9)(*([0.1, 0.2, 0.3] * 3))
    call("calibration_from_points: one point thrice", L.ssd_calibration_from_points(wpts, same, other), other)
    with tempfile.TemporaryDirectory() as d:
        tri, pts = os.path.join(d, "triangle.txt"), os.path.join(d, "points.txt")
        with open(tri, "w") as fh:
            fh.write("calibration triangle\n" + "".join("x%d = %r, y%d = %r, z%d = %r\n" % (n, wpts[3 * n - 3], n, wpts[3 * n - 2], n, wpts[3 * n - 1])
                                                        for n in (1, 2, 3)) + "lowerQuadrant = left\n")
        with open(pts, "w") as fh:
            fh.write("calibration points\n" + "".join("; ".join("%r, %r, %r" % (cpts[3 * k] + 1e-3 * r, cpts[3 * k + 1], cpts[3 * k + 2]) for k in range(3)) + "\n"
                                                      for r in range(10)))
        loaded, lw, lc, cal = C.c_int(-1), (C.c_double * 9)(), (C.c_double * 9)(), ssd.Calibration()
        call("calibration_load", L.ssd_calibration_load(tri.encode(), pts.encode(), cal, loaded, lw, lc), cal, loaded, lw, lc)
        call("calibration_load: no such file", L.ssd_calibration_load(tri.encode(), (pts + ".none").encode(), cal, loaded, None, None), cal, loaded)
        call("calibration_load: null", L.ssd_calibration_load(None, pts.encode(), cal, loaded, None, None))

    # the frame, and the staircase it shows
    xyz, depth, labels = staircase(ssd, truth)
    intr = ssd.Intrinsics(60.0, 60.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.00025)
    prior = ssd.Camera(truth, intr, 1, 0)
    target = ssd.StairPoseTarget()
    target.prior = prior
    target.map.ground = 1
    target.map.stairs.n_steps = 3
    for k in range(3):
        y0 = 0.2 + 0.3 * k
        target.map.stairs.steps[k].height = 0.16 * k
        target.map.stairs.steps[k].quad[:] = [-0.4, y0, 0.4, y0, -0.4, y0 + 0.3, 0.4, y0 + 0.3]
    result = target.map.stairs
    frames = (("vertices", ssd.INPUT_VERTICES, xyz), ("depth", ssd.INPUT_DEPTH16, depth))
    back = np.zeros((W * H, 3), np.float32)
    call("deproject_host", L.ssd_deproject_host(intr, W, H, ptr(depth), ptr(back)), back)
    call("deproject_host: width 0", L.ssd_deproject_host(intr, 0, H, ptr(depth), ptr(back)))

    # ground fit
    gm = ssd.GroundMoments()
    for kind, code, frame in frames:
        call("ground_moments_host, " + kind, L.ssd_ground_moments_host(cfg, prior, code, ptr(frame), 0.05, gm), gm)
    call("ground_moments_host: tol 2", L.ssd_ground_moments_host(cfg, prior, ssd.INPUT_VERTICES, ptr(xyz), 2.0, gm))
    noi = ssd.Camera(truth, intr, 0, 0)
    call("ground_moments_host: depth, no intrinsics", L.ssd_ground_moments_host(cfg, noi, ssd.INPUT_DEPTH16, ptr(depth), 0.05, gm))
    L.ssd_ground_moments_host(cfg, prior, ssd.INPUT_VERTICES, ptr(xyz), 0.05, gm)
    gf = ssd.GroundFit()
    for need in (200, 1 << 30):
        call("ground_fit_solve, min_points %d" % need, L.ssd_ground_fit_solve(gm, truth, need, gf), gf)
    call("ground_fit_solve: null", L.ssd_ground_fit_solve(None, truth, 200, gf))

    # surface fit, gates, refit
    fm, fm2, gates, surf = ssd.FrameMoments(), ssd.FrameMoments(), ssd.FrameGates(), ssd.FrameSurfaces()
    for kind, code, frame in frames:
        call("surface_moments_host, " + kind, L.ssd_surface_moments_host(cfg, code, intr, ptr(frame), ptr(labels), 3, 1, fm), fm)
    call("surface_moments_host: a label above n_surfaces", L.ssd_surface_moments_host(cfg, ssd.INPUT_VERTICES, intr, ptr(xyz), ptr(labels), 2, 1, fm))
    call("surface_moments_host: n_surfaces 18", L.ssd_surface_moments_host(cfg, ssd.INPUT_VERTICES, intr, ptr(xyz), ptr(labels), 18, 1, fm))
    L.ssd_surface_moments_host(cfg, ssd.INPUT_VERTICES, intr, ptr(xyz), ptr(labels), 3, 1, fm)
    call("surface_fit_solve", L.ssd_surface_fit_solve(fm, truth, 200, surf), surf)
    bad = ssd.FrameMoments()
    bad.n_surfaces = 18
    call("surface_fit_solve: n_surfaces 18", L.ssd_surface_fit_solve(bad, truth, 200, surf))
    call("surface_gates_from_moments", L.ssd_surface_gates_from_moments(fm, 200, 2.5, 0.001, gates), gates)
    call("surface_gates_from_moments: k_sigma 0", L.ssd_surface_gates_from_moments(fm, 200, 0.0, 0.001, gates))
    call("surface_gates_from_moments: gate_min 2", L.ssd_surface_gates_from_moments(fm, 200, 2.5, 2.0, gates))
    for kind, code, frame in frames:
        call("surface_refit_moments_host, " + kind, L.ssd_surface_refit_moments_host(cfg, code, intr, ptr(frame), ptr(labels), gates, 3, 1, fm2), fm2)
    call("surface_refit_moments_host: null gates", L.ssd_surface_refit_moments_host(cfg, ssd.INPUT_VERTICES, intr, ptr(xyz), ptr(labels), None, 3, 1, fm2))
    call("surface_refit_moments_host: depth, no intrinsics", L.ssd_surface_refit_moments_host(cfg, ssd.INPUT_DEPTH16, None, ptr(depth), ptr(labels), gates, 3, 1, fm2))

    # the camera fold and its gates: four frames of two cameras
    moments = (ssd.FrameMoments * 4)(fm, fm2, fm, fm2)
    cam_of = (C.c_uint16 * 4)(0, 1, 1, 0)
    cams = (ssd.Camera * 2)(prior, prior)
    drift, drift2 = (ssd.CameraDrift * 2)(), (ssd.CameraDrift * 2)()
    call("camera_drift_fold", L.ssd_camera_drift_fold(moments, cam_of, 4, cams, 2, 200, drift), drift)
    call("camera_drift_fold: a camera beyond the table", L.ssd_camera_drift_fold(moments, cam_of, 4, cams, 1, 200, drift2))
    call("camera_drift_fold: ncams 0", L.ssd_camera_drift_fold(moments, cam_of, 4, cams, 0, 200, drift2))
    fold = (ssd.CameraFold * 2)()
    for c in range(2):
        C.memmove(C.byref(fold[c]), C.byref(drift[c]), C.sizeof(ssd.CameraFold))
    call("camera_drift_from_fold", L.ssd_camera_drift_from_fold(fold, cams, 2, 200, drift2), drift2)
    fold[1].camera = 0
    call("camera_drift_from_fold: a record of another camera", L.ssd_camera_drift_from_fold(fold, cams, 2, 200, drift2))
    cgates = (ssd.FrameGates * 4)()
    call("camera_ground_gates", L.ssd_camera_ground_gates(moments, cam_of, 4, drift, 2, 2.5, 0.001, cgates), cgates)
    call("camera_ground_gates: ncams 0", L.ssd_camera_ground_gates(moments, cam_of, 4, drift, 0, 2.5, 0.001, cgates))
    call("camera_ground_gates: k_sigma 17", L.ssd_camera_ground_gates(moments, cam_of, 4, drift, 2, 17.0, 0.001, cgates))

    # tread clearance
    clm, clear, mask = ssd.FrameMoments(), ssd.FrameClearance(), np.zeros(W * H, np.uint8)
    for rule in (ssd.ClearanceRule(), ssd.ClearanceRule(0.0, 0.03, 0.5)):
        for kind, code, frame in frames:
            call("clearance_host, margin %g, %s" % (rule.margin, kind), L.ssd_clearance_host(cfg, truth, code, intr, ptr(frame), result, 1, rule, clm, ptr(mask)),
                 clm, mask)
        call("clearance_solve, margin %g" % rule.margin, L.ssd_clearance_solve(clm, result, truth, 10, clear), clear)
    call("clearance_host: lo 0", L.ssd_clearance_host(cfg, truth, ssd.INPUT_VERTICES, intr, ptr(xyz), result, 1, ssd.ClearanceRule(0.03, 0.0, 0.5), clm, None))
    call("clearance_host: null rule", L.ssd_clearance_host(cfg, truth, ssd.INPUT_VERTICES, intr, ptr(xyz), result, 1, None, clm, None))
    call("clearance_solve: n_surfaces 18", L.ssd_clearance_solve(bad, result, truth, 10, clear))

    # tread grid, its fold, the stair map
    grid, acc, foot = ssd.FrameTreadGrid(), ssd.FrameTreadGrid(), ssd.FrameFootholds()
    rule = ssd.TreadGridRule()
    for kind, code, frame in frames:
        call("tread_grid_host, " + kind, L.ssd_tread_grid_host(cfg, truth, code, intr, ptr(frame), result, 1, rule, grid), grid)
    call("tread_grid_host: cell 0", L.ssd_tread_grid_host(cfg, truth, ssd.INPUT_VERTICES, intr, ptr(xyz), result, 1, ssd.TreadGridRule(cell=0.0), grid))
    call("tread_grid_host: hi below lo", L.ssd_tread_grid_host(cfg, truth, ssd.INPUT_VERTICES, intr, ptr(xyz), result, 1, ssd.TreadGridRule(hi=0.01), grid))
    L.ssd_tread_grid_host(cfg, truth, ssd.INPUT_VERTICES, intr, ptr(xyz), result, 1, rule, grid)
    for along, deep in ((0.0, 0.0), (0.1, 0.06), (5.0, 5.0)):
        call("tread_grid_solve, foot %g x %g" % (along, deep), L.ssd_tread_grid_solve(grid, result, rule, 1, 1, along, deep, foot), foot)
    call("tread_grid_solve: foot -1", L.ssd_tread_grid_solve(grid, result, rule, 1, 1, -1.0, 0.0, foot))
    call("tread_grid_solve: null rule", L.ssd_tread_grid_solve(grid, result, None, 1, 1, 0.0, 0.0, foot))
    for i in range(3):
        call("tread_grid_add %d" % i, L.ssd_tread_grid_add(grid, acc), acc)
    acc.s[0].n_seen_out = 0xffffffff
    grid.s[0].n_seen_out = 1
    call("tread_grid_add: past 2^32 - 1", L.ssd_tread_grid_add(grid, acc), acc)
    call("tread_grid_add: null", L.ssd_tread_grid_add(None, acc))
    results = (ssd.FrameResult * 5)(result, result, result, result, result)
    results[1].steps[1].height = 0.17
    results[2].n_steps = 2
    results[3].status = 1
    results[4].steps[2].quad[3] = float("nan")
    smap, used = ssd.StairMap(), C.c_int(-1)
    call("stair_map_from_results", L.ssd_stair_map_from_results(results, 5, 1, smap, used), smap, used)
    call("stair_map_from_results: nframes -1", L.ssd_stair_map_from_results(results, -1, 1, smap, used))

    # stair pose, and the riser fit over its riser records
    rec, pacc, pose = ssd.StairPoseMoments(), ssd.StairPoseMoments(), ssd.StairPose()
    prule = ssd.StairPoseRule()
    for kind, code, frame in frames:
        call("stair_pose_host, " + kind, L.ssd_stair_pose_host(cfg, target, code, ptr(frame), prule, rec), rec)
    call("stair_pose_host: reach NaN", L.ssd_stair_pose_host(cfg, target, ssd.INPUT_VERTICES, ptr(xyz), ssd.StairPoseRule(reach=float("nan")), rec))
    odd = ssd.StairPoseTarget.from_buffer_copy(target)
    odd.map.stairs.n_steps = 18
    call("stair_pose_host: n_steps 18", L.ssd_stair_pose_host(cfg, odd, ssd.INPUT_VERTICES, ptr(xyz), prule, rec))
    odd = ssd.StairPoseTarget.from_buffer_copy(target)
    odd.prior.has_intrinsics = 0
    call("stair_pose_host: depth, no intrinsics", L.ssd_stair_pose_host(cfg, odd, ssd.INPUT_DEPTH16, ptr(depth), prule, rec))
    L.ssd_stair_pose_host(cfg, target, ssd.INPUT_VERTICES, ptr(xyz), prule, rec)
    for i in range(3):
        call("stair_pose_add %d" % i, L.ssd_stair_pose_add(rec, pacc), pacc)
    full, one = ssd.StairPoseMoments.from_buffer_copy(pacc), ssd.StairPoseMoments()
    full.risers.s[15].n_far = (1 << 63) - 1
    one.risers.s[15].n_far = 1
    call("stair_pose_add: past int64", L.ssd_stair_pose_add(one, full), full)
    call("stair_pose_add: null", L.ssd_stair_pose_add(None, full))
    call("stair_pose_solve, from the truth", L.ssd_stair_pose_solve(pacc, target, 200, ssd.SP_OBSERVABLE, pose), pose)
    moved = ssd.StairPoseTarget.from_buffer_copy(target)
    moved.prior.cal.t2[1] += 0.02
    moved.prior.cal.world_z += 0.015
    for kind, code, frame in frames:
        L.ssd_stair_pose_host(cfg, moved, code, ptr(frame), prule, rec)
        call("stair_pose_solve, moved prior, " + kind, L.ssd_stair_pose_solve(rec, moved, 1, ssd.SP_OBSERVABLE, pose), pose)
    call("stair_pose_solve, too few", L.ssd_stair_pose_solve(rec, moved, 1 << 30, ssd.SP_OBSERVABLE, pose), pose)
    call("stair_pose_solve: observable 2", L.ssd_stair_pose_solve(rec, moved, 1, 2.0, pose))
    call("stair_pose_solve: null", L.ssd_stair_pose_solve(None, moved, 1, 0.5, pose))
    L.ssd_stair_pose_host(cfg, target, ssd.INPUT_VERTICES, ptr(xyz), prule, rec)
    risers, fits = ssd.FrameRisers(), ssd.FrameRiserFits()
    risers.n_risers = 2
    for i in range(2):
        y = 0.5 + 0.3 * i
        risers.risers[i] = ssd.Riser(1440, 1, 0.16 * i, 0.16 * (i + 1), (C.c_double * 2)(-0.4, y), (C.c_double * 2)(0.4, y), 0.0)
    call("riser_fit_solve", L.ssd_riser_fit_solve(rec.risers, risers, truth, 100, fits), fits)
    risers.n_risers = 1
    call("riser_fit_solve: n_risers differs", L.ssd_riser_fit_solve(rec.risers, risers, truth, 100, fits))

    # labels and the serializer
    mixed = labels.copy()
    mixed[::7] = ssd.LABEL_RISER_BASE + 1
    sur, ris = np.zeros_like(mixed), np.zeros_like(mixed)
    call("labels_split", L.ssd_labels_split(ptr(mixed), mixed.size, ptr(sur), ptr(ris)), sur, ris)
    mixed[5] = 200
    call("labels_split: a label of neither kind", L.ssd_labels_split(ptr(mixed), mixed.size, ptr(sur), ptr(ris)))
    call("labels_split: null", L.ssd_labels_split(None, 4, ptr(sur), ptr(ris)))
    buf = C.create_string_buffer(4096)
    for name, r in (("the map", result), ("a thrown frame", results[3]), ("a NaN corner", results[4]), ("no steps", ssd.FrameResult())):
        call("serialize, " + name, L.ssd_serialize(r, buf, 4096), buf)
    call("serialize: 16 bytes", L.ssd_serialize(result, buf, 16))
    call("serialize: null", L.ssd_serialize(None, buf, 4096))
    print("\n".join(lines))


def main():
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        return child()
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    lists = []
    for lib in sys.argv[1:]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, SSD_HIP_LIB=os.path.abspath(lib)),
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("%s: the child failed\n%s%s" % (lib, r.stdout, r.stderr))
        lists.append(r.stdout.splitlines())
    a, b = lists
    print("# handle-free entry points, call by call: A = %s | B = %s" % tuple(sys.argv[1:]))
    differ = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    for x, y in zip(a, b):
        print(x if x == y else "DIFFERS\n  A " + x + "\n  B " + y)
    refusals = sum(" rc   -" in x or " rc  -" in x for x in a)
    print("verdict: %s (%d calls, %d of them refusals)" % ("identical" if not differ else "%d DIFFER" % differ, len(a), refusals))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
