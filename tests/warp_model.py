"""The depth warp's rule (include/ssd_hip.h) in numpy, written from the rule's text, and the views, frames and
recipes the CPU and the GPU tests share.

For the source pixel (u, v) with sample d under the view (r, t, src) and the target's intrinsics dst, no FMA:
  1. d == 0: EMPTY.  2. float32: dm = d * src.depth_units, x = dm * ((u - src.ppx) / src.fx), y likewise, z = dm.
  3. float64: X = ((r0 x + r1 y) + r2 z) + t0, Y and Z likewise.  4. !(Z > 0): BEHIND.
  5. q = floor(Z / dst.depth_units + 0.5); !(1 <= q <= 65535): RANGE.
  6. a = floor((X / Z) * dst.fx + dst.ppx + 0.5), b likewise; not 0 <= a < W and 0 <= b < H (in doubles; a NaN fails): OUTSIDE.
  7. LANDED on (a, b) with q.  The output pixel is the smallest q that landed on it, 0 where none did."""
import math

import numpy as np

STATS = ("n_empty", "n_behind", "n_range", "n_outside", "n_landed", "n_filled")
F32, F64 = np.float32, np.float64


def intr_tuple(i):
    return (float(i.fx), float(i.fy), float(i.ppx), float(i.ppy), float(i.depth_units))


def view_parts(view):
    """a WarpView -> (r float64 [9], t float64 [3], src's five floats)"""
    return np.array(list(view.r), F64), np.array(list(view.t), F64), intr_tuple(view.src)


def warp_np(frame, view, dst):
    """frame uint16 [H, W]; view: a WarpView or (r, t, src five floats); dst: Intrinsics or five floats -> (warped uint16 [H, W], dict)"""
    r, t, src = view if isinstance(view, tuple) else view_parts(view)
    r, t = np.asarray(r, F64).reshape(9), np.asarray(t, F64).reshape(3)
    dfx, dfy, dppx, dppy, dunits = [F64(F32(v)) for v in (dst if isinstance(dst, tuple) else intr_tuple(dst))]
    sfx, sfy, sppx, sppy, sunits = [F32(v) for v in src]
    f = np.asarray(frame)
    H, W = f.shape
    d = f.reshape(-1).astype(np.int64)
    u = np.tile(np.arange(W), H).astype(F32)
    v = np.repeat(np.arange(H), W).astype(F32)
    xm, ym = (u - sppx) / sfx, (v - sppy) / sfy
    dm = d.astype(F32) * sunits
    x, y, z = (dm * xm).astype(F64), (dm * ym).astype(F64), dm.astype(F64)
    assert (dm * xm).dtype == F32
    with np.errstate(all="ignore"):                                          # (a view may overflow: the rule says what then)
        X = ((r[0] * x + r[1] * y) + r[2] * z) + t[0]
        Y = ((r[3] * x + r[4] * y) + r[5] * z) + t[1]
        Z = ((r[6] * x + r[7] * y) + r[8] * z) + t[2]
    empty = d == 0
    behind = ~empty & ~(Z > 0)
    live = ~empty & ~behind
    with np.errstate(all="ignore"):
        Zs = np.where(live, Z, 1.0)
        q = np.floor(Zs / dunits + 0.5)
        rng = live & ~((q >= 1) & (q <= 65535))
        live = live & ~rng
        a = np.floor((X / Zs) * dfx + dppx + 0.5)
        b = np.floor((Y / Zs) * dfy + dppy + 0.5)
        inside = (a >= 0) & (a < W) & (b >= 0) & (b < H)
    outside = live & ~inside
    landed = live & inside
    out = np.full(H * W, 1 << 20, np.int64)
    np.minimum.at(out, (b[landed].astype(np.int64) * W + a[landed].astype(np.int64)), q[landed].astype(np.int64))
    out[out == 1 << 20] = 0
    stats = dict(n_empty=int(empty.sum()), n_behind=int(behind.sum()), n_range=int(rng.sum()), n_outside=int(outside.sum()),
                 n_landed=int(landed.sum()), n_filled=int((out != 0).sum()))
    return out.astype(np.uint16).reshape(H, W), stats


def stats_dict(s):
    return {k: int(getattr(s, k)) for k in STATS}


def make_view(ssd, r, t, src):
    v = ssd.WarpView()
    v.r[:] = [float(x) for x in np.asarray(r, F64).reshape(9)]
    v.t[:] = [float(x) for x in np.asarray(t, F64).reshape(3)]
    v.src = src
    return v


def identity_view(ssd, src):
    return make_view(ssd, np.eye(3), np.zeros(3), src)


def rotation(rx_deg, ry_deg, rz_deg):
    rx, ry, rz = (math.radians(a) for a in (rx_deg, ry_deg, rz_deg))
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def seeded_views(ssd, src, count=8, seed=77, max_deg=3.0, max_shift=0.05):
    """views with rotations up to max_deg about each axis and shifts up to max_shift metres along each"""
    rng = np.random.default_rng(seed)
    return [make_view(ssd, rotation(*rng.uniform(-max_deg, max_deg, 3)), rng.uniform(-max_shift, max_shift, 3), src) for _ in range(count)]


def push_away_view(ssd, src, by=3.0):
    """the scene `by` metres further along the optical axis: the image shrinks, many samples per target pixel"""
    return make_view(ssd, np.eye(3), [0.0, 0.0, by], src)


def pull_near_view(ssd, src, by=0.4):
    """the scene `by` metres nearer: the image grows, holes between the samples, the near ones BEHIND or out of the frame"""
    return make_view(ssd, np.eye(3), [0.0, 0.0, -by], src)


def scene_src(ssd, w, h):
    sc = ssd.make_scene(w, h, n_steps=3, seed=1000, sigma=0.0)
    return ssd.intrinsics_for_scene(sc)


def scene_frames(ssd, w=64, h=48):
    """the clean, the stress and the 10 %-invalid frame of the 3-step scene, uint16 [3, H, W]"""
    mk = lambda **kw: ssd.make_scene(w, h, n_steps=3, seed=1000, **kw)                                # noqa: E731
    return ssd.synth_depth_host([mk(sigma=0.0), mk(sigma=0.002, outlier_frac=0.05, invalid_frac=0.02), mk(sigma=0.003, outlier_frac=0.05, invalid_frac=0.10)])


# ---- the view between two cameras (ssd_depth_warp_view_between) ------------------------------------------------------------------------
def external_map(cal):
    """e = T p + c of a Calibration: ToExternalWorld (r2, t2 on x and y, world_z on z) behind CameraToWorld (a, b)"""
    a, b = np.array(list(cal.a), F64).reshape(3, 3), np.array(list(cal.b), F64)
    R2 = np.eye(3)
    R2[:2, :2] = np.array(list(cal.r2), F64).reshape(2, 2)
    return R2 @ a, R2 @ b + np.array([cal.t2[0], cal.t2[1], cal.world_z], F64)


def view_between_np(cal_src, cal_dst):
    Ts, cs = external_map(cal_src)
    Td, cd = external_map(cal_dst)
    inv = np.linalg.inv(Td)
    return inv @ Ts, inv @ (cs - cd)


# ---- the accuracy recipe (tools/depth_warp_accuracy.py records it, tests/test_depth_warp.py holds the host statement to it) -------------
ACC_W, ACC_H, ACC_FAR, ACC_SEED = 256, 192, 40, 1000
# (pitch, roll in degrees, camera height, position along the floor in metres): the target first, then four moved poses - up to 1 degree of
# pitch, 0.5 of roll, 2 cm of height and 3 cm along the floor away from it
ACC_POSES = ((50.0, 0.0, 1.00, 0.00), (51.0, 0.0, 1.01, 0.03), (49.5, 0.5, 0.98, -0.02), (50.5, -0.5, 1.02, 0.01), (49.0, 0.3, 0.99, -0.03))


def pose_scene(ssd, pose, seed=ACC_SEED, noisy=False, w=ACC_W, h=ACC_H):
    """the 3-step scene seen from a pose: a camera moved delta along the floor is the generator's camera, which sits at (0, 0, cam_height)
    over an unbounded floor, in front of a staircase shifted by -delta"""
    pitch, roll, height, along = pose
    noise = dict(sigma=0.002, outlier_frac=0.05, invalid_frac=0.02) if noisy else dict(sigma=0.0)
    return ssd.make_scene(w, h, n_steps=3, seed=seed, pitch_deg=pitch, roll_deg=roll, cam_height=height, first_riser_y=0.45 - along, **noise)


def pose_view(ssd, pose_src, pose_dst, w=ACC_W, h=ACC_H):
    """the view between two poses from the scenes' axes and positions: p_dst = A_dst^T (A_src p_src + o_src - o_dst), the columns of A a
    camera's axes in the world and o its position"""
    s, d = pose_scene(ssd, pose_src, w=w, h=h), pose_scene(ssd, pose_dst, w=w, h=h)
    A = lambda sc: np.array([list(sc.axis_right), list(sc.axis_down), list(sc.axis_fwd)], F64).T     # noqa: E731
    o = lambda sc, pose: np.array([0.0, pose[3], sc.cam_height], F64)                                  # noqa: E731
    return make_view(ssd, A(d).T @ A(s), A(d).T @ (o(s, pose_src) - o(d, pose_dst)), ssd.intrinsics_for_scene(s))


def detection_figures(ssd, oracle, figures):
    """the warped-and-fused frame and the target's clean frame through the CPU oracle under the target's calibration: step counts and the
    worst step height difference"""
    import oracle_binding as ob
    sc = pose_scene(ssd, ACC_POSES[0])
    ocfg = ob.to_oracle_config(ssd.default_config(ACC_W, ACC_H))
    ocal = ob.to_oracle_calibration(ssd.transformation_for_scene(sc).constants)

    def detect(depth):
        n, steps, _ = oracle.process_lean(ocfg, ocal, ssd.deproject_host(figures["dst"], depth))
        return n, [float(s[0]) for s in steps]
    clean_n, clean_h = detect(figures["target_clean"])
    fused_n, fused_h = detect(ssd.depth_fuse_host(figures["warped"])[0])
    worst = max((abs(a - b) for a, b in zip(fused_h, clean_h)), default=0.0) if fused_n == clean_n else float("inf")
    return dict(clean_steps=clean_n, clean_heights=clean_h, fused_steps=fused_n, fused_heights=fused_h, worst=worst)


def solved_views(ssd, oracle):
    """the recipe's views from what the stair pose hands back, not from the true poses: the staircase's map is the oracle's result on the
    target's clean frame under the target's calibration; every pose's noisy frame is located against it by stair_pose_model.chain_host
    (ssd_stair_pose_host, ssd_stair_pose_add, ssd_stair_pose_solve, three passes) from the prior "the camera has not moved", the target's
    calibration; ssd_depth_warp_view_between takes the cameras that come back.  A frame whose chain does not end GF_OK keeps the prior.
    -> (views, [the last pass's status per pose], [passes that ended GF_OK per pose])"""
    import clearance_model as cm
    import oracle_binding as ob
    import stair_pose_model as sp
    target = pose_scene(ssd, ACC_POSES[0])
    truth, dst = ssd.transformation_for_scene(target).constants, ssd.intrinsics_for_scene(target)
    cfg = ssd.default_config(ACC_W, ACC_H)
    clean = ssd.deproject_host(dst, ssd.synth_depth_host([target])[0])
    res = cm.result_of_oracle(ssd, oracle.process(ob.to_oracle_config(cfg), ob.to_oracle_calibration(truth), clean)[0])
    stair_map, _ = ssd.stair_map_from_results([res])
    cams, status, passes = [], [], []
    for i, p in enumerate(ACC_POSES):
        sc = pose_scene(ssd, p, seed=ACC_SEED + i, noisy=True)
        intr = ssd.intrinsics_for_scene(sc)
        cals, poses = sp.chain_host(ssd, cfg, [ssd.deproject_host(intr, ssd.synth_depth_host([sc])[0])], truth, stair_map)
        cams.append(ssd._as_camera(cals[-1] if cals else truth, intr))
        status.append(int(poses[-1].status))
        passes.append(len(cals))
    return [ssd.depth_warp_view_between(c, cams[0]) for c in cams], status, passes


def solved_figures(ssd, oracle, figures):
    """the warped-and-fused frame once more with solved_views in place of the true poses' views: its pixel figures against the target's
    clean frame, how far each solved view is from the true one, and detection_figures' dict for it"""
    views, status, passes = solved_views(ssd, oracle)
    true_views = [pose_view(ssd, p, ACC_POSES[0]) for p in ACC_POSES]
    noisy = ssd.synth_depth_host([pose_scene(ssd, p, seed=ACC_SEED + i, noisy=True) for i, p in enumerate(ACC_POSES)])
    warped = np.array([ssd.depth_warp_host(f, v, figures["dst"])[0] for f, v in zip(noisy, views)])
    off = []
    for v, t in zip(views, true_views):
        (r, tr, _), (wr, wt, _) = view_parts(v), view_parts(t)
        d = r.reshape(3, 3) @ wr.reshape(3, 3).T
        off.append((math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(d) - 1.0) / 2.0)))), float(np.linalg.norm(tr - wt))))
    det = detection_figures(ssd, oracle, dict(figures, warped=warped))
    return dict(status=status, passes=passes, view_error=off, pixels=against(ssd.depth_fuse_host(warped)[0], figures["target_clean"]), detection=det)


def against(frame, clean, far=ACC_FAR):
    """a frame against the target's clean one, over the pixels that are valid there -> (share of them valid in the frame, share of those
    more than `far` raw units off, rms of the rest in raw units)"""
    ref = clean != 0
    valid = ref & (frame != 0)
    err = np.abs(frame.astype(np.int64) - clean.astype(np.int64))
    off = valid & (err > far)
    rest = valid & ~off
    return (float(valid.sum()) / max(int(ref.sum()), 1), float(off.sum()) / max(int(valid.sum()), 1),
            float(np.sqrt((err[rest].astype(F64) ** 2).mean())) if rest.any() else 0.0)


def accuracy_figures(ssd):
    """the issue's table from ssd_depth_warp_host and ssd_depth_fuse_host: dict(single, unwarped, warped_fused, clean=[per moved pose])"""
    target = ACC_POSES[0]
    dst = ssd.intrinsics_for_scene(pose_scene(ssd, target))
    clean = ssd.synth_depth_host([pose_scene(ssd, target)])[0]
    views = [pose_view(ssd, p, target) for p in ACC_POSES]
    clean_moved = ssd.synth_depth_host([pose_scene(ssd, p) for p in ACC_POSES])
    noisy = ssd.synth_depth_host([pose_scene(ssd, p, seed=ACC_SEED + i, noisy=True) for i, p in enumerate(ACC_POSES)])
    warped = np.array([ssd.depth_warp_host(f, v, dst)[0] for f, v in zip(noisy, views)])
    return dict(single=against(noisy[0], clean), unwarped=against(ssd.depth_fuse_host(np.ascontiguousarray(noisy))[0], clean),
                warped_fused=against(ssd.depth_fuse_host(warped)[0], clean),
                clean=[against(ssd.depth_warp_host(f, v, dst)[0], clean) for f, v in list(zip(clean_moved, views))[1:]],
                clean_unwarped=[against(f, clean) for f in clean_moved[1:]], warped=warped, target_clean=clean, dst=dst)
