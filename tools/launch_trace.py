#!/usr/bin/env python3
"""tools/launch_trace.py - walks the launch rules of csrc (ssd_launch.h, the launcher sections of ssd_kernels*.hip) at the smallest shapes
that reach them, so that two builds' launches can be compared dispatch by dispatch.  TEST INFRASTRUCTURE (needs a GPU; the library is
SSD_HIP_LIB's, as for every tool, and the test hooks are the ones beside it).

    rocprofv3 --kernel-trace -d OUT_A --output-format csv -- python3 tools/launch_trace.py          (SSD_HIP_LIB = the one build)
    rocprofv3 --kernel-trace -d OUT_B --output-format csv -- python3 tools/launch_trace.py          (SSD_HIP_LIB = the other)
    python3 tools/launch_trace.py --compare OUT_A OUT_B > profiles/launch_layer_trace.txt

The walk: frames of 64 x 16 points (the lower bound of single_pass_geometry; a tile is the frame) and of 96 x 16 (a tile is no whole
number of rows: K1's sorted strips), batches of 2 and of 65 frames (either side of kImgFewFrames), a plain configuration and the checked
one of tests/test_gpu_prefilter_regimes.py (the z range ends inside a bin: the CHECKS instantiations), under the handle's calibration
and under a table of two cameras, from 16-byte aligned vertices, vertices 4 bytes off, and 16-bit depth, in two passes and with the
single pass forced (the test hook: the product only takes it for large batches); then labels, surface moments with a refit under host
gates and one under device gates behind them, risers, riser moments, riser labels, and debug capture with images (k_inquad's FULL).
Everything runs in the handle's one workspace on the null stream, each batch fetched before the next: the dispatches are a sequence.

--compare reads the kernel traces of two such runs and holds (kernel name, grid, workgroup size, LDS) of dispatch i of the one against
dispatch i of the other; exit status 1 when a line differs.
"""
import csv
import ctypes as C
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((64, 16), (96, 16))
BATCHES = (2, 65)


def walk(ssd, W, H, n, checked):
    import numpy as np
    scs = [ssd.make_scene(W, H, seed=100 + i, pitch_deg=50.0 + (i % 2)) for i in range(n)]
    trans = [ssd.transformation_for_scene(scs[0]), ssd.transformation_for_scene(scs[1])]
    intr = ssd.intrinsics_for_scene(scs[0])
    cfg = ssd.default_config(W, H, max_frames_per_batch=n, batches_in_flight=1)
    if checked:
        cfg.z_max = cfg.z_min + 100.5 * cfg.height_interval
    det = ssd.Detector(cfg, trans[0], 0)
    det.set_intrinsics(intr)
    wh, rec = W * H, C.sizeof(ssd.FrameMoments)
    vert, off, dep = ssd.DeviceBuffer(n * wh * 12, 0), ssd.DeviceBuffer(n * wh * 12 + 16, 0), ssd.DeviceBuffer(n * wh * 2, 0)
    labels, mom, out = ssd.DeviceBuffer(n * wh, 0), ssd.DeviceBuffer(n * rec, 0), ssd.DeviceBuffer(n * rec, 0)
    xyz = ssd.synth_host(scs)
    vert.upload(xyz)
    off.upload(xyz, offset=4)
    dep.upload(ssd.synth_depth_host(scs))
    camera_of = np.arange(n, dtype=np.uint16) % 2
    calls = 0
    try:
        for cams in (False, True):
            det.set_cameras([(trans[0], intr), (trans[1], intr)] if cams else [])
            for ptr, depth in ((vert.ptr, False), (off.ptr + 4, False), (dep.ptr, True)):

                def batch(with_labels=False):
                    if cams:
                        det.enqueue_cameras(ptr, n, camera_of, depth=depth, d_labels=labels.ptr if with_labels else None)
                    elif with_labels:
                        (det.enqueue_depth_labels if depth else det.enqueue_labels)(ptr, n, labels.ptr)
                    else:
                        (det.enqueue_depth if depth else det.enqueue)(ptr, n)
                    det.fetch(n)
                    return 1

                for forced in (0, 1):
                    det.single_pass(forced)
                    calls += batch()
                    calls += batch(with_labels=True)
                det.single_pass(0)
                # surface moments, and the refit behind them: gates from the host, then made on the device
                if cams:
                    det.enqueue_cameras_surface_moments(ptr, n, camera_of, mom.ptr, depth=depth)
                else:
                    det.enqueue_surface_moments(ptr, n, mom.ptr, depth=depth)
                det.fetch(n)
                first = (ssd.FrameMoments * n).from_buffer_copy(np.ascontiguousarray(mom.download(n * rec)).tobytes())
                gates = (ssd.FrameGates * n)(*[ssd.surface_gates_from_moments(m, 200, 2.5, 0.0) for m in first])
                (det.enqueue_cameras_surface_refit if cams else det.enqueue_surface_refit)(ptr, n, gates, out.ptr, depth=depth)
                det.fetch_surface_refit()
                (det.enqueue_cameras_surface_refit_device if cams else det.enqueue_surface_refit_device)(ptr, n, mom.ptr, out.ptr, depth=depth)
                det.fetch_surface_refit()
                calls += 3
                # the riser pass, with its moments, with its labels
                det.set_risers(True)
                calls += batch()
                det.set_riser_moments(True)
                calls += batch()
                det.set_riser_labels(True)
                calls += batch(with_labels=True)
                det.set_riser_labels(False)
                det.set_riser_moments(False)
                det.set_risers(False)
                # debug capture with images: the whole ground image
                det.set_debug(True, images=True)
                calls += batch()
                det.set_debug(False)
    finally:
        for b in (vert, off, dep, labels, mom, out):
            b.free()
        det.close()
    return calls


def drive():
    import importlib
    sys.path.insert(0, ROOT)
    ssd = importlib.import_module("stair-step-detector_amd")
    calls = 0
    for W, H in SHAPES:
        for n in BATCHES:
            for checked in (False, True):
                calls += walk(ssd, W, H, n, checked)
                print("%d x %d, %2d frames, %s: done" % (W, H, n, "checked" if checked else "plain"), flush=True)
    print("launch_trace: %d calls into %s" % (calls, ssd.LIB_PATH))
    return 0


def dispatches(directory):
    """[(kernel name, grid, workgroup size, LDS bytes)] of a rocprofv3 kernel trace under `directory`, in dispatch order"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    if len(files) != 1:
        sys.exit("%s: expected one *kernel_trace.csv, found %d" % (directory, len(files)))
    rows = list(csv.DictReader(open(files[0])))

    def cols(prefix):
        return [k for k in rows[0] if k.startswith(prefix)]

    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], "x".join(r[k] for k in cols("Grid_Size")), "x".join(r[k] for k in cols("Workgroup_Size")), r[cols("LDS_Block_Size")[0]])
            for r in rows]


def compare(dir_a, dir_b):
    a, b = dispatches(dir_a), dispatches(dir_b)
    bad = [i for i in range(min(len(a), len(b))) if a[i] != b[i]]
    print("# tools/launch_trace.py under rocprofv3 --kernel-trace, two builds: (kernel name, grid, workgroup size, LDS) dispatch by dispatch")
    print("# dispatches: %d | %d; distinct kernels: %d | %d; distinct (kernel, grid, workgroup, LDS): %d | %d"
          % (len(a), len(b), len({d[0] for d in a}), len({d[0] for d in b}), len(set(a)), len(set(b))))
    for i in bad[:40]:
        print("dispatch %d differs:\n    A %s\n    B %s" % (i, a[i], b[i]))
    same = not bad and len(a) == len(b)
    print("# kernels launched (dispatches in A | B):")
    names = sorted({d[0] for d in a} | {d[0] for d in b})
    for name in names:
        print("%6d | %6d  %s" % (sum(d[0] == name for d in a), sum(d[0] == name for d in b), name.split("(")[0]))
    print("verdict: %s" % ("equal line for line, %d dispatches" % len(a) if same else "DIFFERENT (%d lines, lengths %d | %d)" % (len(bad), len(a), len(b))))
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(drive())
