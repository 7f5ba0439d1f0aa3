"""Per-frame calibration (ssd_set_cameras / ssd_enqueue_cameras; include/ssd_hip.h), CPU tier: the ABI's
layout and null-handle contract, and that the scene sets of tests/test_gpu_cameras.py can tell cameras apart."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle_binding as ob
import scenes

VGA_NAMES = ["vga_3steps_noise2mm", "vga_8steps_outliers", "vga_yaw_outliers", "xga_low_camera"]      # the last: its pose at 640 x 480
XGA_NAMES = ["xga_config1", "xga_low_camera", "xga_roll3", "xga_8steps_outliers"]
SETS = {"vga": (640, 480, VGA_NAMES), "xga": (1024, 768, XGA_NAMES)}
E_ARG = -1


def scene_set(ssd, key):
    """-> (W, H, the set's scenes, all at W x H)"""
    w, h, names = SETS[key]
    return w, h, [ssd.make_scene(w, h, **scenes.scene_params()[n][1]) for n in names]


def test_sizeof_ssd_camera_matches_the_ctypes_mirror(ssd):
    # ssd_calibration: 9 + 3 + 4 + 2 + 1 doubles; ssd_intrinsics: 5 floats; two int32; 8-byte aligned
    assert C.sizeof(ssd.Calibration) == 19 * 8 and C.sizeof(ssd.Intrinsics) == 20
    assert C.sizeof(ssd.Camera) == 19 * 8 + 20 + 4 + 4 + 4                # the four bytes: padding to the doubles' alignment
    assert ssd.Camera.intr.offset == 19 * 8 and ssd.Camera.has_intrinsics.offset == 19 * 8 + 20


def test_sizeof_ssd_camera_as_a_c_compiler_sees_it(ssd, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizeof_camera.c"
    src.write_text('#include "ssd_hip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void)\n{\n'
                   '  printf("%d %d %d\\n", (int)sizeof(ssd_camera), (int)offsetof(ssd_camera, intr), (int)offsetof(ssd_camera, has_intrinsics));\n  return 0;\n}\n')
    exe = tmp_path / "sizeof_camera"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(ssd.Camera), ssd.Camera.intr.offset, ssd.Camera.has_intrinsics.offset]


def test_the_header_states_the_same_struct_and_limits(ssd):
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "ssd_hip.h")).read()
    m = re.search(r"typedef struct\s*\{([^}]*)\}\s*ssd_camera;", text)
    assert m, "ssd_camera is not declared"
    fields = [re.sub(r"/\*.*?\*/", "", f).strip() for f in m.group(1).split(";")]
    assert [f for f in fields if f] == ["ssd_calibration cal", "ssd_intrinsics intr", "int32_t has_intrinsics", "int32_t reserved"]
    assert re.search(r"#define SSD_MAX_CAMERAS\s+%d\b" % ssd.MAX_CAMERAS, text)
    assert re.search(r"#define SSD_INPUT_VERTICES\s+%d\b" % ssd.INPUT_VERTICES, text) and re.search(r"#define SSD_INPUT_DEPTH16\s+%d\b" % ssd.INPUT_DEPTH16, text)
    for name in ("ssd_set_cameras", "ssd_camera_count", "ssd_enqueue_cameras", "ssd_process_host_cameras"):
        assert name in ssd.EXPORTS and hasattr(ssd.lib(), name)


def test_a_null_handle_is_refused(ssd):
    L = ssd.lib()
    cams = (ssd.Camera * 1)()
    idx = (C.c_uint16 * 1)(0)
    res = (ssd.FrameResult * 1)()
    frame = np.zeros(16, dtype=np.float32)
    assert L.ssd_set_cameras(None, cams, 1) == E_ARG
    assert b"null handle" in L.ssd_last_error()
    assert L.ssd_enqueue_cameras(None, frame.ctypes.data_as(C.c_void_p), 192, 1, None, idx, ssd.INPUT_VERTICES, None, 0) == E_ARG
    assert L.ssd_last_error()
    assert L.ssd_process_host_cameras(None, frame.ctypes.data_as(C.c_void_p), 1, idx, ssd.INPUT_VERTICES, res, None) == E_ARG
    assert L.ssd_last_error()
    assert L.ssd_camera_count(None) == 0


@pytest.mark.parametrize("key", ["vga", "xga"])
def test_the_oracle_tells_the_sets_cameras_apart(ssd, oracle, key):
    """A frame's line under the NEXT camera's calibration differs from its line under its own: a batch that mixed cameras up
    could not pass the GPU tests."""
    w, h, scs = scene_set(ssd, key)
    cfg = ob.to_oracle_config(ssd.default_config(w, h))
    cals = [ob.to_oracle_calibration(ssd.transformation_for_scene(sc).constants) for sc in scs]
    frames = ssd.synth_host(scs)
    for i in range(len(scs)):
        own = oracle.process_lean(cfg, cals[i], frames[i])
        other = oracle.process_lean(cfg, cals[(i + 1) % len(scs)], frames[i])
        assert own[0] >= 2, "the frame's own camera sees its stairs"
        assert (own[0], [tuple(s) for s in own[1][:own[0]]], own[2]) != (other[0], [tuple(s) for s in other[1][:other[0]]], other[2]), SETS[key][2][i]
