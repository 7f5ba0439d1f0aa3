"""csrc/ssd_owned.h by itself: tests/owned_main.cpp, a program of its own, built with hipcc and run.

No GPU is needed: without a device every HIP acquisition fails, which is exactly what the program is about - a failed acquire
leaves its owner empty, a failed all-or-nothing group leaves its target and the counted bytes as they were, moves empty their
source, reset() and release() of an empty owner do nothing, and a HIP error maps to SSD_E_NOMEM or SSD_E_HIP.  Where a device
exists the program runs the successful paths too."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "stair-step-detector_amd", "csrc")


def test_owners_by_themselves(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "owned_main")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-Wall", "-I", CSRC, os.path.join(HERE, "owned_main.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("owned: ok"), run.stdout
