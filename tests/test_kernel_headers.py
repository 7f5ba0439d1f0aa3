"""csrc/ssd_k_*.h, ssd_prefilter.h and ssd_launch_rules.h: what the stages of the per-frame path share, and the extension stages
themselves (the per-point decision, the walk, K7, K8, K6), in headers.

Every one of them includes what it uses: a file that includes only that header compiles (syntax only, gfx950 device pass, the
product's language flags); ssd_launch_rules.h, which the launchers read, for the host as well.  No GPU is needed; without hipcc the
compiles are skipped.

Which file includes which .hip is held to the list below.  The refit unit and its three passes take what they build on from
headers and include no body of the chain.  What is left: the chain's bodies, K1 to K5, still stand in ssd_kernels.hip, and
ssd_kernels_cams.hip, which instantiates every stage, is the one file that includes it; when those bodies are cut into headers too,
its entry leaves INCLUDED_HIP and what remains is the rule the layout aims at: no file includes a .hip but the three passes the refit
unit pulls in and the stair pose in the ground unit."""
import glob
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "stair-step-detector_amd", "csrc")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "ssd_k_*.h"))) + ["ssd_prefilter.h", "ssd_launch_rules.h"]
FLAGS = ["-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-fsyntax-only", "-I", CSRC, "-x", "hip"]
BODIES = "ssd_kernels.hip"
INCLUDED_HIP = {"ssd_kernels_cams.hip": {BODIES},
                "ssd_kernels_refit.hip": {"ssd_kernels_clearance.hip", "ssd_kernels_treadgrid.hip", "ssd_kernels_stairmap.hip"},
                "ssd_kernels_ground.hip": {"ssd_kernels_pose.hip"}}


def compile_alone(header, tmp_path, side):
    src = tmp_path / ("only_" + header.replace(".h", ".hip"))
    src.write_text('#include "%s"\n' % header)
    run = subprocess.run([HIPCC, side] + FLAGS + [str(src)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]


def test_the_shared_headers_are_there():
    assert {"ssd_k_entry.h", "ssd_k_point.h", "ssd_k_cells.h", "ssd_k_windows.h", "ssd_launch_rules.h", "ssd_prefilter.h",
            "ssd_k_decide.h", "ssd_k_walk.h", "ssd_k_labels.h", "ssd_k_moments.h", "ssd_k_risers.h"} <= set(HEADERS), HEADERS


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone_for_the_device(header, tmp_path):
    compile_alone(header, tmp_path, "--offload-device-only")


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_launch_rules_compile_alone_for_the_host(tmp_path):
    compile_alone("ssd_launch_rules.h", tmp_path, "--offload-host-only")


def test_chunk_rules_compile_alone_without_hip(tmp_path):
    """The chunk rules (ssd_chunks.h) are a plain header: g++ alone compiles a file that includes nothing else."""
    src = tmp_path / "only_ssd_chunks.cpp"
    src.write_text('#include "ssd_chunks.h"\n')
    run = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-4000:]


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_capi_header_compiles_alone_as_plain_cxx(tmp_path):
    """What the units of the C ABI that call HIP share (ssd_capi.h), under the compiler line of the Makefile's HOSTFLAGS."""
    rocm = subprocess.run([os.path.join(os.path.dirname(HIPCC), "hipconfig"), "--rocmpath"], check=True, capture_output=True, text=True).stdout.strip()
    src = tmp_path / "only_ssd_capi.cpp"
    src.write_text('#include "ssd_capi.h"\n')
    run = subprocess.run([HIPCC, "-x", "c++", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                          "-Wall", "-Wno-unused-function", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]


def test_which_file_includes_which_hip():
    found = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not os.path.isfile(path) or not path.endswith((".h", ".hip", ".cpp")):
            continue
        with open(path, encoding="utf-8") as f:
            names = set(re.findall(r'^\s*#\s*include\s+"([^"]+\.hip)"', f.read(), flags=re.M))
        if names:
            found[os.path.basename(path)] = names
    assert found == INCLUDED_HIP, found
