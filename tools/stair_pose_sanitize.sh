#!/bin/bash
# tools/stair_pose_sanitize.sh - the stair pose's host rule, fold and solve under AddressSanitizer + UBSan: the library's sources and
# tools/stair_pose_sanitize.cpp (a stand-alone program with its own main) linked into one executable, the HOST code instrumented
# (-fno-gpu-sanitize: the device code is compiled as always and never runs here), and run once.  CPU only; needs no GPU and no preload.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/ssd_pose_sanitize
mkdir -p $OUT
cd $ROOT/stair-step-detector_amd/csrc
${HIPCC:-hipcc} -O1 -g -std=c++17 -ffp-contract=off --offload-arch=${ARCH:-gfx950} -fsanitize=address,undefined -fno-sanitize-recover=undefined \
    -fno-gpu-sanitize -Wno-unused-private-field -x hip ssd_kernels.hip ssd_kernels_cams.hip ssd_kernels_ground.hip ssd_kernels_refit.hip \
    ssd_kernels_solve.hip ssd_kernels_fold.hip ssd_capi.hip ssd_pipeline.hip stairs_api.cpp $ROOT/tools/stair_pose_sanitize.cpp \
    -o $OUT/stair_pose_sanitize
ASAN_OPTIONS=detect_leaks=1 $OUT/stair_pose_sanitize
