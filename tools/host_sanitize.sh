#!/bin/bash
# tools/host_sanitize.sh [PROGRAM ...] - the host statements of the stand-alone frame passes under AddressSanitizer + UBSan: csrc/ssd_host.cpp,
# the handle-free half of the C ABI (plain C++: no device compile, no kernel file), compiled once, then each tools/<PROGRAM>_sanitize.cpp
# (a stand-alone program with its own main; default: stair_pose depth_fuse depth_edges depth_warp depth_fill) linked with it and run once.  CPU only; needs no GPU
# and no preload.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mktemp -d "${TMPDIR:-/tmp}/ssd_host_sanitize.XXXXXX")      # a directory per run: two runs at once do not share an object
trap 'rm -rf "$OUT"' EXIT
CXX="${CXX:-$(hipconfig -l)/clang++} -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I$(hipconfig --rocmpath)/include"
$CXX -c $ROOT/stair-step-detector_amd/csrc/ssd_host.cpp -o $OUT/ssd_host.o
for p in ${@:-stair_pose depth_fuse depth_edges depth_warp depth_fill}; do
    $CXX $OUT/ssd_host.o $ROOT/tools/${p}_sanitize.cpp -o $OUT/${p}_sanitize
    ASAN_OPTIONS=detect_leaks=1 $OUT/${p}_sanitize
done
