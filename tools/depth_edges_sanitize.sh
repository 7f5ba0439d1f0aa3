#!/bin/bash
# tools/depth_edges_sanitize.sh - the depth edge filter's host statement under AddressSanitizer + UBSan: csrc/ssd_host.cpp, the handle-free
# half of the C ABI (plain C++: no device compile, no kernel file), and tools/depth_edges_sanitize.cpp (a stand-alone program with its own
# main) compiled into one instrumented executable, and run once.  CPU only; needs no GPU and no preload.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${TMPDIR:-/tmp}/ssd_edges_sanitize
mkdir -p $OUT
${CXX:-$(hipconfig -l)/clang++} -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
    -I$(hipconfig --rocmpath)/include $ROOT/stair-step-detector_amd/csrc/ssd_host.cpp $ROOT/tools/depth_edges_sanitize.cpp -o $OUT/depth_edges_sanitize
ASAN_OPTIONS=detect_leaks=1 $OUT/depth_edges_sanitize
