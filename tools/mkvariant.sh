#!/bin/bash
# tools/mkvariant.sh NAME [GIT_REV] [EXTRA_FLAGS] [SED_EXPR] — builds stair-step-detector_amd/lib_NAME/ for A/B runs (tools/ab.sh,
# tools/ab_inflight.py, SSD_HIP_LIB=.../lib_NAME/libssd_hip.so): all three libraries, because __init__.py looks for the source and hook
# libraries beside SSD_HIP_LIB.  The current tree, or with GIT_REV the whole of csrc/ and include/ as that commit has them (git archive),
# so that the parent of a change that spans files can be built.  SED_EXPR, when given, is applied to the copy's kernel files,
# ssd_kernels*.hip and the headers ssd_k_*.h (experiments that are not worth a macro in the source).  Tools only; lib_* is git-ignored
# and travels to the GPU box.
set -e
NAME=$1; REV=$2; EXTRA=$3; SEDX=$4
R=$(cd $(dirname $0)/.. && pwd)
T=$(mktemp -d)
trap 'rm -rf $T' EXIT
# the Makefile reaches the headers through ../../include
if [ -n "$REV" ]; then
  git -C $R archive $REV stair-step-detector_amd/csrc include | tar -x -C $T
else
  mkdir -p $T/stair-step-detector_amd && cp -r $R/stair-step-detector_amd/csrc $T/stair-step-detector_amd/csrc && cp -r $R/include $T/include
fi
if [ -n "$SEDX" ]; then sed -i -e "$SEDX" $(ls $T/stair-step-detector_amd/csrc/ssd_kernels*.hip $T/stair-step-detector_amd/csrc/ssd_k_*.h 2>/dev/null); fi
mkdir -p $R/stair-step-detector_amd/lib_$NAME
make -C $T/stair-step-detector_amd/csrc OUT=$R/stair-step-detector_amd/lib_$NAME EXTRA="$EXTRA" 2>&1 | grep -E "error|Error" || true
ls -la $R/stair-step-detector_amd/lib_$NAME/libssd_hip.so $R/stair-step-detector_amd/lib_$NAME/libssd_source.so $R/stair-step-detector_amd/lib_$NAME/libssd_testhooks.so
