#!/usr/bin/env python3
"""Kernel resources of the depth-fill build beside its parent, from the code objects alone (no GPU needed).

    python tools/depth_fill_kernel_resources.py PARENT/libssd_hip.so [THIS/libssd_hip.so] > profiles/depth_fill_kernel_resources.txt

As tools/depth_edges_kernel_resources.py (it uses the readers of tools/cameras_kernel_resources.py):
  1. every kernel symbol of the parent with VGPRs / AGPRs / SGPRs / LDS / scratch / occupancy in the parent and in this build:
     they must be equal, symbol by symbol (exit status 1 otherwise);
  2. the new entry points, k_depth_fill<WIDE>: scratch must be 0 and the static LDS 0 (exit status 1 otherwise).  Both add 256 bytes of
     dynamic LDS at launch, the waves' partial sums.
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cameras_kernel_resources as ckr  # noqa: E402


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ckr.ROOT, "stair-step-detector_amd", "lib", "libssd_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a")), os.makedirs(os.path.join(tmp, "b"))
        kp, kt = ckr.kernels(parent, os.path.join(tmp, "a")), ckr.kernels(this, os.path.join(tmp, "b"))
    names = ckr.demangle(sorted(set(kp) | set(kt)))
    bad = 0
    print("# kernel resources, %s code objects: parent commit | this build" % ckr.ARCH)
    print("# v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane; occupancy by arithmetic (see the tool)")
    print()
    print("## 1. every kernel symbol of the parent: parent | this build")
    for n in sorted(kp, key=lambda n: names[n]):
        same = n in kt and ckr.row(kp[n]) == ckr.row(kt[n])
        bad += 0 if same else 1
        print("%-62s %s | %s%s" % (ckr.short(names[n])[:62], ckr.row(kp[n]), ckr.row(kt[n]) if n in kt else "MISSING", "" if same else "   <-- DIFFERS"))
    print("# %d symbols of the parent, %d differ" % (len(kp), bad))
    print()
    print("## 2. new entry points (WIDE = 16-byte loads and stores of a strip of 8 pixels; otherwise 2-byte accesses)")
    new = [n for n in kt if n not in kp]
    for n in sorted(new, key=lambda n: names[n]):
        wrong = kt[n][".private_segment_fixed_size"] != 0 or kt[n][".group_segment_fixed_size"] != 0
        bad += 1 if wrong else 0
        print("%-62s %s%s" % (ckr.short(names[n])[:62], ckr.row(kt[n]), "   <-- SCRATCH OR STATIC LDS" if wrong else ""))
    print("# %d new entry points" % len(new))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
