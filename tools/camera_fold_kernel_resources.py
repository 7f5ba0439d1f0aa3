#!/usr/bin/env python3
"""Kernel resources of the camera-fold build beside its parent, from the code objects alone (no GPU needed).

    python tools/camera_fold_kernel_resources.py PARENT/libssd_hip.so [THIS/libssd_hip.so] > profiles/camera_fold_kernel_resources.txt

With the readers of tools/cameras_kernel_resources.py and tools/surface_refit_kernel_resources.py (the method of
tools/camera_surfaces_refit_kernel_resources.py):
  1. every kernel symbol of the parent, in the parent and in this build: registers, LDS, scratch and code size must agree line for
     line (exit status 1 otherwise) - the new kernels live in a translation unit of their own (ssd_kernels_fold.hip), so no code object
     of the chain may move;
  2. the new symbols: k_camera_fold and k_camera_ground_gates, no other, neither with scratch (exit status 1 otherwise).
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cameras_kernel_resources as ckr  # noqa: E402
import surface_refit_kernel_resources as srk  # noqa: E402


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ckr.ROOT, "stair-step-detector_amd", "lib", "libssd_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a")), os.makedirs(os.path.join(tmp, "b"))
        kp, kt = srk.kernels_with_size(parent, os.path.join(tmp, "a")), srk.kernels_with_size(this, os.path.join(tmp, "b"))
    names = ckr.demangle(sorted(set(kp) | set(kt)))
    short = {n: ckr.short(names[n]) for n in names}
    bad = differ = 0
    print("# kernel resources, %s code objects: parent commit | this build" % ckr.ARCH)
    print("# v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane, code = bytes of the kernel's code;")
    print("# occupancy by arithmetic (tools/cameras_kernel_resources.py)")
    print()
    print("## 1. every kernel symbol of the parent: parent | this build")
    for n in sorted(kp, key=lambda n: names[n]):
        same = n in kt and srk.row(kp[n]) == srk.row(kt[n])
        differ += 0 if same else 1
        print("%-40s %s | %s%s" % (short[n][:40], srk.row(kp[n]), srk.row(kt[n]) if n in kt else "MISSING", "" if same else "   <-- DIFFERS"))
    print("# %d symbols, %d differ" % (len(kp), differ))
    print()
    print("## 2. new kernel symbols")
    new = sorted((n for n in kt if n not in kp), key=lambda n: names[n])
    for n in new:
        k = kt[n]
        flags = []
        if k[".private_segment_fixed_size"] != 0:
            flags.append("SCRATCH")
        if not short[n].startswith(("k_camera_fold", "k_camera_ground_gates")):
            flags.append("UNEXPECTED")
        bad += 1 if flags else 0
        print("%-40s %s%s" % (short[n][:40], srk.row(k), "   <-- " + ", ".join(flags) if flags else ""))
    print("# %d new entry points" % len(new))
    if len(new) != 2:
        bad += 1
    return 1 if bad or differ else 0


if __name__ == "__main__":
    sys.exit(main())
