#!/usr/bin/env python3
"""Kernel resources of the cameras-refit build beside its parent, from the code objects alone (no GPU needed).

    python tools/camera_surfaces_refit_kernel_resources.py PARENT/libssd_hip.so [THIS/libssd_hip.so] > profiles/camera_surfaces_refit_kernel_resources.txt

With the readers of tools/cameras_kernel_resources.py and tools/surface_refit_kernel_resources.py:
  1. every instantiation of k_surface_refit in the parent and in this build: registers, LDS, scratch and code size must agree line
     for line (exit status 1 otherwise) - the one-calibration pass is the yardstick the cameras pass is timed against.  (With its
     body moved into a device function shared with the cameras entry point the lines did NOT agree - 68 bytes of code less, two
     SGPRs more for <0, false> and <1, false> -, so the entry point kept its text and the cameras kernel got a copy of the body:
     DESIGN.md section 7h);
  2. every other kernel symbol of the parent, the same way (camera_of moved from ssd_kernels_cams.hip into ssd_device.h);
  3. the new instantiations, k_surface_refit_cams<SRC, CHECKS>, each beside the k_surface_refit instantiation it is the sibling
     of, with the scalar registers it takes more: scratch must be 0 where the sibling's is, the LDS the sibling's, and the VGPRs
     must allow the sibling's waves per SIMD (exit status 1 otherwise).
"""
import os
import re
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
    bad = 0

    def compare(title, pick):
        nonlocal bad
        rows = differ = 0
        print(title)
        for n in sorted((n for n in kp if pick(short[n])), key=lambda n: names[n]):
            same = n in kt and srk.row(kp[n]) == srk.row(kt[n])
            differ += 0 if same else 1
            rows += 1
            print("%-40s %s | %s%s" % (short[n][:40], srk.row(kp[n]), srk.row(kt[n]) if n in kt else "MISSING", "" if same else "   <-- DIFFERS"))
        print("# %d symbols, %d differ" % (rows, differ))
        print()
        bad += differ

    reshaped = re.compile(r"^k_surface_refit<")
    print("# kernel resources, %s code objects: parent commit | this build" % ckr.ARCH)
    print("# v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane, code = bytes of the kernel's code;")
    print("# occupancy by arithmetic (tools/cameras_kernel_resources.py)")
    print()
    compare("## 1. k_surface_refit: parent | this build", lambda s: reshaped.match(s) is not None)
    compare("## 2. every other kernel symbol of the parent: parent | this build", lambda s: reshaped.match(s) is None)
    print("## 3. new instantiations beside the k_surface_refit instantiation each is the sibling of: k_surface_refit | k_surface_refit_cams")
    new = [n for n in kt if n not in kp]
    by_short = {short[n]: n for n in kt}
    for n in sorted(new, key=lambda n: names[n]):
        sib = by_short.get(short[n].replace("k_surface_refit_cams", "k_surface_refit", 1))
        k = kt[n]
        flags = []
        if sib is None:
            flags.append("NO SIBLING")
        else:
            s = kt[sib]
            if s[".private_segment_fixed_size"] == 0 and k[".private_segment_fixed_size"] != 0:
                flags.append("SCRATCH")
            if k[".group_segment_fixed_size"] != s[".group_segment_fixed_size"]:
                flags.append("LDS")
            if ckr.occupancy(k).split()[0] != ckr.occupancy(s).split()[0]:
                flags.append("WAVES")
        bad += 1 if flags else 0
        print("%-40s %s | %s   s%+d%s" % (short[n][:40], srk.row(kt[sib]) if sib else "(no sibling)", srk.row(k),
                                         k[".sgpr_count"] - kt[sib][".sgpr_count"] if sib else 0, "   <-- " + ", ".join(flags) if flags else ""))
    print("# %d new entry points" % len(new))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
