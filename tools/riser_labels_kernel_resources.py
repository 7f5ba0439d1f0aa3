#!/usr/bin/env python3
"""Kernel resources of the riser-labels build beside its parent, from the code objects alone (no GPU needed).

    python tools/riser_labels_kernel_resources.py PARENT/libssd_hip.so [THIS/libssd_hip.so] > profiles/riser_labels_kernel_resources.txt

With the readers of tools/cameras_kernel_resources.py and tools/riser_fit_kernel_resources.py:
  1. every kernel symbol of the parent in the parent and in this build: registers, LDS, scratch and code size must agree line for line
     (exit status 1 otherwise) - the riser labels are a body of their own (k_riser_labels), launched behind k_labels and the riser pass
     only while riser labels and risers are on;
  2. the new instantiations, k_riser_labels<SRC> and k_riser_labels_cams<SRC>, each beside the k_risers instantiation whose cells it
     walks once more; scratch must be 0 (exit status 1 otherwise).
"""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cameras_kernel_resources as ckr  # noqa: E402
from riser_fit_kernel_resources import kernels_with_size, row  # noqa: E402


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ckr.ROOT, "stair-step-detector_amd", "lib", "libssd_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a")), os.makedirs(os.path.join(tmp, "b"))
        kp, kt = kernels_with_size(parent, os.path.join(tmp, "a")), kernels_with_size(this, os.path.join(tmp, "b"))
    names = ckr.demangle(sorted(set(kp) | set(kt)))
    short = {n: ckr.short(names[n]) for n in names}
    bad = differ = 0
    print("# kernel resources, %s code objects: parent commit | this build" % ckr.ARCH)
    print("# v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane, code = bytes of the kernel's code;")
    print("# occupancy by arithmetic (tools/cameras_kernel_resources.py)")
    print()
    print("## 1. every kernel symbol of the parent: parent | this build")
    for n in sorted(kp, key=lambda n: names[n]):
        same = n in kt and row(kp[n]) == row(kt[n])
        differ += 0 if same else 1
        print("%-40s %s | %s%s" % (short[n][:40], row(kp[n]), row(kt[n]) if n in kt else "MISSING", "" if same else "   <-- DIFFERS"))
    print("# %d symbols, %d differ" % (len(kp), differ))
    print()
    bad += differ
    print("## 2. new instantiations beside the k_risers instantiation whose cells each walks once more: k_risers | k_riser_labels")
    new = [n for n in kt if n not in kp]
    by_short = {short[n]: n for n in kt}
    for n in sorted(new, key=lambda n: names[n]):
        sib = by_short.get(short[n].replace("k_riser_labels", "k_risers", 1))
        scratch = kt[n][".private_segment_fixed_size"] != 0
        stray = not short[n].startswith("k_riser_labels")
        bad += 1 if scratch or stray else 0
        print("%-40s %s | %s%s%s" % (short[n][:40], row(kt[sib]) if sib else "(no sibling)", row(kt[n]), "   <-- SCRATCH" if scratch else "",
                                     "   <-- NOT A RISER LABELS KERNEL" if stray else ""))
    print("# %d new entry points" % len(new))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
