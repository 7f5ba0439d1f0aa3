#!/usr/bin/env python3
"""Registers, LDS and scratch of every k_predict instantiation, parent build beside this one, from the code objects alone (no GPU needed).

    python tools/predict_kernel_resources.py PARENT/libssd_hip.so [THIS/libssd_hip.so] > profiles/predict_whole_lines_kernel_resources.txt

With the readers of tools/cameras_kernel_resources.py.  Exit status 1 if an instantiation of this build uses scratch memory."""
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cameras_kernel_resources as ckr


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ckr.ROOT, "stair-step-detector_amd", "lib", "libssd_hip.so")
    bad = 0
    for tag, lib in (("parent", parent), ("this build", this)):
        with tempfile.TemporaryDirectory() as tmp:
            ks = ckr.kernels(lib, tmp)
        names = ckr.demangle(sorted(n for n in ks if "k_predict" in n))
        print("%s (vector / accumulator / scalar registers, LDS bytes, scratch bytes, residency)" % tag)
        for n in sorted(names, key=lambda n: names[n]):
            print("  %-28s %s" % (ckr.short(names[n]), ckr.row(ks[n])))
            if tag == "this build" and ks[n][".private_segment_fixed_size"]:
                bad = 1
    return bad


if __name__ == "__main__":
    sys.exit(main())
