#!/usr/bin/env python3
"""Kernel resources of the trimmed-surface-refit build beside its parent, from the code objects alone (no GPU needed).

    python tools/surface_refit_kernel_resources.py PARENT/libssd_hip.so [THIS/libssd_hip.so] > profiles/surface_refit_kernel_resources.txt

With the readers of tools/cameras_kernel_resources.py, and the size of each kernel's code from the code object's symbol table:
  1. every instantiation of k_surface_moments and k_surface_moments_cams in the parent and in this build: registers, LDS, scratch and
     code size must agree line for line (exit status 1 otherwise) - the refit is a sibling body (k_surface_refit) in a translation
     unit of its own, launched only by ssd_enqueue_surface_refit;
  2. every other kernel symbol of the parent, the same way;
  3. the new instantiations, k_surface_refit<SRC, CHECKS>, each beside the k_surface_moments instantiation it is the sibling of;
     scratch must be 0 (exit status 1 otherwise).
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cameras_kernel_resources as ckr  # noqa: E402


def kernels_with_size(lib, tmp):
    """ckr.kernels, each record with '.code_bytes': the size of the kernel's function symbol"""
    res = {}
    for co in ckr.code_objects(lib, tmp):
        ks = ckr.kernels_of(co)
        syms = subprocess.run([os.path.join(ckr.LLVM, "llvm-readelf"), "--symbols", "--wide", co], check=True, capture_output=True, text=True).stdout
        for line in syms.splitlines():
            f = line.split()
            if len(f) >= 8 and f[3] == "FUNC" and f[7] in ks:
                ks[f[7]][".code_bytes"] = int(f[2], 0)
        res.update(ks)
    return res


def row(k):
    return "%s code%-6d" % (ckr.row(k), k.get(".code_bytes", -1))


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ckr.ROOT, "stair-step-detector_amd", "lib", "libssd_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a")), os.makedirs(os.path.join(tmp, "b"))
        kp, kt = kernels_with_size(parent, os.path.join(tmp, "a")), kernels_with_size(this, os.path.join(tmp, "b"))
    names = ckr.demangle(sorted(set(kp) | set(kt)))
    short = {n: ckr.short(names[n]) for n in names}
    bad = 0

    def compare(title, pick):
        nonlocal bad
        rows = differ = 0
        print(title)
        for n in sorted((n for n in kp if pick(short[n])), key=lambda n: names[n]):
            same = n in kt and row(kp[n]) == row(kt[n])
            differ += 0 if same else 1
            rows += 1
            print("%-40s %s | %s%s" % (short[n][:40], row(kp[n]), row(kt[n]) if n in kt else "MISSING", "" if same else "   <-- DIFFERS"))
        print("# %d symbols, %d differ" % (rows, differ))
        print()
        bad += differ

    product = re.compile(r"^(k_surface_moments|k_surface_moments_cams)<")
    print("# kernel resources, %s code objects: parent commit | this build" % ckr.ARCH)
    print("# v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane, code = bytes of the kernel's code;")
    print("# occupancy by arithmetic (tools/cameras_kernel_resources.py)")
    print()
    compare("## 1. k_surface_moments and k_surface_moments_cams: parent | this build", lambda s: product.match(s) is not None)
    compare("## 2. every other kernel symbol of the parent: parent | this build", lambda s: product.match(s) is None)
    print("## 3. new instantiations beside the k_surface_moments instantiation each is the sibling of: k_surface_moments | k_surface_refit")
    new = [n for n in kt if n not in kp]
    by_short = {short[n]: n for n in kt}
    for n in sorted(new, key=lambda n: names[n]):
        sib = by_short.get(short[n].replace("k_surface_refit", "k_surface_moments", 1))
        scratch = kt[n][".private_segment_fixed_size"] != 0
        bad += 1 if scratch else 0
        print("%-40s %s | %s%s" % (short[n][:40], row(kt[sib]) if sib else "(no sibling)", row(kt[n]), "   <-- SCRATCH" if scratch else ""))
    print("# %d new entry points" % len(new))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
