#!/usr/bin/env python3
"""Kernel resources of the cameras build beside its parent, from the code objects alone (no GPU needed).

    python tools/cameras_kernel_resources.py PARENT/libssd_hip.so [THIS/libssd_hip.so] > profiles/cameras_kernel_resources.txt

Reads the gfx950 code object out of each library (llvm-objcopy, clang-offload-bundler, llvm-readelf --notes; one bundle per translation unit) and prints
  1. every kernel symbol of the parent with VGPRs / AGPRs / SGPRs / LDS / scratch / occupancy in the parent and in this build:
     they must be equal, symbol by symbol (exit status 1 otherwise);
  2. every *_cams entry point beside its one-calibration sibling (the same template arguments); scratch must be 0 wherever the
     sibling's is (exit status 1 otherwise).
Occupancy: waves per SIMD the registers allow (512 unified VGPRs per SIMD in granules of 8, at most 8 waves) and workgroups per
CU the LDS allows (160 KiB), as MI355X_MICROARCH-style arithmetic, not a measurement.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
ARCH = "gfx950"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".max_flat_workgroup_size")


MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib, tmp):
    """the gfx950 code object of every translation unit of the library (.hip_fatbin holds one bundle per unit)"""
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "discard.so")], check=True)
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for i, at in enumerate(starts):
        piece = "%s.%d" % (fat, i)
        with open(piece, "wb") as f:
            f.write(data[at:starts[i + 1] if i + 1 < len(starts) else len(data)])
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + piece, "--output=" + piece + ".co",
                            "--targets=hipv4-amdgcn-amd-amdhsa--" + ARCH], capture_output=True)
        if r.returncode == 0 and os.path.exists(piece + ".co") and os.path.getsize(piece + ".co") > 0:
            out.append(piece + ".co")
    return out


def kernels(lib, tmp):
    res = {}
    for co in code_objects(lib, tmp):
        res.update(kernels_of(co))
    return res


def kernels_of(co):
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    res, cur = {}, None
    for line in notes.splitlines():
        top = re.match(r"  - (\.[a-z_]+):\s*(.*)$", line)          # a kernel's record opens at this indentation (its arguments lie deeper)
        m = top or re.match(r"    (\.[a-z_]+):\s*(.*)$", line)
        if top:
            cur = {}
        if not m or cur is None:
            continue
        key, val = m.group(1), m.group(2).strip().strip("'")
        if key in FIELDS:
            cur[key] = int(val)
        elif key == ".name":
            res[val] = cur
    return res


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def occupancy(k):
    regs = (k[".vgpr_count"] - k[".agpr_count"] + 3) // 4 * 4 + k[".agpr_count"] if k[".agpr_count"] else k[".vgpr_count"]
    gran = max(8, (regs + 7) // 8 * 8)
    waves = min(8, 512 // gran)
    lds = k[".group_segment_fixed_size"]
    return "%dw/SIMD" % waves + (" %dwg/CU(LDS)" % (163840 // lds) if lds else "")


def row(k):
    return "v%-3d a%-3d s%-3d lds%-6d scr%-4d %s" % (k[".vgpr_count"], k[".agpr_count"], k[".sgpr_count"], k[".group_segment_fixed_size"],
                                                   k[".private_segment_fixed_size"], occupancy(k))


def short(d):
    d = re.sub(r"^(void )?ssd::", "", d)
    return re.sub(r"\(.*$", "", d)


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "stair-step-detector_amd", "lib", "libssd_hip.so")
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "a")), os.makedirs(os.path.join(tmp, "b"))
        kp, kt = kernels(parent, os.path.join(tmp, "a")), kernels(this, os.path.join(tmp, "b"))
    names = demangle(sorted(set(kp) | set(kt)))
    bad = 0
    print("# kernel resources, %s code objects: parent commit | this build" % ARCH)
    print("# v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane; occupancy by arithmetic (see the tool)")
    print()
    print("## 1. every kernel symbol of the parent: parent | this build")
    for n in sorted(kp, key=lambda n: names[n]):
        same = n in kt and row(kp[n]) == row(kt[n])
        bad += 0 if same else 1
        print("%-62s %s | %s%s" % (short(names[n])[:62], row(kp[n]), row(kt[n]) if n in kt else "MISSING", "" if same else "   <-- DIFFERS"))
    print("# %d symbols of the parent, %d differ" % (len(kp), bad))
    print()
    print("## 2. new entry points beside their one-calibration siblings: sibling | cameras entry point")
    new = [n for n in kt if n not in kp]
    by_short = {short(names[n]): n for n in kt}
    for n in sorted(new, key=lambda n: names[n]):
        s = short(names[n])
        sib = by_short.get(s.replace("_cams", "", 1))
        if sib is None:
            print("%-62s (no sibling) | %s" % (s[:62], row(kt[n])))
            continue
        worse = kt[sib][".private_segment_fixed_size"] == 0 and kt[n][".private_segment_fixed_size"] != 0
        bad += 1 if worse else 0
        print("%-62s %s | %s%s" % (s[:62], row(kt[sib]), row(kt[n]), "   <-- SCRATCH" if worse else ""))
    print("# %d new entry points" % len(new))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
