#!/usr/bin/env python3
"""tools/same_kernels.py LIB_A LIB_B — is the device code of two builds of a library the same, kernel by kernel?  (no GPU needed)

    python tools/same_kernels.py PARENT/libssd_hip.so stair-step-detector_amd/lib/libssd_hip.so > profiles/launch_layer_same_kernels.txt

For a change that must not touch device code (host-side launchers, the C ABI).  Pulls every gfx950 code object out of both libraries
(llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle: one bundle per translation unit, as
tools/cameras_kernel_resources.py does) and compares, translation unit by translation unit and symbol by symbol,
  - the set of symbols that hold code,
  - each symbol's disassembly (llvm-objdump -d) with the addresses, the address in front of each encoding and the <symbol+offset>
    annotations of branches removed: the instructions and their encodings are left (and not the run of zero bytes llvm-objdump shows
    as "..." behind a symbol: the padding up to the next symbol's alignment, which belongs to where the symbol lies),
  - each kernel's record in the metadata note (llvm-readelf --notes): registers, LDS, scratch, kernarg size, every argument.
By symbol and not by the files' bytes, because the compiler emits kernels in the order in which the HOST code first names them: a
launcher that is only rearranged moves them around in the code object and leaves every one of them as it was.
Prints a line per translation unit and a verdict; exit status 0 only for "identical".
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")
ARCH = "gfx950"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf")


def tools_present():
    return all(os.path.exists(os.path.join(LLVM, t)) for t in TOOLS)


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, capture_output=True, text=True).stdout


def code_objects(lib, tmp):
    """the gfx950 code object of every translation unit of the library that has one, in the library's order"""
    fat = os.path.join(tmp, "fatbin")
    run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "discard.so"))
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


def disassembly(co):
    """{symbol: [instruction with its encoding, positions removed]}"""
    out, name = {}, None
    for line in run("llvm-objdump", "-d", co).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and re.match(r"^\s+\S", line) and line.strip() != "...":     # "...": zero bytes up to the next symbol's alignment
            line = re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line)            # where the instruction lies
            line = re.sub(r"\s*<[^<>]*(<[^<>]*>[^<>]*)*>\s*$", "", line)   # <symbol+offset> of a branch target (a symbol may hold template brackets)
            out[name].append(" ".join(line.split()))
    return out


def metadata(co):
    """{kernel symbol: its record in the amdhsa.kernels note, line by line}"""
    out, rec, inside = {}, None, False

    def close():
        if rec:
            names = [m.group(1).strip().strip("'") for m in (re.match(r"^(?:  - |    )\.name:\s*(.*)$", l) for l in rec) if m]
            out[names[0] if names else "?%d" % len(out)] = rec

    for line in run("llvm-readelf", "--notes", co).split("\n"):
        if re.match(r"^amdhsa\.kernels:", line):
            inside = True
        elif inside and re.match(r"^  - ", line):
            close()
            rec = [line]
        elif inside and re.match(r"^\S", line):
            close()
            rec, inside = None, False
        elif inside and rec is not None:
            rec.append(line)
    close()
    return out


def units(lib):
    """[(disassembly, metadata)] of the translation units of `lib` that hold device code"""
    tmp = tempfile.mkdtemp(prefix="ssd_same_")
    try:
        res = [(disassembly(co), metadata(co)) for co in code_objects(lib, tmp)]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return [u for u in res if u[0] or u[1]]


def label(unit):
    """a translation unit by its kernels: how many, and the first by name"""
    names = sorted(unit[1]) or sorted(unit[0])
    d = subprocess.run(["c++filt", names[0]], capture_output=True, text=True).stdout.strip() if shutil.which("c++filt") else names[0]
    return "%3d kernels, %3d symbols (%s ...)" % (len(unit[1]), len(unit[0]), re.sub(r"\(.*$", "", re.sub(r"^void ", "", d))[:48])


def compare(a, b):
    """-> (lines, symbols that differ, whether the sets of symbols differ)"""
    lines, differ, sets = [], 0, False
    if len(a) != len(b):
        sa, sb = set().union(*[set(u[0]) for u in a] or [set()]), set().union(*[set(u[0]) for u in b] or [set()])
        lines.append("translation units with device code: %d | %d; symbols: %d | %d, %d only in A, %d only in B"
                     % (len(a), len(b), len(sa), len(sb), len(sa - sb), len(sb - sa)))
        return lines, 0, True
    for i, (ua, ub) in enumerate(zip(a, b)):
        only_a, only_b = sorted(set(ua[0]) - set(ub[0])), sorted(set(ub[0]) - set(ua[0]))
        only_a += [k for k in sorted(set(ua[1]) - set(ub[1])) if k not in only_a]
        only_b += [k for k in sorted(set(ub[1]) - set(ua[1])) if k not in only_b]
        bad = []
        for s in sorted(set(ua[0]) & set(ub[0])):
            what = []
            if ua[0][s] != ub[0][s]:
                what.append("instructions")
            if s in ua[1] and s in ub[1] and ua[1][s] != ub[1][s]:
                what.append("metadata")
            if what:
                bad.append("%s: %s" % (s, " and ".join(what)))
        n_ins = sum(len(v) for v in ua[0].values())
        verdict = "identical" if not (bad or only_a or only_b) else "DIFFERENT"
        lines.append("unit %d: %s: %d instructions compared: %s" % (i, label(ua), n_ins, verdict))
        for s in only_a:
            lines.append("    only in A: " + s)
        for s in only_b:
            lines.append("    only in B: " + s)
        for s in bad:
            lines.append("    differs: " + s)
        differ += len(bad)
        sets = sets or bool(only_a or only_b)
    return lines, differ, sets


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    if not tools_present():
        sys.exit("the ROCm llvm tools (%s) are not under %s" % (", ".join(TOOLS), LLVM))
    a, b = units(sys.argv[1]), units(sys.argv[2])
    lines, differ, sets = compare(a, b)
    print("# device code of two builds, %s code objects, symbol by symbol: A = %s | B = %s" % (ARCH, sys.argv[1], sys.argv[2]))
    print("\n".join(lines))
    if sets:
        print("verdict: DIFFERENT SETS of symbols")
    elif differ:
        print("verdict: DIFFERENT (%d symbols)" % differ)
    else:
        print("verdict: identical (%d translation units, %d kernels, every instruction, encoding and metadata record)" % (len(a), sum(len(u[1]) for u in a)))
    return 1 if (sets or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
