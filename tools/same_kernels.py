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

    python tools/same_kernels.py PARENT/libssd_hip.so THIS/libssd_hip.so --may-differ 'k_(labels|risers)' > profiles/extension_kernels_same_kernels.txt

--may-differ REGEX: for a change that rewrites SOME kernels.  A symbol whose demangled name (without "void ssd::" and the argument list)
the pattern matches may differ; for each that does, the two resource rows are printed in the form of tools/riser_labels_kernel_resources.py
(VGPR, AGPR, SGPR, LDS, scratch, waves per SIMD, code size), and it still counts as DIFFERENT if it has scratch, other LDS bytes than in A
or fewer waves per SIMD than in A.  Exit status 0 only if every other symbol is identical and the symbol sets are equal.

    python tools/same_kernels.py PARENT/libssd_hip.so THIS/libssd_hip.so --new '^k_clearance' > profiles/clearance_same_kernels.txt

--new REGEX: for a change that ADDS kernels to a translation unit.  A symbol that only B holds and whose demangled name the pattern matches
is listed with its resource row and does not make the sets differ; every symbol of A must still be there, identical.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cameras_kernel_resources as ckr  # noqa: E402

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


def resources(record, instructions):
    """a kernel's record for ckr.row out of its metadata lines, and '.code_bytes' out of its instructions' encodings"""
    k = {f: 0 for f in ckr.FIELDS}
    for line in record or []:
        m = re.match(r"^(?:  - |    )(\.[a-z_]+):\s*(\d+)\s*$", line)
        if m and m.group(1) in k:
            k[m.group(1)] = int(m.group(2))
    k[".code_bytes"] = 4 * sum(len(re.findall(r"\b[0-9A-Fa-f]{8}\b", line.split("//")[-1])) for line in instructions)
    return k


def row(k):
    return "%s code%-6d" % (ckr.row(k), k[".code_bytes"])


def waves(k):
    return int(ckr.occupancy(k).split("w/SIMD")[0])


def compare(a, b, may_differ=None, new=None):
    """-> (lines, symbols that differ and may not, whether the sets of symbols differ); may_differ, new: compiled patterns (see above)"""
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
        added = [k for k in only_b if new and new.search(ckr.short(ckr.demangle([k])[k]))]
        only_b = [k for k in only_b if k not in added]
        bad, allowed = [], []
        for s in sorted(set(ua[0]) & set(ub[0])):
            what = []
            if ua[0][s] != ub[0][s]:
                what.append("instructions")
            if s in ua[1] and s in ub[1] and ua[1][s] != ub[1][s]:
                what.append("metadata")
            if not what:
                continue
            name = ckr.short(ckr.demangle([s])[s]) if may_differ else s
            if not (may_differ and may_differ.search(name)):
                bad.append("%s: %s" % (s, " and ".join(what)))
                continue
            ka, kb = resources(ua[1].get(s), ua[0][s]), resources(ub[1].get(s), ub[0][s])
            broken = []
            if kb[".private_segment_fixed_size"] != 0:
                broken.append("SCRATCH")
            if kb[".group_segment_fixed_size"] != ka[".group_segment_fixed_size"]:
                broken.append("LDS BYTES")
            if s in ua[1] and waves(kb) < waves(ka):
                broken.append("FEWER WAVES")
            allowed.append("%-44s %s | %s%s" % (name[:44], row(ka), row(kb), "   <-- " + ", ".join(broken) if broken else ""))
            if broken:
                bad.append("%s: %s" % (s, ", ".join(broken).lower()))
        n_ins = sum(len(v) for v in ua[0].values())
        verdict = "DIFFERENT" if (bad or only_a or only_b) else "identical but for %d symbols that may differ" % len(allowed) if allowed else "identical"
        lines.append("unit %d: %s: %d instructions compared: %s" % (i, label(ua), n_ins, verdict))
        for s in only_a:
            lines.append("    only in A: " + s)
        for s in only_b:
            lines.append("    only in B: " + s)
        for s in added:
            lines.append("    new in B: %-46s %s" % (ckr.short(ckr.demangle([s])[s])[:46], row(resources(ub[1].get(s), ub[0].get(s, [])))))
        for s in allowed:
            lines.append("    may differ: " + s)
        for s in bad:
            lines.append("    differs: " + s)
        differ += len(bad)
        sets = sets or bool(only_a or only_b)
    return lines, differ, sets


def main():
    argv, pattern, new = sys.argv[1:], None, None
    if "--may-differ" in argv[:-1]:
        at = argv.index("--may-differ")
        pattern = re.compile(argv[at + 1])
        del argv[at:at + 2]
    if "--new" in argv[:-1]:
        at = argv.index("--new")
        new = re.compile(argv[at + 1])
        del argv[at:at + 2]
    if len(argv) != 2:
        sys.exit(__doc__)
    if not tools_present():
        sys.exit("the ROCm llvm tools (%s) are not under %s" % (", ".join(TOOLS), LLVM))
    a, b = units(argv[0]), units(argv[1])
    lines, differ, sets = compare(a, b, pattern, new)
    allowed = sum(1 for l in lines if l.startswith("    may differ: "))
    added = sum(1 for l in lines if l.startswith("    new in B: "))
    print("# device code of two builds, %s code objects, symbol by symbol: A = %s | B = %s" % (ARCH, argv[0], argv[1]))
    if new:
        print("# new in B: %s; their rows: v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane," % new.pattern)
        print("# occupancy by arithmetic (tools/cameras_kernel_resources.py), code = bytes of the symbol's instructions")
    if pattern:
        print("# may differ: %s; their rows A | B: v = VGPRs, a = AGPRs, s = SGPRs, lds / scr = bytes of LDS / scratch per workgroup / lane," % pattern.pattern)
        print("# occupancy by arithmetic (tools/cameras_kernel_resources.py), code = bytes of the symbol's instructions")
    print("\n".join(lines))
    if sets:
        print("verdict: DIFFERENT SETS of symbols")
    elif differ:
        print("verdict: DIFFERENT (%d symbols)" % differ)
    elif allowed:
        print("verdict: identical but for %d symbols that may differ, each without scratch, with A's LDS bytes and no fewer waves per SIMD (%d symbols in all)"
              % (allowed, sum(len(u[0]) for u in a)))
    elif added:
        print("verdict: every symbol of A identical (%d translation units, %d kernels, every instruction, encoding and metadata record); %d new symbols in B"
              % (len(a), sum(len(u[1]) for u in a), added))
    else:
        print("verdict: identical (%d translation units, %d kernels, every instruction, encoding and metadata record)" % (len(a), sum(len(u[1]) for u in a)))
    return 1 if (sets or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
