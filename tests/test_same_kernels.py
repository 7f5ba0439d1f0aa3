"""tools/same_kernels.py - the per-kernel comparison of two builds' device code (no GPU) - checked on the built libraries: a library is
identical to itself, and the product and the test-hook library, which hold different kernels, are told apart as different sets."""
import importlib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
same = importlib.import_module("same_kernels")

LIB = os.path.join(ROOT, "stair-step-detector_amd", "lib", "libssd_hip.so")
HOOKS = os.path.join(ROOT, "stair-step-detector_amd", "lib", "libssd_testhooks.so")

pytestmark = pytest.mark.skipif(not (same.tools_present() and os.path.exists(LIB) and os.path.exists(HOOKS)),
                                reason="needs the built libraries and the ROCm llvm tools")


@pytest.fixture(scope="module")
def product():
    return same.units(LIB)


def test_a_library_is_identical_to_itself(product):
    assert len(product) == 6, "the six translation units with kernels"
    assert all(u[1] and set(u[1]) <= set(u[0]) and all(u[0][k] for k in u[1]) for u in product), "every kernel has a metadata record and instructions"
    lines, differ, sets = same.compare(product, same.units(LIB))
    assert (differ, sets) == (0, False), lines
    assert len(lines) == 6 and all(l.endswith("identical") for l in lines), lines


def test_one_changed_instruction_or_argument_is_found(product):
    other = [(dict(u[0]), dict(u[1])) for u in product]
    k = sorted(other[3][1])[0]
    other[3][0][k] = other[3][0][k][:-1] + ["s_nop 0 // BF800000"]
    k2 = sorted(other[4][1])[0]
    other[4][1][k2] = [l.replace(".size:", ".size: 1") for l in other[4][1][k2]]
    lines, differ, sets = same.compare(product, other)
    assert (differ, sets) == (2, False), lines
    assert any(k in l and "instructions" in l for l in lines) and any(k2 in l and "metadata" in l for l in lines), lines


def _doctored(product, prefix, field=None, value=None):
    """a copy of `product` with one more instruction in the first kernel whose short name starts with `prefix`, and, given `field`,
    that field of its metadata record set to `value`; -> (copy, the kernel's symbol)"""
    other = [(dict(u[0]), dict(u[1])) for u in product]
    for u in other:
        for k in sorted(u[1]):
            if same.ckr.short(same.ckr.demangle([k])[k]).startswith(prefix):
                u[0][k] = u[0][k] + ["s_nop 0 // BF800000"]
                if field:
                    assert any(re.match(r"^    %s:\s*\d+$" % re.escape(field), l) for l in u[1][k]), u[1][k]
                    u[1][k] = [re.sub(r"^(    %s:\s*)\d+$" % re.escape(field), r"\g<1>%d" % value, l) for l in u[1][k]]
                return other, k
    raise AssertionError("no kernel " + prefix)


def test_a_symbol_inside_the_pattern_may_differ(product):
    other, k = _doctored(product, "k_risers<")
    lines, differ, sets = same.compare(product, other, re.compile(r"^k_risers(_cams)?<"))
    assert (differ, sets) == (0, False), lines
    rows = [l for l in lines if l.startswith("    may differ: k_risers<")]
    assert len(rows) == 1 and " | " in rows[0] and "scr0" in rows[0] and "w/SIMD" in rows[0] and "code" in rows[0], lines
    a, b = (int(x) for x in re.findall(r"code(\d+)", rows[0]))
    assert b == a + 4, "the doctored kernel is one 4-byte instruction longer: " + rows[0]
    assert not any(l.startswith("    differs:") for l in lines), lines


def test_a_symbol_outside_the_pattern_may_not(product):
    other, k = _doctored(product, "k_risers<")
    lines, differ, sets = same.compare(product, other, re.compile(r"^k_riser_labels"))
    assert (differ, sets) == (1, False), lines
    assert any(l.startswith("    differs:") and k in l and "instructions" in l for l in lines), lines
    assert not any(l.startswith("    may differ:") for l in lines), lines


@pytest.mark.parametrize("field, value, word", [(".private_segment_fixed_size", 16, "scratch"), (".group_segment_fixed_size", 8, "lds bytes"),
                                                (".vgpr_count", 256, "fewer waves")])
def test_a_symbol_inside_the_pattern_keeps_its_resources(product, field, value, word):
    other, k = _doctored(product, "k_risers<", field, value)
    lines, differ, sets = same.compare(product, other, re.compile(r"^k_risers(_cams)?<"))
    assert (differ, sets) == (1, False), lines
    assert any(l.startswith("    differs:") and k in l and word in l for l in lines), lines


def test_the_hook_library_is_a_different_set(product):
    lines, differ, sets = same.compare(product, same.units(HOOKS))
    assert sets, lines


def test_the_command_line_says_so():
    import subprocess
    tool = os.path.join(ROOT, "tools", "same_kernels.py")
    r = subprocess.run([sys.executable, tool, HOOKS, HOOKS], capture_output=True, text=True)
    assert r.returncode == 0 and "verdict: identical" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, tool, HOOKS, LIB], capture_output=True, text=True)
    assert r.returncode != 0 and "DIFFERENT SETS" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, tool, HOOKS, HOOKS, "--may-differ", "^k_"], capture_output=True, text=True)
    assert r.returncode == 0 and "verdict: identical (" in r.stdout, r.stdout + r.stderr
