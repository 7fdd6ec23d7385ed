"""Key sets as a key cache, CPU side (no GPU): the exports of the open-set verify by key value
(dsv_verify_keyed_open*, include/dsv.h), the workspace formula, the calls before dsv_init, and the register budget
of k_keyed_open.hip's kernels against the kernel k_verify_listed mirrors."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN_SYMBOLS = ("dsv_keyed_open_workspace_bytes", "dsv_verify_keyed_open_dev", "dsv_verify_keyed_open")
# launch.h: one-wave workgroups, at most 4096 of them; a per-lane window table of 9 entries x 36 words, three per
# lane in the workspace (dsv_host.h: kTablesPerLane)
VERIFY_BLOCK, MAX_VERIFY_GRID, LANE_TABLE_BYTES, TABLES_PER_LANE = 64, 4096, 9 * 36 * 4, 3


def _up(x, a=256):
    return (x + a - 1) // a * a


def var_table_bytes(n):
    return min((n + VERIFY_BLOCK - 1) // VERIFY_BLOCK, MAX_VERIFY_GRID) * VERIFY_BLOCK * LANE_TABLE_BYTES * TABLES_PER_LANE


def test_open_symbols_are_exported_and_declared():
    from schnorr_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsv.h")).read()
    for name in OPEN_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
        assert name + "(" in header, name


def test_open_workspace_formula():
    from schnorr_amd import engine as E

    last = -1
    for n in (0, 1, 64, 65, 1 << 16, (1 << 20) + 1):
        want = E.keyed_lookup_workspace_bytes(n) + _up(4 * n) + 256 + var_table_bytes(n)
        got = E.keyed_open_workspace_bytes(n)
        assert got == want, (n, got, want)
        assert got % 256 == 0
        assert got > last, (n, got, last)
        last = got
    assert E.keyed_open_workspace_bytes(0) == 256
    # monotonic over every size up to a few workgroups, and across the point where the grid stops growing
    sizes = list(range(0, 400)) + [MAX_VERIFY_GRID * VERIFY_BLOCK + d for d in (-65, -64, -1, 0, 1, 64, 65)]
    vals = [E.keyed_open_workspace_bytes(n) for n in sizes]
    assert all(a <= b for a, b in zip(vals, vals[1:]))


def test_open_calls_before_init_are_not_initialized():
    """In a process of its own: before any dsv_init both open calls return DSV_ERR_NOT_INITIALIZED for the NULL
    handle that is all a caller can have then, and touch nothing."""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
b = np.zeros((1, 64), np.uint8)
ok = np.full(1, 7, np.uint8)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
n, ws = ctypes.c_size_t(1), ctypes.c_size_t(1 << 20)
misses = ctypes.c_size_t(77)
assert L.dsv_verify_keyed_open(None, p(b), p(b), p(b), p(b), p(b), p(b), n, p(ok), ctypes.byref(misses)) == -1
assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_verify_keyed_open_dev(None, p(b), p(b), p(b), p(b), p(b), p(b), n, p(ok), p(b), ws, None, None) == -1
assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_verify_keyed_open(None, None, None, None, None, None, None, ctypes.c_size_t(0), None, None) == -1
assert misses.value == 77 and ok[0] == 7
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- register budget of k_keyed_open.hip (assembly cached like tests/test_isa_guard.py) ------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_open_kernels_register_budget():
    """k_verify_listed sits on the budget of the kernel it mirrors — 256 VGPRs, two waves per SIMD, no AGPRs — and
    the indirection through the list costs it no scratch: no more scratch bytes and no more spilled VGPRs than
    k_verify_fixed_half of the same chain count, compiled by this run.  k_miss_list stays in registers."""
    from concurrent.futures import ThreadPoolExecutor

    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    stamp = _stamp()
    with ThreadPoolExecutor(2) as ex:
        listed_s, fixed_s = ex.map(lambda u: _asm(os.path.join(CSRC, u), stamp), ("k_keyed_open.hip", "k_verify.hip"))
    listed, fixed = _kernel_info(listed_s), _kernel_info(fixed_s)

    def one(info, needle):
        hits = [k for k in info if needle in k]
        assert len(hits) == 1, (needle, sorted(info))
        return info[hits[0]]

    for chains in (1, 2):
        k = one(listed, "k_verify_listedILi%dE" % chains)
        ref = one(fixed, "k_verify_fixed_halfILi%dE" % chains)
        assert k["occupancy"] == 2 and k["agprs"] == 0 and k["vgprs"] <= 256, k
        assert k["scratch"] <= ref["scratch"], (chains, k, ref)
        assert k["vgpr_spill_count"] <= ref["vgpr_spill_count"], (chains, k, ref)
    miss = one(listed, "k_miss_list")
    assert miss["scratch"] == 0 and miss["vgpr_spill_count"] == 0, miss


# ---- one source per item body (DESIGN.md §10.5 "One body or two", §10.9) ---------------------------------
def test_item_bodies_have_one_source():
    """The unkeyed equations and the helpers of the typed-object front exist once in csrc/: each miss-branch kernel
    includes the fragment its unkeyed kernel includes and neither restates it, and the shared helpers are defined
    once, in a header."""
    import re

    from isa_asm import CSRC

    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}
    code = {f: re.sub(r"//[^\n]*", "", s) for f, s in files.items()}  # (comments may name what they like)
    count = lambda name: {f: n for f, n in ((f, len(re.findall(r"(?<![A-Za-z0-9_])%s\(" % name, s)))
                                            for f, s in code.items()) if n}
    includes = lambda f: set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', code[f], re.M))

    # the fixed-generator body: the scalar preparation and the window loop are written in the fragment alone — the
    # other callers of half_scalars are another method (the eight-lane kernel, k_quad.hip) and the introspection
    # kernel of the tests (k_vargen.hip: k_debug_half_scalars)
    half = "verify_half_item_body.h"
    assert count("half_scalars") == {"halfgcd.h": 1, half: 1, "k_quad.hip": 1, "k_vargen.hip": 1}
    assert count("ext_mul4") == {"common.h": 1, half: 1}
    assert count("build_joint_table") == {"common.h": 1, half: 1}
    for unit in ("k_verify.hip", "k_keyed_open.hip"):
        assert half in includes(unit), unit
        assert code[unit].count('#include "%s"' % half) == 1, unit
    # the var-generator body: k_vargen.hip keeps two calls of its own — k_verify_var_hex, another method, and the
    # introspection kernel k_debug_lattice3 — and the listed unit none
    var = "verify_var_item_body.h"
    assert count("lattice3_scalars") == {"lattice3.h": 1, var: 1, "k_vargen.hip": 2}
    assert count("load_var_entry_raw").keys() == {"common.h", var}
    for unit in ("k_vargen.hip", "k_keyed_open_var.hip"):
        assert var in includes(unit), unit
        assert code[unit].count('#include "%s"' % var) == 1, unit
    # a fragment is text for its two kernels and nobody else's
    for frag, users in ((half, {"k_verify.hip", "k_keyed_open.hip"}), (var, {"k_vargen.hip", "k_keyed_open_var.hip"})):
        assert {f for f in code if frag in includes(f)} == users, frag
        assert "#pragma once" not in code[frag] and "namespace" not in code[frag], frag

    # the typed-object helpers and the index walk: one definition each, in a header both users include
    defined = lambda name: [f for f, s in code.items()
                            if re.search(r"^(?:DSV_DEV|__device__)[^;{}()]*\b%s\(" % name, s, re.M)]
    assert defined("load_z_for_product") == ["normalize_items.h"]
    assert defined("scalars_from_mont_item") == ["normalize_items.h"]
    assert defined("walk_index") == ["keyed_lookup.h"]
    assert [f for f, s in code.items() if re.search(r"\bkTwo5\[", s)] == ["normalize_items.h"]
    for unit in ("k_misc.hip", "k_keyed_open_mont.hip"):
        assert "normalize_items.h" in includes(unit), unit
    assert {f for f, s in code.items() if re.search(r"\bwalk_index\b", s)} == {
        "keyed_lookup.h", "k_keyed_lookup.hip", "k_keyed_open_mont.hip"}
    # a set without an index reads nothing: the guard stands at the fused kernel's call site, not in the walk
    assert re.search(r"key_ok && nkeys \? walk_index<W>\(", code["k_keyed_open_mont.hip"])
