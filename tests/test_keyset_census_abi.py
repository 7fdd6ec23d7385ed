"""The key census, CPU side (no GPU): the exports of include/dsv.h against the binding's signature table, the Rust
shim and the C++ mirror; the two workspace formulas against a restatement; the calls before dsv_init; the register
budget of the census kernels from the cross-compiled gfx950 assembly; and the lookup unit, which the census reuses
and must not touch."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import pytest

from abi_model import POINTS, _up, cap_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"single": 0, "double": 1, "vargen": 2}

DEV_TAIL = ("void *key_idx_out, void *hits, void *miss_rep, void *miss_count, void *totals, void *workspace, "
            "size_t workspace_bytes, void *stream);")
HOST_TAIL = "uint32_t *key_idx_out, uint32_t *hits, uint32_t *miss_rep, uint32_t *miss_count, size_t totals[4]);"
# the declarations of include/dsv.h, comments removed, and each one's code in schnorr_amd._lib.SIGNATURES
DECLARED = {
    "dsv_keyset_census_workspace_bytes": ("size_t dsv_keyset_census_workspace_bytes(size_t n);", "zz"),
    "dsv_keyset_census_mont_workspace_bytes":
        ("size_t dsv_keyset_census_mont_workspace_bytes(int scheme, size_t n);", "ziz"),
    "dsv_keyset_census_dev": ("int dsv_keyset_census_dev(const dsv_keyset *ks, const void *key_a, const void *key_b, "
                              "size_t n, " + DEV_TAIL, "ipppzppppppzp"),
    "dsv_keyset_census_wire_dev": ("int dsv_keyset_census_wire_dev(const dsv_keyset *ks, const void *pk_records, "
                                   "size_t n, " + DEV_TAIL, "ippzppppppzp"),
    "dsv_keyset_census_mont_dev": ("int dsv_keyset_census_mont_dev(const dsv_keyset *ks, const void *key_a_uvz, "
                                   "const void *key_b_uvz, size_t n, " + DEV_TAIL, "ipppzppppppzp"),
    "dsv_keyset_census": ("int dsv_keyset_census(const dsv_keyset *ks, const uint8_t *key_a, const uint8_t *key_b, "
                          "size_t n, " + HOST_TAIL, "ipppzppppp"),
    "dsv_keyset_census_wire": ("int dsv_keyset_census_wire(const dsv_keyset *ks, const uint8_t *pk_records, size_t n, "
                               + HOST_TAIL, "ippzppppp"),
    "dsv_keyset_census_mont_cols": ("int dsv_keyset_census_mont_cols(const dsv_keyset *ks, const dsv_column *cols, "
                                    "size_t n, " + HOST_TAIL, "ippzppppp"),
    "dsv_debug_census_lds_keys": ("int dsv_debug_census_lds_keys(void);", "i"),
}


def test_exports_declarations_and_signature_table():
    from schnorr_amd import _lib

    L = _lib.load()
    with open(os.path.join(ROOT, "include", "dsv.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    flat = " ".join(text.split()).replace(" ,", ",").replace("( ", "(").replace(" )", ")")
    with open(os.path.join(ROOT, "rust", "dusk-schnorr-gpu", "src", "lib.rs")) as f:
        shim = f.read()
    for name, (decl, code) in DECLARED.items():
        assert " ".join(decl.split()) in flat, name
        assert _lib.SIGNATURES[name] == code, name
        fn = getattr(L, name)
        assert fn.restype is _lib._CTYPES[code[0]] and list(fn.argtypes) == [_lib._CTYPES[c] for c in code[1:]], name
        assert "pub fn %s(" % name in shim, name
    assert sorted(n for n in _lib.SYMBOLS if "census" in n) == sorted(DECLARED)


def test_cpp_mirror_and_python_surface():
    with open(os.path.join(ROOT, "include", "dusk_schnorr.hpp")) as f:
        hpp = f.read()
    assert "struct KeyCensus" in hpp and "KeyCensus census(" in hpp and "dsv_keyset_census_mont_cols(" in hpp
    from schnorr_amd import engine as E
    from schnorr_amd import keycache

    for name in ("census", "census_wire", "census_mont_cols", "census_dev", "census_wire_dev", "census_mont_dev"):
        assert callable(getattr(E.KeySet, name)), name
    assert callable(E.keyset_census_workspace_bytes) and callable(E.keyset_census_mont_workspace_bytes)
    assert "replace" in keycache.KeyCache.maintain.__doc__ and "captur" in keycache.KeyCache.maintain.__doc__


def test_workspace_formulas():
    """slots + counts for keyset_index_cap(n), each rounded to 256; the typed form adds the normalised key columns,
    the validity bytes and the prefix products ((n + 32) * 36 B per key point), each rounded to 256"""
    from schnorr_amd import engine as E

    table = lambda n: 2 * _up(4 * cap_of(n))
    sizes = [0, 1, 31, 32, 33, 63, 64, 65, 4099, (1 << 18) + 5, (1 << 20) + 257, 1 << 28]
    assert [E.keyset_census_workspace_bytes(n) for n in sizes] == [table(n) for n in sizes]
    assert E.keyset_census_workspace_bytes(64) == 2 * 4 * 128 and E.keyset_census_workspace_bytes(1) == 512
    for scheme, np_ in POINTS.items():
        want = [table(n) + np_ * _up(64 * n) + _up(n) + _up(np_ * (n + 32) * 36) for n in sizes]
        got = [E.keyset_census_mont_workspace_bytes(scheme, n) for n in sizes]
        assert got == want, scheme
        assert all(a <= b for a, b in zip(got, got[1:])), scheme
    L = __import__("schnorr_amd._lib", fromlist=["load"]).load()
    for scheme in (-1, 3, 99):
        assert L.dsv_keyset_census_mont_workspace_bytes(scheme, 100) == 0
    plain = [E.keyset_census_workspace_bytes(n) for n in range(0, 5000, 7)]
    assert all(a <= b for a, b in zip(plain, plain[1:]))
    assert L.dsv_debug_census_lds_keys() == 4096  # the default, before any dsv_init


def test_calls_before_init():
    """in a process of its own, before and without dsv_init: every census call with a NULL handle is told that
    nothing is up — whatever its other arguments are, n = 0 and n beyond every limit included — and writes nothing;
    DSV_CENSUS_LDS_KEYS is not read before dsv_init"""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
keys = np.zeros((4, 96), np.uint8)
out = np.full(16, 7, np.uint32)
totals = (ctypes.c_size_t * 4)(9, 9, 9, 9)
col = (_lib.Column * 2)()
p = lambda a: a.ctypes.data
NOT_INITIALIZED = -1
for n in (0, 4, 1 << 40):
    assert L.dsv_keyset_census_dev(None, p(keys), p(keys), n, p(out), p(out), p(out), p(out), p(out), p(out), 64, None) == NOT_INITIALIZED
    assert b"dsv_init" in L.dsv_last_error()
    assert L.dsv_keyset_census_wire_dev(None, p(keys), n, None, None, p(out), p(out), p(out), p(out), 64, None) == NOT_INITIALIZED
    assert L.dsv_keyset_census_mont_dev(None, p(keys), None, n, None, None, p(out), p(out), p(out), p(out), 64, None) == NOT_INITIALIZED
    assert L.dsv_keyset_census(None, p(keys), p(keys), n, p(out), p(out), p(out), p(out), totals) == NOT_INITIALIZED
    assert L.dsv_keyset_census_wire(None, p(keys), n, p(out), p(out), p(out), p(out), totals) == NOT_INITIALIZED
    assert L.dsv_keyset_census_mont_cols(None, col, n, p(out), p(out), p(out), p(out), totals) == NOT_INITIALIZED
    assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_keyset_census_dev(None, None, None, 0, None, None, None, None, None, None, 0, None) == NOT_INITIALIZED
assert (out == 7).all() and list(totals) == [9, 9, 9, 9]
assert L.dsv_debug_census_lds_keys() == 4096
print("ok")
""" % ROOT
    env = dict(os.environ, DSV_CENSUS_LDS_KEYS="0")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# VGPRs the compiler gives the census kernels, pinned as ceilings
VGPR_CEILING = {"k_census_clear": 16, "k_census_report": 17, "AffineKeyILi1": 58, "AffineKeyILi2": 87,
                "RecordKeyILi1": 42, "RecordKeyILi2": 58}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_census_kernels_stay_in_registers():
    """k_keyed_census.hip: the clearing, the census of every key form and the report use no scratch memory, spill no
    VGPR, take no AGPR and stay within the recorded VGPR counts"""
    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    info = _kernel_info(_asm(os.path.join(CSRC, "k_keyed_census.hip"), _stamp()))
    kernels = {name: k for name, k in info.items() if "vgprs" in k}
    assert len(kernels) == 6, sorted(kernels)
    for tag, ceiling in VGPR_CEILING.items():
        hits = [name for name in kernels if tag in name]
        assert len(hits) == 1, (tag, sorted(kernels))
        k = kernels[hits[0]]
        assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0 and k["agprs"] == 0, (tag, k)
        assert k["vgprs"] <= ceiling, (tag, k)
    assert sum("k_censusI" in name for name in kernels) == 4
    # the lookup and the append stay in their own unit
    assert not [name for name in kernels if "k_index_" in name]


def test_lookup_unit_is_untouched():
    """the census reuses keyed_lookup.h's walk and key forms and leaves k_keyed_lookup.hip byte for byte as it was"""
    with open(os.path.join(ROOT, "schnorr_amd", "csrc", "k_keyed_lookup.hip"), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == \
            "a6073231ebe3e11ef90b9119f226e133823d34301933a69cf1278575921365ad"
    from schnorr_amd import build as B

    assert "k_keyed_census.hip" in B.UNITS and "dsv_keyed_census.hip" in B.UNITS
    with open(os.path.join(ROOT, "schnorr_amd", "csrc", "k_keyed_census.hip")) as f:
        text = f.read()
    assert "#define DSV_INDEX_KERNELS" in text and '#include "keyed_census.h"' in text
    # the walk is keyed_lookup.h's, reached through its guarded form find_key (a set of no keys has no index)
    for name in ("find_key<", "home_hash<", "same_words<", "AffineKey<", "RecordKey<"):
        assert name in text, name
    with open(os.path.join(ROOT, "schnorr_amd", "csrc", "keyed_lookup.h")) as f:
        assert re.search(r"find_key\([^)]*\)\s*\{\s*return k \? walk_index<W>\(", f.read())
