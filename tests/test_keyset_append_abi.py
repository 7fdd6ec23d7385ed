"""Key sets that grow, CPU side (no GPU): the new exports and their signatures in include/dsv.h, the size formulas
a reserved set is allocated by, the argument checks of dsv_keyset_create_reserved / dsv_keyset_append* that need no
device, the calls before dsv_init, and the register budget of the affine k_index_append and the guarded k_index_lookup."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from abi_model import POINTS, _up, cap_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_BYTES = 594432
NOT_INITIALIZED, INVALID, TOO_LARGE = -1, -2, -5

SIGNATURES = {
    "dsv_keyset_create_reserved": "int dsv_keyset_create_reserved(int scheme, const uint8_t *pk_uv, "
                                  "const uint8_t *pk2_uv, size_t k, size_t capacity, dsv_keyset **out);",
    "dsv_keyset_append": "int dsv_keyset_append(dsv_keyset *ks, const uint8_t *pk_uv, const uint8_t *pk2_uv, "
                         "size_t m, uint32_t *first_index);",
    "dsv_keyset_append_wire": "int dsv_keyset_append_wire(dsv_keyset *ks, const uint8_t *pk_bytes, size_t m, "
                              "uint32_t *first_index);",
    "dsv_keyset_append_mont_cols": "int dsv_keyset_append_mont_cols(dsv_keyset *ks, const dsv_column *cols, "
                                   "size_t m, uint32_t *first_index);",
    "dsv_keyset_capacity": "int dsv_keyset_capacity(const dsv_keyset *ks, size_t *capacity);",
    "dsv_keyset_key_ok_n": "int dsv_keyset_key_ok_n(const dsv_keyset *ks, uint8_t *out, size_t room, size_t *k_out);",
}


def test_exports_and_declared_signatures():
    from schnorr_amd import _lib

    L = _lib.load()
    with open(os.path.join(ROOT, "include", "dsv.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    flat = " ".join(text.split()).replace(" ,", ",")  # (a comment may stand between a parameter and its comma)
    for name, decl in SIGNATURES.items():
        assert name in _lib.SYMBOLS and getattr(L, name) is not None, name
        assert " ".join(decl.split()) in flat, name


@pytest.mark.parametrize("scheme", sorted(POINTS))
def test_reserved_set_sizes_follow_the_capacity(scheme):
    """a reserved set is allocated by dsv_keyset_bytes / dsv_keyset_index_bytes of its capacity, whatever k is"""
    from schnorr_amd import engine as E

    for capacity in (1, 40, 256, 257, 4096, 16385):
        assert E.keyset_bytes(scheme, capacity) == POINTS[scheme] * capacity * POINT_BYTES + _up(capacity)
        assert E.keyset_index_bytes(scheme, capacity) == _up(POINTS[scheme] * 64 * capacity) + _up(4 * cap_of(capacity))
    assert cap_of(40) == 128 and cap_of(16385) == 65536
    key = np.arange(128, dtype=np.uint8)
    a, b = key[:64], (key[64:] if POINTS[scheme] == 2 else None)
    assert E.keyset_home_slot(scheme, 40, a, b) < 128  # a test aims at slots with the capacity


def test_argument_checks_without_a_device():
    """in a process of its own, before and without dsv_init: the checks of create_reserved come in the order NULL
    out, unknown scheme, capacity < k, capacity > 2^32 - 2, NULL keys — all of them in front of the device — and
    every call that gets that far is told that nothing is initialised"""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
pk = np.zeros((2, 64), np.uint8)
p = pk.ctypes.data_as(ctypes.c_void_p)
sz, null = ctypes.c_size_t, ctypes.c_void_p(None)
NOT_INITIALIZED, INVALID, TOO_LARGE = -1, -2, -5
def reserved(scheme, a, b, k, capacity, out=True):
    h = ctypes.c_void_p(1)
    rc = L.dsv_keyset_create_reserved(scheme, a, b, sz(k), sz(capacity), ctypes.byref(h) if out else None)
    assert h.value is None or not out
    return rc
assert reserved(3, p, p, 5, 2, out=False) == INVALID and b"output" in L.dsv_last_error()
assert reserved(3, p, p, 5, 2) == INVALID and b"scheme" in L.dsv_last_error()
assert reserved(-1, p, p, 1, 2) == INVALID and b"scheme" in L.dsv_last_error()
for scheme in (0, 1, 2):
    assert reserved(scheme, p, p, 2, 1) == INVALID and b"capacity" in L.dsv_last_error()
    assert reserved(scheme, null, null, 2, 1) == INVALID and b"capacity" in L.dsv_last_error()
    assert reserved(scheme, p, p, 2, 2**32 - 1) == TOO_LARGE and b"capacity" in L.dsv_last_error()
    assert reserved(scheme, null, null, 1 << 33, 1 << 33) == TOO_LARGE
    assert reserved(scheme, null, null, 2, 2**32 - 2) == INVALID and b"null pointer" in L.dsv_last_error()
    assert reserved(scheme, p, null, 2, 4) == (NOT_INITIALIZED if scheme == 0 else INVALID)
    assert reserved(scheme, p, p, 2, 2) == NOT_INITIALIZED and b"dsv_init" in L.dsv_last_error()
    assert reserved(scheme, p, p, 2, 2**32 - 2) == NOT_INITIALIZED
    assert reserved(scheme, null, null, 0, 8) == NOT_INITIALIZED and b"dsv_init" in L.dsv_last_error()
first = ctypes.c_uint32(77)
col = (_lib.Column * 2)()
assert L.dsv_keyset_append(None, p, p, sz(1), ctypes.byref(first)) == INVALID
assert L.dsv_keyset_append(None, p, p, sz(0), None) == INVALID
assert L.dsv_keyset_append_wire(None, p, sz(1), ctypes.byref(first)) == INVALID
assert L.dsv_keyset_append_mont_cols(None, col, sz(1), ctypes.byref(first)) == INVALID
assert b"null key set" in L.dsv_last_error()
cap = sz(55)
assert L.dsv_keyset_capacity(None, ctypes.byref(cap)) == INVALID
assert L.dsv_keyset_key_ok_n(None, p, sz(2), ctypes.byref(cap)) == INVALID
assert first.value == 77 and cap.value == 55
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- register budget (assembly cached like tests/test_isa_guard.py) ----------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_append_and_lookup_kernels_stay_in_registers():
    """k_index_append<AffineKey<NP>>: no scratch, no spilled VGPRs, no AGPRs, and no more than 44 (NP = 1) / 70
    (NP = 2) VGPRs, what the build kernel of a fresh set took at the commit before the append kernel existed
     and the append kernel, which now serves fresh sets too (first = 0), has kept to since: a fixed
    ceiling.  k_index_lookup<AffineKey<NP>> with the k guard: within the 42 - 68 VGPRs DESIGN.md §10.4 records for
    the kernel without it (one more scalar argument, one compare per slot)."""
    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    info = _kernel_info(_asm(os.path.join(CSRC, "k_keyed_lookup.hip"), _stamp()))

    def one(kernel, needle):
        hits = [k for k in info if kernel in k and needle in k]
        assert len(hits) == 1, (kernel, needle, sorted(info))
        return info[hits[0]]

    for np_ in (1, 2):
        append, lookup = (one(name, "AffineKeyILi%dE" % np_) for name in ("k_index_append", "k_index_lookup"))
        for k in (append, lookup):
            assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0 and k["agprs"] == 0, (np_, k)
        assert 42 <= append["vgprs"] <= {1: 44, 2: 70}[np_], (np_, append)
        assert 42 <= lookup["vgprs"] <= 68, (np_, lookup)
