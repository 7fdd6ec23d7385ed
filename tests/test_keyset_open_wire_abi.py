"""The key cache for serialized records, CPU side (no GPU): the exports of the wire index and of the open-set verify
by compressed key (dsv_keyset_lookup_wire*, dsv_verify_*_keyed_open_wire*, include/dsv.h), the size formulas, the
calls before dsv_init, the home slot of a record against a Python KeyHash, and the register budget of
the record kernels against the kernels they mirror."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
POINTS = {"single": 1, "double": 2, "vargen": 2}  # key points per key
WIRE_SYMBOLS = (
    "dsv_keyset_wire_index_bytes", "dsv_keyset_lookup_wire_dev", "dsv_keyset_lookup_wire",
    "dsv_debug_keyset_wire_home_slot", "dsv_keyed_open_wire_workspace_bytes",
    "dsv_verify_single_keyed_open_wire_dev", "dsv_verify_double_keyed_open_wire_dev",
    "dsv_verify_vargen_keyed_open_wire_dev", "dsv_verify_single_keyed_open_wire",
    "dsv_verify_double_keyed_open_wire", "dsv_verify_vargen_keyed_open_wire")


def _up(x, a=256):
    return (x + a - 1) // a * a


def _cap(k):
    cap = 64
    while cap < 2 * k:
        cap <<= 1
    return cap


def test_wire_symbols_are_exported_and_declared():
    from schnorr_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsv.h")).read()
    rust = open(os.path.join(ROOT, "rust", "dusk-schnorr-gpu", "src", "lib.rs")).read()
    for name in WIRE_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
        assert name + "(" in header, name
        assert re.search(r"\bfn %s\(" % name, rust), name


def test_wire_index_bytes_formula():
    from schnorr_amd import _lib
    from schnorr_amd import engine as E

    for scheme in SCHEMES:
        assert E.keyset_wire_index_bytes(scheme, 0) == 0
        last = 0
        for k in (1, 2, 8, 32, 33, 64, 1000, 1 << 16, (1 << 20) + 1):
            want = _up(32 * POINTS[scheme] * k) + _up(4 * _cap(k))
            got = E.keyset_wire_index_bytes(scheme, k)
            assert got == want, (scheme, k, got, want)
            assert got >= last
            last = got
            # the slots are those of the affine index; its key bytes are twice the records
            assert E.keyset_index_bytes(scheme, k) - got == _up(64 * POINTS[scheme] * k) - _up(32 * POINTS[scheme] * k)
    L = _lib.load()
    for scheme in (-1, 3, 99):
        assert L.dsv_keyset_wire_index_bytes(ctypes.c_int(scheme), ctypes.c_size_t(5)) == 0
        assert L.dsv_keyed_open_wire_workspace_bytes(ctypes.c_int(scheme), ctypes.c_size_t(5)) == 0
    with pytest.raises(ValueError):
        E.keyset_wire_index_bytes("triple", 1)
    with pytest.raises(ValueError):
        E.keyed_open_wire_workspace_bytes("triple", 1)


def test_open_wire_workspace_formula():
    """the decoded signature columns of the keyed wire form + one 64-byte column per key point + everything the
    open-set form by affine bytes needs"""
    from schnorr_amd import engine as E

    sizes = (0, 1, 64, 65, 4099, 1 << 16, (1 << 20) + 1)
    for scheme in SCHEMES:
        last = -1
        for n in sizes:
            wire_cols = E.keyed_wire_workspace_bytes(scheme, n) - E.keyed_workspace_bytes(n)
            want = wire_cols + POINTS[scheme] * _up(64 * n) + E.keyed_open_workspace_bytes(n)
            got = E.keyed_open_wire_workspace_bytes(scheme, n)
            assert got == want, (scheme, n, got, want)
            assert got % 256 == 0 and got > last
            last = got
        vals = [E.keyed_open_wire_workspace_bytes(scheme, n) for n in range(0, 400)]
        assert all(a <= b for a, b in zip(vals, vals[1:]))


def test_wire_calls_before_init_are_not_initialized():
    """In a process of its own: before any dsv_init every new call that takes a handle returns
    DSV_ERR_NOT_INITIALIZED for the NULL handle that is all a caller can have then, and touches nothing."""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
b = np.zeros((1, 96), np.uint8)
ok = np.full(1, 7, np.uint8)
idx = np.full(1, 0x5A5A5A5A, np.uint32)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
n, ws = ctypes.c_size_t(1), ctypes.c_size_t(1 << 22)
misses = ctypes.c_size_t(77)
for scheme in ("single", "double", "vargen"):
    host = getattr(L, "dsv_verify_%%s_keyed_open_wire" %% scheme)
    dev = getattr(L, "dsv_verify_%%s_keyed_open_wire_dev" %% scheme)
    assert host(None, p(b), p(b), p(b), n, p(ok), ctypes.byref(misses)) == -1
    assert b"dsv_init" in L.dsv_last_error()
    assert dev(None, p(b), p(b), p(b), n, p(ok), p(b), ws, None, None) == -1
    assert b"dsv_init" in L.dsv_last_error()
    assert host(None, None, None, None, ctypes.c_size_t(0), None, None) == -1
assert L.dsv_keyset_lookup_wire(None, p(b), n, p(idx), ctypes.byref(misses)) == -1
assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_keyset_lookup_wire_dev(None, p(b), n, p(idx), None, None) == -1
assert b"dsv_init" in L.dsv_last_error()
assert misses.value == 77 and ok[0] == 7 and idx[0] == 0x5A5A5A5A
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def _key_hash(words):
    """KeyHash (keyed_lookup.h) over 32-bit words"""
    m32 = 0xFFFFFFFF
    h = 0
    for w in words:
        h = ((h ^ int(w)) * 0x9E3779B1) & m32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & m32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & m32
    h ^= h >> 16
    return h


def test_wire_home_slot_is_keyhash_of_the_record_words():
    from schnorr_amd import _lib
    from schnorr_amd import engine as E

    rng = np.random.default_rng(20261019)
    for scheme in SCHEMES:
        width = 32 * POINTS[scheme]
        recs = rng.integers(0, 256, size=(40, width), dtype=np.uint8)
        recs[0] = 0
        recs[1] = 0xFF
        for capacity in (1, 32, 33, 1000):
            for rec in recs:
                want = _key_hash(rec.view("<u4")) & (_cap(capacity) - 1)
                assert E.keyset_wire_home_slot(scheme, capacity, rec) == want, (scheme, capacity)
    L = _lib.load()
    slot = ctypes.c_uint64(99)
    rec = np.zeros(64, np.uint8)
    p = rec.ctypes.data_as(ctypes.c_void_p)
    assert L.dsv_debug_keyset_wire_home_slot(ctypes.c_int(7), ctypes.c_size_t(4), p, ctypes.byref(slot)) == -2
    assert L.dsv_debug_keyset_wire_home_slot(ctypes.c_int(0), ctypes.c_size_t(0), p, ctypes.byref(slot)) == -2
    assert L.dsv_debug_keyset_wire_home_slot(ctypes.c_int(0), ctypes.c_size_t(4), None, ctypes.byref(slot)) == -2
    assert L.dsv_debug_keyset_wire_home_slot(ctypes.c_int(0), ctypes.c_size_t(4), p, None) == -2
    assert slot.value == 99


# ---- register budget of k_keyed_open_wire.hip (assembly cached like tests/test_isa_guard.py) -------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_wire_kernels_register_budget():
    """VGPRs, scratch and occupancy only.  The record instantiations of the index kernels move half the bytes of
    the affine ones: no scratch, no AGPRs, no more VGPRs and no less occupancy than the affine instantiation of the
    same key-point count, compiled by this run from the same unit.  k_decompress_listed is k_keyed_wire_decode's
    arithmetic behind one more indirection: no more VGPRs and no more scratch than the decode kernel with as many
    points per item."""
    from concurrent.futures import ThreadPoolExecutor

    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    stamp = _stamp()
    units = ("k_keyed_open_wire.hip", "k_keyed_lookup.hip", "k_keyed_wire.hip")
    with ThreadPoolExecutor(3) as ex:
        wire, lookup, decode = [_kernel_info(s) for s in ex.map(lambda u: _asm(os.path.join(CSRC, u), stamp), units)]

    def one(info, *needles):
        hits = [k for k in info if all(n in k for n in needles)]
        assert len(hits) == 1, (needles, sorted(info))
        return info[hits[0]]

    for np_ in (1, 2):
        for kernel in ("k_index_append", "k_index_lookup"):
            k, r = one(lookup, kernel, "RecordKeyILi%dE" % np_), one(lookup, kernel, "AffineKeyILi%dE" % np_)
            print(kernel, "records", np_, k, "against affine", r)
            assert k["scratch"] == 0 and k["agprs"] == 0, (kernel, np_, k)
            assert k["vgprs"] <= r["vgprs"], (kernel, np_, k, r)
            assert k["occupancy"] >= r["occupancy"], (kernel, np_, k, r)
        # points per item: k_keyed_wire_decode<0> (single) decodes one, <1> (double) two in adjacent lanes
        k, r = one(wire, "k_decompress_listedILi%dE" % np_), one(decode, "k_keyed_wire_decodeILi%dE" % (np_ - 1))
        print("k_decompress_listed<%d>" % np_, k, "against k_keyed_wire_decode<%d>" % (np_ - 1), r)
        assert k["vgprs"] <= r["vgprs"], (np_, k, r)
        assert k["scratch"] <= r["scratch"], (np_, k, r)
        assert k["occupancy"] >= r["occupancy"], (np_, k, r)
