"""Key sets by key value, CPU side (no GPU): the size formulas of dsv_keyset_index_bytes and
dsv_keyed_lookup_workspace_bytes, the home slot of dsv_debug_keyset_home_slot against a Python model of the hash
(include/dsv.h), the by-value calls before dsv_init, and the register budget of k_keyed_lookup.hip's kernels."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from abi_model import POINTS, _up, cap_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODE = {"single": 0, "double": 1, "vargen": 2}
M32 = 0xFFFFFFFF


def model_hash(key_bytes):
    """h of include/dsv.h over the 32-bit little-endian words of key_a (then key_b)"""
    h = 0
    for w in np.frombuffer(bytes(key_bytes), dtype="<u4").tolist():
        h = ((h ^ w) * 0x9E3779B1) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


@pytest.mark.parametrize("scheme", sorted(POINTS))
def test_index_bytes_formula(scheme):
    from schnorr_amd import engine as E

    for k in (0, 1, 31, 32, 33, 1000, 16384):
        want = _up(POINTS[scheme] * 64 * k) + _up(4 * cap_of(k)) if k else 0
        assert E.keyset_index_bytes(scheme, k) == want, (scheme, k)
    assert cap_of(31) == 64 and cap_of(32) == 64 and cap_of(33) == 128 and cap_of(16384) == 32768


def test_index_bytes_unknown_scheme():
    from schnorr_amd import _lib

    L = _lib.load()
    for k in (0, 1, 1000):
        assert L.dsv_keyset_index_bytes(3, ctypes.c_size_t(k)) == 0
        assert L.dsv_keyset_index_bytes(-1, ctypes.c_size_t(k)) == 0


def test_lookup_workspace_formula():
    from schnorr_amd import engine as E

    for n in (0, 1, 255, 256, 1 << 20):
        assert E.keyed_lookup_workspace_bytes(n) == _up(4 * n) + E.keyed_workspace_bytes(n), n
        assert E.keyed_workspace_bytes(n) == _up(32 * n) + _up(n), n


@pytest.mark.parametrize("scheme", sorted(POINTS))
def test_home_slot_matches_the_model(scheme):
    from schnorr_amd import engine as E

    rng = np.random.default_rng(20261018 + CODE[scheme])
    np_ = POINTS[scheme]
    for k in (1, 24, 1500):
        cap = cap_of(k)
        assert cap == {1: 64, 24: 64, 1500: 4096}[k]
        for _ in range(200):
            key = rng.integers(0, 256, size=64 * np_, dtype=np.uint8)
            a, b = key[:64], (key[64:] if np_ == 2 else None)
            got = E.keyset_home_slot(scheme, k, a, b)
            assert got < cap
            assert got == model_hash(key) & (cap - 1), (scheme, k, key.tobytes().hex())


def test_home_slot_sees_the_last_byte():
    """at k = 2^31 the capacity is 2^32 and the home slot is the whole of h: a one-bit flip in the last byte of
    key_b (key_a for a one-point key) changes it — every step of the hash is a bijection of h"""
    from schnorr_amd import engine as E

    rng = np.random.default_rng(7)
    k = 1 << 31
    for scheme in sorted(POINTS):
        for _ in range(50):
            key = rng.integers(0, 256, size=64 * POINTS[scheme], dtype=np.uint8)
            flipped = key.copy()
            flipped[-1] ^= 1 << int(rng.integers(0, 8))
            split = lambda x: (x[:64], x[64:] if POINTS[scheme] == 2 else None)
            h0, h1 = E.keyset_home_slot(scheme, k, *split(key)), E.keyset_home_slot(scheme, k, *split(flipped))
            assert h0 == model_hash(key) and h1 == model_hash(flipped)
            assert h0 != h1


def test_home_slot_bad_arguments():
    from schnorr_amd import _lib

    L = _lib.load()
    key = np.zeros(64, np.uint8)
    p = ctypes.c_void_p(key.ctypes.data)
    none = (1 << 64) - 1
    assert L.dsv_debug_keyset_home_slot(3, ctypes.c_size_t(5), p, p) == none
    assert L.dsv_debug_keyset_home_slot(0, ctypes.c_size_t(0), p, None) == none
    assert L.dsv_debug_keyset_home_slot(1, ctypes.c_size_t(5), p, None) == none
    assert L.dsv_debug_keyset_home_slot(0, ctypes.c_size_t(5), p, None) < 64


def test_by_value_calls_before_init_are_not_initialized():
    """In a process of its own: before any dsv_init, both lookups and both verifies return
    DSV_ERR_NOT_INITIALIZED (there is no handle to give them yet: NULL)."""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
b = np.zeros((1, 64), np.uint8)
idx = np.zeros(1, np.uint32)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
n, ws = ctypes.c_size_t(1), ctypes.c_size_t(1 << 12)
misses = ctypes.c_size_t(77)
assert L.dsv_keyset_lookup(None, p(b), p(b), n, p(idx), ctypes.byref(misses)) == -1
assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_keyset_lookup_dev(None, p(b), p(b), n, p(idx), None, None) == -1
assert L.dsv_verify_keyed_lookup(None, p(b), p(b), p(b), p(b), p(b), p(b), n, p(b), ctypes.byref(misses)) == -1
assert L.dsv_verify_keyed_lookup_dev(None, p(b), p(b), p(b), p(b), p(b), p(b), n, p(b), p(b), ws, None, None) == -1
assert b"dsv_init" in L.dsv_last_error()
out = (ctypes.c_uint64 * 4)()
assert L.dsv_debug_keyset_index_stats(None, out) == -1
assert misses.value == 77 and idx[0] == 0
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- register budget of k_keyed_lookup.hip (assembly cached like tests/test_isa_guard.py) ----------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_lookup_kernels_stay_in_registers():
    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    info = _kernel_info(_asm(os.path.join(CSRC, "k_keyed_lookup.hip"), _stamp()))
    # the affine instantiations of the two index kernels (the fresh set's build is the append kernel at first = 0)
    for kernel in ("k_index_append", "k_index_lookup"):
        for np_ in (1, 2):
            needle = "AffineKeyILi%dE" % np_
            hits = [k for k in info if kernel in k and needle in k]
            assert len(hits) == 1, (kernel, needle, sorted(info))
            k = info[hits[0]]
            assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0, (kernel, needle, k)
