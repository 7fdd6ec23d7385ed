"""Registered key sets, CPU side (no GPU): the size formula of dsv_keyset_bytes, creation before dsv_init,
a word-level model of the signed 8-bit recoding of k_verify_keyed (keyed.h: recode_key / next_key_digit),
and the register budget of k_keyed.hip's kernels (no scratch, at least two waves per SIMD)."""
import ctypes
import os
import subprocess
import sys

import pytest

import pymodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT_BYTES = 32 * 129 * 144  # 32 windows x 129 entries x 144 B
POINTS = {"single": 1, "double": 2, "vargen": 2}


def _layout_bytes(scheme, k):
    return POINTS[scheme] * k * POINT_BYTES + (k + 255) // 256 * 256


@pytest.mark.parametrize("scheme", sorted(POINTS))
def test_keyset_bytes_formula(scheme):
    from schnorr_amd import engine as E

    assert POINT_BYTES == 594432
    for k in (0, 1, 2, 37, 255, 256, 257, 1000, 16384):
        assert E.keyset_bytes(scheme, k) == _layout_bytes(scheme, k), (scheme, k)
    assert E.keyset_bytes(scheme, 0) == 0


def test_keyset_bytes_unknown_scheme_and_workspace():
    from schnorr_amd import _lib

    L = _lib.load()
    assert L.dsv_keyset_bytes(3, ctypes.c_size_t(5)) == 0 and L.dsv_keyset_bytes(-1, ctypes.c_size_t(5)) == 0
    for n in (0, 1, 255, 256, 1 << 20):
        assert L.dsv_keyed_workspace_bytes(ctypes.c_size_t(n)) >= 33 * n


def test_keyset_create_before_init_is_not_initialized():
    """In a process of its own: before any dsv_init, both constructors return DSV_ERR_NOT_INITIALIZED and
    leave the handle NULL."""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
pk = np.zeros((2, 64), np.uint8)
for scheme in (0, 1, 2):
    h = ctypes.c_void_p(1)
    rc = L.dsv_keyset_create(scheme, pk.ctypes.data_as(ctypes.c_void_p), pk.ctypes.data_as(ctypes.c_void_p),
                             ctypes.c_size_t(2), ctypes.byref(h))
    assert rc == -1 and h.value is None, (scheme, rc, h.value)
    h = ctypes.c_void_p(1)
    rc = L.dsv_keyset_create_wire(scheme, pk.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(2), ctypes.byref(h))
    assert rc == -1 and h.value is None, (scheme, rc, h.value)
assert b"dsv_init" in L.dsv_last_error()
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- the signed 8-bit recoding, word for word as keyed.h computes it --------------------------------------
def _words(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def recode_key(s):
    """y = s + 0x8080..80 over eight 32-bit words (the carry out of word 7 is dropped, as on the device)"""
    w = _words(s)
    y, carry = [], 0
    for i in range(8):
        t = w[i] + 0x80808080 + carry
        y.append(t & 0xFFFFFFFF)
        carry = t >> 32
    return y


def key_digits(s):
    y = recode_key(s)
    out = []
    for _ in range(32):
        out.append((y[0] & 0xFF) - 128)
        y = [((y[i] >> 8) | (y[i + 1] << 24)) & 0xFFFFFFFF for i in range(7)] + [y[7] >> 8]
    return out


CASES = [0, 1, 2, 127, 128, 255, 256, M.R_ORDER - 1, M.R_ORDER - 2, (1 << 250) - 1, (1 << 252) - 1,
         (1 << 253) - 1, 1 << 252, 0x7F * sum(1 << (8 * k) for k in range(31)),
         0x80 * sum(1 << (8 * k) for k in range(31)), 0xFF * sum(1 << (8 * k) for k in range(31)),
         sum(0x80 << (16 * k) for k in range(15)), sum(0x7F80 << (16 * k) for k in range(15)),
         int("7f" * 31 + "80", 16) & ((1 << 253) - 1), int("80" * 31 + "7f", 16) & ((1 << 253) - 1)]


@pytest.mark.parametrize("s", CASES, ids=[hex(c)[:18] for c in CASES])
def test_key_recoding_reassembles(s):
    assert s < 1 << 253
    d = key_digits(s)
    assert len(d) == 32 and all(-128 <= x <= 127 for x in d), d
    assert sum(x << (8 * k) for k, x in enumerate(d)) == s


def test_key_recoding_random_scalars():
    import random

    rng = random.Random(20261016)
    for bits in (250, 252, 253):
        for _ in range(2000):
            s = rng.getrandbits(bits)
            d = key_digits(s)
            assert all(-128 <= x <= 127 for x in d)
            assert sum(x << (8 * k) for k, x in enumerate(d)) == s


def test_key_recoding_needs_the_bound():
    """the model is exact only below 2^254: past that the carry out of the top word is lost"""
    s = (1 << 256) - 1
    assert sum(x << (8 * k) for k, x in enumerate(key_digits(s))) != s


# ---- register budget of k_keyed.hip (assembly cached like tests/test_isa_guard.py) ----------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_keyed_kernels_stay_in_registers():
    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    info = _kernel_info(_asm(os.path.join(CSRC, "k_keyed.hip"), _stamp()))
    names = {"k_build_key_tables": 1, "k_verify_keyedILi0E": 1, "k_verify_keyedILi1E": 1, "k_verify_keyedILi2E": 1}
    for needle in names:
        hits = [k for k in info if needle in k]
        assert len(hits) == 1, (needle, sorted(info))
        k = info[hits[0]]
        assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0, (needle, k)
        assert k["occupancy"] >= 2 and k["agprs"] == 0, (needle, k)
