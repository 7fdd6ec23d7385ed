"""The key cache for typed objects, CPU side (no GPU): the exports of the open-set verify over verify_batch's arguments
(dsv_verify_keyed_open_mont_*, include/dsv.h), the workspace formula against a restatement, the
calls before dsv_init, and the register budget of the front kernel k_normalize_lookup against the normalisation
kernel of as many points."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
NSIG = {"single": 1, "double": 2, "vargen": 1}  # nonce points per signature
NKEY = {"single": 1, "double": 2, "vargen": 2}  # key points per key
SYMBOLS = ("dsv_keyed_open_mont_workspace_bytes", "dsv_verify_keyed_open_mont_dev", "dsv_verify_keyed_open_mont_cols",
           "dsv_verify_keyed_open_mont_cols_submit")


def _up(x, a=256):
    return (x + a - 1) // a * a


def test_open_mont_symbols_are_exported_and_declared():
    from schnorr_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsv.h")).read()
    rust = open(os.path.join(ROOT, "rust", "dusk-schnorr-gpu", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
        assert name + "(" in header, name
        assert re.search(r"\bfn %s\(" % name, rust), name
    assert re.search(r"\bfn verify_batch_open\b", rust)
    hpp = open(os.path.join(ROOT, "include", "dusk_schnorr.hpp")).read()
    for name in ("verify_batch_open_bytes", "verify_batch_open", "verify_batch_open_submit"):
        assert re.search(r"\b%s\(" % name, hpp), name


def test_open_mont_workspace_formula():
    """index column | miss list | its length | the unkeyed kernel's window tables | one 64-byte column per key point
    | u | m | R [| R'] | valid | prefix products of all points | the keyed workspace; the index column first"""
    from schnorr_amd import _lib
    from schnorr_amd import engine as E

    sizes = (0, 1, 64, 65, 4099, 1 << 16, (1 << 20) + 1)
    for scheme in SCHEMES:
        ns, nk = NSIG[scheme], NKEY[scheme]
        last = -1
        for n in sizes:
            # the open-set form by affine bytes: index column + keyed workspace + miss list, length, window tables
            open_affine = E.keyed_open_workspace_bytes(n)
            assert open_affine >= _up(4 * n) + E.keyed_workspace_bytes(n)
            front = 2 * _up(32 * n) + ns * _up(64 * n) + _up(n) + _up((ns + nk) * (n + 32) * 36)
            want = open_affine + nk * _up(64 * n) + front
            got = E.keyed_open_mont_workspace_bytes(scheme, n)
            assert got == want, (scheme, n, got, want)
            assert got % 256 == 0 and got > last
            last = got
            # what the keyed typed form's front takes, with the key points' prefix products on top
            keyed_front = E.keyed_mont_workspace_bytes(scheme, n) - E.keyed_workspace_bytes(n)
            assert front - keyed_front == _up((ns + nk) * (n + 32) * 36) - _up(ns * (n + 32) * 36)
        vals = [E.keyed_open_mont_workspace_bytes(scheme, n) for n in range(0, 400)]
        assert all(a <= b for a, b in zip(vals, vals[1:]))
    L = _lib.load()
    for scheme in (-1, 3, 99):
        assert L.dsv_keyed_open_mont_workspace_bytes(ctypes.c_int(scheme), ctypes.c_size_t(5)) == 0
    with pytest.raises(ValueError):
        E.keyed_open_mont_workspace_bytes("triple", 1)


def test_open_mont_calls_before_init_are_not_initialized():
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
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
n, ws = ctypes.c_size_t(1), ctypes.c_size_t(1 << 22)
misses = ctypes.c_size_t(77)
cols = (_lib.Column * 6)()
for c in range(6):
    cols[c].base, cols[c].stride = b.ctypes.data, 96
assert L.dsv_verify_keyed_open_mont_cols(None, cols, n, p(ok), ctypes.byref(misses)) == -1
assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_verify_keyed_open_mont_dev(None, p(b), p(b), p(b), p(b), p(b), p(b), n, p(ok), p(b), ws, None, None) == -1
assert b"dsv_init" in L.dsv_last_error()
job = ctypes.c_void_p(1)
assert L.dsv_verify_keyed_open_mont_cols_submit(None, cols, n, p(ok), ctypes.byref(job)) == -1
assert b"dsv_init" in L.dsv_last_error() and job.value is None
assert L.dsv_verify_keyed_open_mont_cols(None, None, ctypes.c_size_t(0), None, None) == -1
assert misses.value == 77 and ok[0] == 7
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


# ---- register budget of k_keyed_open_mont.hip (assembly cached like tests/test_isa_guard.py) ---------------
# VGPRs, AGPRs, scratch bytes, occupancy of k_normalize_lookup<NPS, NPK>, as this build's gfx950 assembly states
# them (DESIGN.md §10.9 quotes the same figures)
BUDGET = {(1, 1): (131, 0, 0, 3), (2, 2): (131, 0, 0, 3), (1, 2): (131, 0, 0, 3)}


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_front_kernel_register_budget():
    """k_normalize_lookup<NPS, NPK> is k_normalize_uvz<NPS + NPK> with the key's row held in registers across a
    table walk: no more scratch than that kernel, compiled by this run; VGPRs, AGPRs, scratch and occupancy pinned
    as they come out."""
    from concurrent.futures import ThreadPoolExecutor

    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    stamp = _stamp()
    units = ("k_keyed_open_mont.hip", "k_misc.hip")
    with ThreadPoolExecutor(2) as ex:
        front, misc = [_kernel_info(s) for s in ex.map(lambda u: _asm(os.path.join(CSRC, u), stamp), units)]

    def one(info, *needles):
        hits = [k for k in info if all(n in k for n in needles)]
        assert len(hits) == 1, (needles, sorted(info))
        return info[hits[0]]

    for (nps, npk), (vgprs, agprs, scratch, occupancy) in BUDGET.items():
        k = one(front, "k_normalize_lookupILi%dELi%dE" % (nps, npk))
        r = one(misc, "k_normalize_uvzILi%dE" % (nps + npk))
        print("k_normalize_lookup<%d, %d>" % (nps, npk), k, "against k_normalize_uvz<%d>" % (nps + npk), r)
        assert k["scratch"] <= r["scratch"], (nps, npk, k, r)
        assert (k["vgprs"], k["agprs"], k["scratch"], k["occupancy"]) == (vgprs, agprs, scratch, occupancy), (nps, npk, k)
