"""The var-generator scheme's open-set verify by key value, CPU side (no GPU): the exports
(dsv_verify_vargen_keyed_open*, include/dsv.h), the calls before dsv_init, and the register budget of
k_verify_var_listed (k_keyed_open_var.hip) against the kernel it mirrors, k_verify_var (k_vargen.hip)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARGEN_OPEN_SYMBOLS = ("dsv_verify_vargen_keyed_open_dev", "dsv_verify_vargen_keyed_open")


def test_vargen_open_symbols_are_exported_and_declared():
    from schnorr_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "dsv.h")).read()
    for name in VARGEN_OPEN_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert getattr(L, name) is not None
        assert name + "(" in header, name


def test_vargen_open_calls_before_init_are_not_initialized():
    """In a process of its own: before any dsv_init both calls return DSV_ERR_NOT_INITIALIZED for the NULL handle
    that is all a caller can have then, and touch neither ok nor misses."""
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
assert L.dsv_verify_vargen_keyed_open(None, p(b), p(b), p(b), p(b), p(b), n, p(ok), ctypes.byref(misses)) == -1
assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_verify_vargen_keyed_open_dev(None, p(b), p(b), p(b), p(b), p(b), n, p(ok), p(b), ws, None, None) == -1
assert b"dsv_init" in L.dsv_last_error()
assert L.dsv_verify_vargen_keyed_open(None, None, None, None, None, None, ctypes.c_size_t(0), None, None) == -1
assert misses.value == 77 and ok[0] == 7
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_vargen_listed_kernel_register_budget():
    """k_verify_var_listed sits on the budget of the kernel it mirrors — at most 256 VGPRs, two waves per SIMD, no
    AGPRs — and the indirection through the list costs it no scratch: no more scratch bytes and no more spilled
    VGPRs than k_verify_var, compiled by this run (the bound is the mirrored kernel's figure, not a fixed one)."""
    from concurrent.futures import ThreadPoolExecutor

    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    stamp = _stamp()
    with ThreadPoolExecutor(2) as ex:
        listed_s, var_s = ex.map(lambda u: _asm(os.path.join(CSRC, u), stamp), ("k_keyed_open_var.hip", "k_vargen.hip"))
    listed, var = _kernel_info(listed_s), _kernel_info(var_s)

    def one(info, needle):
        hits = [k for k in info if needle in k]
        assert len(hits) == 1, (needle, sorted(info))
        return info[hits[0]]

    k = one(listed, "19k_verify_var_listedE")
    ref = one(var, "12k_verify_varE")
    print("k_verify_var_listed", k, "k_verify_var", ref)
    assert k["occupancy"] == 2 and k["agprs"] == 0 and k["vgprs"] <= 256, k
    assert k["scratch"] <= ref["scratch"], (k, ref)
    assert k["vgpr_spill_count"] <= ref["vgpr_spill_count"], (k, ref)
