"""The keyed wire form, CPU side (no GPU): the size formula of dsv_keyed_wire_workspace_bytes, the entry
points before dsv_init, and the register budget of the decode kernel (k_keyed_wire.hip: no scratch, no
spills, no AGPRs, at least k_decompress's two waves per SIMD)."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
NONCE_POINTS = {"single": 1, "double": 2, "vargen": 1}


def _up(x):
    return (x + 255) // 256 * 256


def _documented(scheme, n):
    """u, R[, R'], the decode flags, then dsv_keyed_workspace_bytes(n); each part rounded up to 256 B"""
    from schnorr_amd import engine as E

    return _up(32 * n) + NONCE_POINTS[scheme] * _up(64 * n) + _up(n) + E.keyed_workspace_bytes(n)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_workspace_bytes_formula(scheme):
    from schnorr_amd import engine as E

    sizes = sorted(set(list(range(0, 300)) + [1 << b for b in range(9, 23)] + [(1 << b) + 1 for b in range(9, 23)] +
                       [(1 << b) - 1 for b in range(9, 23)] + [4099, 65539, 1000003]))
    assert len(sizes) > 300
    prev = 0
    for n in sizes:
        got = E.keyed_wire_workspace_bytes(scheme, n)
        assert got == _documented(scheme, n), (scheme, n)
        assert got >= prev, (scheme, n)
        assert got >= (32 + 64 * NONCE_POINTS[scheme] + 1 + 33) * n
        assert got % 256 == 0
        prev = got
    assert E.keyed_wire_workspace_bytes(scheme, 0) == 0


def test_workspace_bytes_unknown_scheme_and_order():
    from schnorr_amd import _lib, engine as E

    L = _lib.load()
    for bad in (-1, 3, 7):
        assert L.dsv_keyed_wire_workspace_bytes(bad, ctypes.c_size_t(1000)) == 0
    with pytest.raises(ValueError):
        E.keyed_wire_workspace_bytes("triple", 5)
    for n in (1, 255, 256, 257, 4099, 1 << 20):
        s, d, v = (E.keyed_wire_workspace_bytes(x, n) for x in SCHEMES)
        assert d >= s and v == s and d - s == _up(64 * n)


def test_entry_points_before_init():
    """In a process of its own: before any dsv_init the workspace function answers, and every entry point
    returns DSV_ERR_INVALID_ARGUMENT for a NULL key set without touching a device."""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
assert L.dsv_keyed_wire_workspace_bytes(0, ctypes.c_size_t(1)) == 256 * 5
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
m = np.zeros((2, 32), np.uint8); idx = np.zeros(2, np.uint32); ok = np.full(2, 7, np.uint8)
for scheme, w in (("single", 64), ("double", 96), ("vargen", 64)):
    sig = np.zeros((2, w), np.uint8)
    host = getattr(L, "dsv_verify_%%s_keyed_wire" %% scheme)
    dev = getattr(L, "dsv_verify_%%s_keyed_wire_dev" %% scheme)
    assert host(None, p(sig), p(idx), p(m), ctypes.c_size_t(2), p(ok)) == -2, scheme
    assert b"null key set" in L.dsv_last_error()
    assert host(None, p(sig), p(idx), p(m), ctypes.c_size_t(0), p(ok)) == -2, scheme
    assert dev(None, p(sig), p(idx), p(m), ctypes.c_size_t(2), p(ok), p(ok), ctypes.c_size_t(1 << 20), None) == -2, scheme
    assert (ok == 7).all()
# a key set cannot exist before dsv_init: its constructors say so
h = ctypes.c_void_p(1)
assert L.dsv_keyset_create_wire(0, p(m), ctypes.c_size_t(2), ctypes.byref(h)) == -1 and h.value is None
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_decode_kernel_stays_in_registers():
    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    info = _kernel_info(_asm(os.path.join(CSRC, "k_keyed_wire.hip"), _stamp()))
    kernels = sorted(k for k in info if "k_keyed_wire_decode" in k)
    for scheme in (0, 1, 2):
        hits = [k for k in kernels if "k_keyed_wire_decodeILi%dE" % scheme in k]
        assert len(hits) == 1, (scheme, sorted(info))
    assert len(kernels) == 3, kernels
    for name in kernels:
        k = info[name]
        assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
        assert k["agprs"] == 0 and k["occupancy"] >= 2, (name, k)


def test_launcher_is_declared_outside_the_profiled_headers():
    """profiles/pmc_latest.json carries hashes of everything k_verify.hip and k_hash.hip include: the keyed
    wire form's declarations live in headers of their own"""
    from schnorr_amd import build as B

    own = open(os.path.join(B.CSRC, "keyed_wire.h")).read()
    assert "launch_keyed_wire_decode" in own
    assert "k_keyed_wire.hip" in B.UNITS and "dsv_keyed_wire.hip" in B.UNITS
    for unit in ("k_verify.hip", "k_hash.hip"):
        seen = set()
        B._includes(os.path.join(B.CSRC, unit), seen)
        names = {os.path.basename(p) for p in seen}
        assert not names & {"keyed_wire.h", "keyed.h", "keyset_host.h"}, (unit, names)
        for p in seen:
            assert "keyed_wire" not in open(p, errors="replace").read(), p
