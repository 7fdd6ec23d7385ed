"""The keyed typed-object form, CPU side (no GPU): the size formula of dsv_keyed_mont_workspace_bytes, the entry
points before dsv_init, and where the form's code lives (a unit and a header of its own, outside everything the
profiled kernels include; no kernel of its own, so there is no register budget to pin)."""
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
    """u, m, R[, R'], valid, the normalisation's prefix products (points * (n + 32) * 36 B), then
    dsv_keyed_workspace_bytes(n); each part rounded up to 256 B"""
    from schnorr_amd import engine as E

    p = NONCE_POINTS[scheme]
    return 2 * _up(32 * n) + p * _up(64 * n) + _up(n) + _up(p * (n + 32) * 36) + E.keyed_workspace_bytes(n)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_workspace_bytes_formula(scheme):
    from schnorr_amd import engine as E

    sizes = sorted(set(list(range(0, 300)) + [1 << b for b in range(9, 23)] + [(1 << b) + 1 for b in range(9, 23)] +
                       [(1 << b) - 1 for b in range(9, 23)] + [4099, 65539, 1000003]))
    assert len(sizes) > 300
    prev = 0
    for n in sizes:
        got = E.keyed_mont_workspace_bytes(scheme, n)
        assert got == _documented(scheme, n), (scheme, n)
        assert got >= prev, (scheme, n)
        assert got % 256 == 0
        prev = got


def test_workspace_bytes_unknown_scheme_and_order():
    from schnorr_amd import _lib, engine as E

    L = _lib.load()
    for bad in (-1, 3, 7):
        assert L.dsv_keyed_mont_workspace_bytes(bad, ctypes.c_size_t(1000)) == 0
    with pytest.raises(ValueError):
        E.keyed_mont_workspace_bytes("triple", 5)
    for n in (1, 255, 256, 257, 4099, 1 << 20):
        s, d, v = (E.keyed_mont_workspace_bytes(x, n) for x in SCHEMES)
        assert v == s
        # the second nonce point: its affine column, and its share of the prefix products
        assert d - s == _up(64 * n) + _up(2 * (n + 32) * 36) - _up((n + 32) * 36), n


def test_entry_points_before_init():
    """In a process of its own: before any dsv_init the workspace function answers, every verify entry point
    returns DSV_ERR_INVALID_ARGUMENT for a NULL key set and leaves `ok` alone, and the constructor reports that
    nothing is initialised."""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
# n = 1, single: u 256 + m 256 + R 256 + valid 256 + prefix up(33 * 36) = 1280, keyed workspace 512
assert L.dsv_keyed_mont_workspace_bytes(0, ctypes.c_size_t(1)) == 4 * 256 + 1280 + 512
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
u = np.zeros((2, 32), np.uint8); R = np.zeros((2, 96), np.uint8); idx = np.zeros(2, np.uint32)
ok = np.full(2, 7, np.uint8)
cols = (_lib.Column * 5)()
for k, a in enumerate((u, R, R, idx, u)):
    cols[k].base, cols[k].stride = a.ctypes.data, a.strides[0]
for n in (2, 0):
    assert L.dsv_verify_keyed_mont_cols(None, cols, ctypes.c_size_t(n), p(ok)) == -2
    assert b"null key set" in L.dsv_last_error()
    job = ctypes.c_void_p(1)
    assert L.dsv_verify_keyed_mont_cols_submit(None, cols, ctypes.c_size_t(n), p(ok), ctypes.byref(job)) == -2
    assert b"null key set" in L.dsv_last_error() and job.value is None
    assert L.dsv_verify_keyed_mont_dev(None, p(u), p(R), p(R), p(idx), p(u), ctypes.c_size_t(n), p(ok), p(ok),
                                       ctypes.c_size_t(1 << 20), None) == -2
    assert b"null key set" in L.dsv_last_error()
assert L.dsv_verify_keyed_mont_cols_submit(None, cols, ctypes.c_size_t(2), p(ok), None) == -2
assert (ok == 7).all()
pts = ctypes.byref(cols, ctypes.sizeof(_lib.Column))  # R, R: two 96-byte columns
# a key set cannot exist before dsv_init: the constructor says so
for scheme in (0, 1, 2):
    h = ctypes.c_void_p(1)
    assert L.dsv_keyset_create_mont_cols(scheme, pts, ctypes.c_size_t(2), ctypes.byref(h)) == -1
    assert h.value is None
# ... after its argument checks
h = ctypes.c_void_p(1)
assert L.dsv_keyset_create_mont_cols(3, pts, ctypes.c_size_t(2), ctypes.byref(h)) == -2 and h.value is None
assert L.dsv_keyset_create_mont_cols(0, cols, ctypes.c_size_t(2), ctypes.byref(h)) == -2  # u: stride 32 < 96
assert b"column 0" in L.dsv_last_error()
assert L.dsv_keyset_create_mont_cols(0, pts, ctypes.c_size_t(2), None) == -2
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_unit_and_header_are_outside_the_profiled_headers():
    """profiles/pmc_latest.json carries hashes of everything k_verify.hip and k_hash.hip include: the keyed typed
    form lives in a unit and a header of its own and adds no kernel"""
    import re

    from schnorr_amd import build as B

    assert "dsv_keyed_mont.hip" in B.UNITS
    own = open(os.path.join(B.CSRC, "keyed_mont.h")).read()
    assert "normalize_keyed_mont" in own and "verify_keyed_mont_cols_locked" in own
    unit = open(os.path.join(B.CSRC, "dsv_keyed_mont.hip")).read()
    assert "__global__" not in unit and "__global__" not in own
    assert len(re.findall(r"launch_normalize_uvz\(", unit)) == 2  # the verify paths' one call, the constructor's
    for u in ("k_verify.hip", "k_hash.hip"):
        seen = set()
        B._includes(os.path.join(B.CSRC, u), seen)
        names = {os.path.basename(p) for p in seen}
        assert not names & {"keyed_mont.h", "keyset_host.h", "dsv_host.h"}, (u, names)
        for p in seen:
            assert "keyed_mont" not in open(p, errors="replace").read(), p


def test_python_surface():
    from schnorr_amd import _lib, engine as E

    for name in ("dsv_keyset_create_mont_cols", "dsv_keyed_mont_workspace_bytes", "dsv_verify_keyed_mont_dev",
                 "dsv_verify_keyed_mont_cols", "dsv_verify_keyed_mont_cols_submit"):
        assert name in _lib.SYMBOLS
        assert hasattr(_lib.load(), name)
    for name in ("from_mont_cols", "verify_mont_dev", "verify_mont_cols", "submit_mont_cols"):
        assert callable(getattr(E.KeySet, name))
    assert issubclass(E.KeyedMontColsJob, E.MontColsJob)
