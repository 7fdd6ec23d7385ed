"""Keys replaced in place, CPU side (no GPU): the new exports and their signatures in include/dsv.h, the calls before
dsv_init, the register budget of the commit and rebuild kernels of k_keyed_replace.hip, and the properties of the
Python model of the canonical index layout (tests/keyset_index_model.py) that the GPU tests compare against."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import keyset_index_model as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGNATURES = {
    "dsv_keyset_replace": "int dsv_keyset_replace(dsv_keyset *ks, const uint32_t *indices, const uint8_t *pk_uv, "
                          "const uint8_t *pk2_uv, size_t m);",
    "dsv_keyset_replace_wire": "int dsv_keyset_replace_wire(dsv_keyset *ks, const uint32_t *indices, "
                               "const uint8_t *pk_bytes, size_t m);",
    "dsv_debug_keyset_slots": "int dsv_debug_keyset_slots(const dsv_keyset *ks, int form, uint32_t *out, size_t room, "
                              "size_t *slots_out);",
}


def test_exports_and_declared_signatures():
    from schnorr_amd import _lib

    L = _lib.load()
    with open(os.path.join(ROOT, "include", "dsv.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    flat = " ".join(text.split()).replace(" ,", ",")
    for name, decl in SIGNATURES.items():
        assert name in _lib.SYMBOLS and getattr(L, name) is not None, name
        assert " ".join(decl.split()) in flat, name
    with open(os.path.join(ROOT, "rust", "dusk-schnorr-gpu", "src", "lib.rs")) as f:
        shim = f.read()
    for name in SIGNATURES:
        assert "pub fn %s(" % name in shim, name


def test_calls_before_init():
    """in a process of its own, before and without dsv_init: a NULL handle is an invalid argument to both replace
    calls, like the append calls, whatever the other arguments are; the slot introspection has no handle to be
    given yet and is told that nothing is up; nothing is written"""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
from schnorr_amd import _lib
L = _lib.load()
pk = np.zeros((2, 64), np.uint8)
idx = np.zeros(2, np.uint32)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
sz = ctypes.c_size_t
NOT_INITIALIZED, INVALID = -1, -2
assert L.dsv_keyset_replace(None, p(idx), p(pk), p(pk), sz(2)) == INVALID
assert b"null key set" in L.dsv_last_error()
assert L.dsv_keyset_replace(None, None, None, None, sz(0)) == INVALID
assert L.dsv_keyset_replace_wire(None, p(idx), p(pk), sz(2)) == INVALID
assert L.dsv_keyset_replace_wire(None, None, None, sz(0)) == INVALID
assert b"null key set" in L.dsv_last_error()
out = np.full(4, 7, np.uint32)
slots = sz(55)
for form in (0, 1, 2):
    assert L.dsv_debug_keyset_slots(None, form, p(out), sz(4), ctypes.byref(slots)) == NOT_INITIALIZED
    assert b"dsv_init" in L.dsv_last_error()
assert slots.value == 55 and (out == 7).all()
assert L.dsv_debug_keyset_replace_exclusive_ns() == 0
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_commit_and_rebuild_kernels_stay_in_registers():
    """k_keyed_replace.hip: the commit, the planar copy and the ordered insertion — for one- and two-point keys, and
    both key forms of the insertion — use no scratch memory, spill no VGPR and take no AGPR"""
    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    info = _kernel_info(_asm(os.path.join(CSRC, "k_keyed_replace.hip"), _stamp()))
    kernels = {name: k for name, k in info.items() if "vgprs" in k}
    for kernel, count in (("k_replace_commit", 2), ("k_rows_to_planar", 2), ("k_index_reinsert", 4)):
        hits = [name for name in kernels if kernel in name]
        assert len(hits) == count, (kernel, sorted(kernels))
        for name in hits:
            k = kernels[name]
            assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0 and k["agprs"] == 0, (name, k)
    assert len(kernels) == 8, sorted(kernels)
    # the two index kernels of k_keyed_lookup.hip stay where they are, one per key form
    assert not [name for name in kernels if "k_index_append" in name or "k_index_lookup" in name]


# ---- the model's own properties ---------------------------------------------------------------------------------
@pytest.mark.parametrize("form", IM.FORMS)
@pytest.mark.parametrize("scheme", ("single", "double", "vargen"))
def test_model_layout_is_ordered_and_has_one_entry_per_distinct_valid_key(scheme, form):
    """random keys (random bytes: the model only hashes and compares them), a third of them copies of others, a fifth
    invalid, in sets that are full (k = capacity) and half full: the layout has exactly one entry per distinct valid
    key, at the lowest index of its equals, every slot between a key's home and its place holds a lower index, and
    the layout does not depend on the order of insertion as long as that invariant is kept (inserting in reverse
    with displacement gives the same array)."""
    from schnorr_amd import engine as E

    rng = np.random.default_rng(20261020 + len(scheme) + len(form))
    two = scheme != "single"
    for capacity, k in ((8, 8), (40, 40), (40, 17), (200, 200)):
        P0 = rng.integers(0, 256, size=(k, 64), dtype=np.uint8)
        P1 = rng.integers(0, 256, size=(k, 64), dtype=np.uint8) if two else None
        for j in np.flatnonzero(rng.integers(0, 3, size=k) == 0):
            src = int(rng.integers(0, k))
            P0[j] = P0[src]
            if two:
                P1[j] = P1[src]
        key_ok = (rng.integers(0, 5, size=k) != 0).astype(np.uint8)
        cap = IM.cap_of(capacity)
        homes = [IM.home_slot(E, scheme, capacity, form, P0[j], P1[j] if two else None) for j in range(k)]
        slots = IM.canonical_slots(E, scheme, P0, P1, key_ok, capacity, form, homes=homes)
        assert slots.shape == (cap,) and cap >= 2 * capacity
        row = lambda j: bytes(P0[j]) + (bytes(P1[j]) if two else b"")
        lowest = {}
        for j in range(k):
            if key_ok[j]:
                lowest.setdefault(row(j), j)
        occupants = sorted(int(x) for x in slots if x != IM.NONE)
        assert occupants == sorted(lowest.values())
        IM.check_ordered(slots, {j: homes[j] for j in occupants})
        # a key is found by a walk from its home that stops at the first empty slot, also by a reader that takes
        # every occupant >= k' for empty, for every k'
        for kk in (k, k // 2, 1):
            for j in occupants:
                s, found = homes[j], IM.NONE
                while slots[s] != IM.NONE and slots[s] < kk:
                    if slots[s] == j:
                        found = j
                        break
                    s = (s + 1) % cap
                assert (found == j) == (j < kk), (kk, j)
        # ordered insertion in the reverse order: the same array
        other = np.full(cap, IM.NONE, dtype=np.uint32)
        for j in reversed(occupants):
            carried, s = j, homes[j]
            while True:
                old = int(other[s])
                other[s] = min(old, carried)
                if old == IM.NONE:
                    break
                carried = max(old, carried)
                s = (s + 1) % cap
        assert (other == slots).all()
