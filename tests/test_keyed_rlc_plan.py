"""The keyed fast accept (dsv_verify_*_keyed_rlc_dev, schnorr_amd/csrc/keyed_rlc.h), CPU side: the new symbols,
the geometry of the keyed plan (dsv_keyed_rlc_plan_info needs no GPU) against the unkeyed one, the workspace
size, argument checks, a Python model of the per-key aggregation, and the register budget of k_keyed_rlc.hip."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import pymodel as M
from schnorr_amd import _lib, engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
SIZES = [1, 2, 63, 64, 65, 1000, 4095, 4096, (1 << 14) - 1, 1 << 14, (1 << 17) - 1, 1 << 17, (1 << 19) - 1, 1 << 19,
         (1 << 20) + 12345, 1 << 22]
NEW = ("dsv_keyed_rlc_workspace_bytes", "dsv_keyed_rlc_plan_info", "dsv_debug_keyed_rlc_history",
       "dsv_verify_single_keyed_rlc_dev", "dsv_verify_double_keyed_rlc_dev", "dsv_verify_vargen_keyed_rlc_dev")


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "dsv.h")).read()
    L = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert getattr(L, name) is not None


@pytest.mark.parametrize("scheme", SCHEMES)
def test_keyed_plan_invariants(scheme):
    spts, fixed = {"single": (1, 1), "double": (2, 2), "vargen": (1, 0)}[scheme]
    for n in SIZES:
        for bits in (0, 4, 6, 8, 12, 14, 16):
            p = E.keyed_rlc_plan_info(scheme, n, 64, bits)
            q = E.rlc_plan_info(scheme, n, bits)
            c = p["c"]
            assert c == q["c"] and (bits == 0 or c == bits)
            # no key windows, not empty ones: only the nonce points have digit rows
            assert p["wpk"] == 0 and p["lpts"] == 0
            assert (p["spts"], p["fixed"]) == (spts, fixed)
            assert p["wr"] == q["wr"] and p["windows"] == p["wr"]
            assert p["rows"] == p["wr"] * spts
            assert p["buckets"] == p["windows"] << c and p["bins"] == p["windows"] << p["coarse_bits"]
            assert (p["fine_bits"], p["coarse_bits"], p["nseg"], p["nseg2"]) == \
                (q["fine_bits"], q["coarse_bits"], q["nseg"], q["nseg2"])
            assert (p["groups"], p["sub"], p["row_stride"]) == (q["groups"], q["sub"], q["row_stride"])
            assert p["entries"] == p["sub"] * p["rows"]
            # a window holds spts x sub entries at most; its bins take them all, or mean + 8 sigma
            most = spts * p["sub"]
            assert p["bin_cap"] % 64 == 0 and p["bin_cap"] <= max(64, (most + 63) // 64 * 64)
            if p["coarse_bits"] == 0:
                assert p["bin_cap"] >= most
            else:
                assert p["bin_cap"] >= (most >> p["coarse_bits"]) + 8 * int((most >> p["coarse_bits"]) ** 0.5)
            side = 1 << p["half"]
            lanes = p["windows"] * c
            assert p["tmp0"] >= max(p["windows"] * 2 * side * p["nseg"], lanes + 1)
            assert p["bytes"] % 256 == 0 or p["bytes"] > 0


@pytest.mark.parametrize("scheme", SCHEMES)
def test_keyed_sub_group_plans(scheme):
    for n in (1000, (1 << 17) + 5, (1 << 20) + 12345):
        for g in (2, 3, 16):
            p = E.keyed_rlc_plan_info(scheme, n, 5, 8, g)
            q = E.rlc_plan_info(scheme, n, 8, g)
            assert (p["groups"], p["sub"]) == (q["groups"], q["sub"])
            assert p["groups"] * p["sub"] >= n > (p["groups"] - 1) * p["sub"]


def test_keyed_workspace_size():
    for bits in (0, 8, 16):
        prev = 0
        for n in SIZES + [(1 << 22) + 1, 3 << 22]:
            sizes = [E.keyed_rlc_workspace_bytes(n, k, bits) for k in (0, 1, 64, 4096, 16384)]
            assert all(s % 256 == 0 for s in sizes), (n, bits, sizes)
            assert sizes == sorted(sizes), (n, bits, sizes)      # never smaller for more keys
            assert sizes[2] >= prev, (n, bits)                    # ... nor for more items
            prev = sizes[2]
            if n <= 1 << 22:
                for scheme in SCHEMES:
                    for g in (1, 4, 16):
                        assert sizes[2] >= E.keyed_rlc_plan_info(scheme, n, 64, bits, g)["bytes"], (scheme, n, g)
    L = _lib.load()
    assert L.dsv_keyed_rlc_workspace_bytes(ctypes.c_size_t(10), ctypes.c_size_t(3), ctypes.c_int(10)) == 0
    assert L.dsv_keyed_rlc_workspace_bytes(ctypes.c_size_t(10), ctypes.c_size_t(3), ctypes.c_int(5)) == 0


def test_keyed_plan_argument_checks():
    L = _lib.load()
    out = (ctypes.c_uint64 * 24)()

    def info(scheme, n, k, bits, groups):
        return L.dsv_keyed_rlc_plan_info(ctypes.c_int(scheme), ctypes.c_size_t(n), ctypes.c_size_t(k),
                                         ctypes.c_int(bits), ctypes.c_int(groups), out)

    assert info(0, 100, 4, 8, 1) == 0
    for bad in ((3, 100, 4, 8, 1), (-1, 100, 4, 8, 1), (0, 100, 4, 10, 1), (0, 100, 4, 7, 1),
                (0, (1 << 22) + 1, 4, 8, 1), (0, 0, 4, 8, 1), (0, 100, 4, 8, 17), (1, 100, 4, 8, -1)):
        assert info(*bad) != 0, bad
    # the unkeyed plan still knows three schemes only
    assert L.dsv_rlc_plan_info(ctypes.c_int(3), ctypes.c_size_t(100), ctypes.c_int(8), ctypes.c_int(1), out) != 0


# ---- a model of the per-key aggregation (keyed_rlc.h), on the curve model of tests/pymodel.py ----------------
def _keyed_batch(scheme, n, k, rnd):
    keys = []
    for _ in range(k):
        sk = rnd.randrange(1, M.R_ORDER)
        if scheme == "single":
            keys.append((sk, M.pmul(M.GEN, sk), None))
        elif scheme == "double":
            keys.append((sk, M.pmul(M.GEN, sk), M.pmul(M.GEN_NUMS, sk)))
        else:
            gen = M.pmul(M.GEN, rnd.randrange(1, M.R_ORDER))
            keys.append((sk, M.pmul(gen, sk), gen))
    items = []
    for _ in range(n):
        j = rnd.randrange(k)
        sk, pk, p2 = keys[j]
        m, r = rnd.randrange(M.Q), rnd.randrange(1, M.R_ORDER)
        if scheme == "single":
            u, R = M.sign_single(sk, m, r)
            items.append((j, u, M.challenge(R, m), R, None))
        elif scheme == "double":
            u, R, Rp = M.sign_double(sk, m, r)
            items.append((j, u, M.challenge_double(R, Rp, m), R, Rp))
        else:
            u, R = M.sign_vargen(sk, p2, m, r)
            items.append((j, u, M.challenge(R, m), R, None))
    return keys, items


def _aggregate(scheme, keys, items, rnd):
    """the identity test (3) of keyed_rlc.h, with per-key scalars accumulated as the prep does: eight 32-bit
    chunks of each z c (z u) mod r summed unreduced, reduced once per key"""
    r = M.R_ORDER
    chunks = {}
    fixed = [0, 0]
    tot = M.IDENTITY
    for (j, u, c, R, Rp) in items:
        zs = [rnd.getrandbits(128) for _ in range(2 if scheme == "double" else 1)]
        scal = [z * c % r for z in zs] if scheme != "vargen" else [zs[0] * c % r, zs[0] * u % r]
        if scheme != "vargen":
            for h, z in enumerate(zs):
                fixed[h] = (fixed[h] + z * u) % r
        acc = chunks.setdefault(j, [[0] * 8 for _ in scal])
        for s, v in enumerate(scal):
            for w in range(8):
                acc[s][w] += (v >> (32 * w)) & 0xFFFFFFFF
        tot = M.padd(tot, M.pneg(M.pmul(R, zs[0])))
        if Rp is not None:
            tot = M.padd(tot, M.pneg(M.pmul(Rp, zs[1])))
    for j, acc in chunks.items():
        sk, pk, p2 = keys[j]
        pts = [pk] + ([p2] if scheme != "single" else [])
        for s, words in enumerate(acc):
            total = sum(x << (32 * w) for w, x in enumerate(words))
            assert total < 1 << 278
            tot = M.padd(tot, M.pmul(pts[s], total % r))
    if scheme != "vargen":
        tot = M.padd(tot, M.pmul(M.GEN, fixed[0]))
        if scheme == "double":
            tot = M.padd(tot, M.pmul(M.GEN_NUMS, fixed[1]))
    return tot == M.IDENTITY


@pytest.mark.parametrize("scheme", SCHEMES)
def test_model_of_the_per_key_aggregate(scheme):
    rnd = random.Random({"single": 11, "double": 12, "vargen": 13}[scheme])
    keys, items = _keyed_batch(scheme, 12, 3, rnd)
    assert _aggregate(scheme, keys, items, rnd)
    j, u, c, R, Rp = items[5]
    wrong = list(items)
    wrong[5] = (j, (u + 1) % M.R_ORDER, c, R, Rp)  # one wrong signature
    assert not _aggregate(scheme, keys, wrong, rnd)
    moved = list(items)
    moved[7] = ((items[7][0] + 1) % 3,) + items[7][1:]  # signed under one key, claimed under another
    assert not _aggregate(scheme, keys, moved, rnd)


def test_chunked_key_sums_reduce_like_the_whole():
    """the prep's unreduced chunk sums (at most 2^22 terms below 2^32 per chunk) reduce to the sum mod r"""
    rnd = random.Random(5)
    vals = [rnd.randrange(M.R_ORDER) for _ in range(500)] + [M.R_ORDER - 1] * 20
    words = [sum((v >> (32 * w)) & 0xFFFFFFFF for v in vals) for w in range(8)]
    total = sum(x << (32 * w) for w, x in enumerate(words))
    assert total % M.R_ORDER == sum(vals) % M.R_ORDER
    assert (1 << 22) * ((1 << 32) - 1) < 1 << 54


# ---- register budget of k_keyed_rlc.hip (assembly cached like tests/test_isa_guard.py) ----------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and
                    subprocess.run(["which", "hipcc"], capture_output=True).returncode != 0,
                    reason="hipcc not available")
def test_keyed_rlc_kernels_stay_in_registers():
    from isa_asm import CSRC, _asm, _kernel_info, _stamp

    info = _kernel_info(_asm(os.path.join(CSRC, "k_keyed_rlc.hip"), _stamp()))
    names = ["k_keyed_rlc_prepILi0E", "k_keyed_rlc_prepILi1E", "k_keyed_rlc_prepILi2E", "k_keyed_rlc_torsion",
             "k_keyed_rlc_termsILi0E", "k_keyed_rlc_termsILi1E", "k_keyed_rlc_termsILi2E", "k_keyed_rlc_reduce",
             "k_keyed_fallbackILi0E", "k_keyed_fallbackILi1E", "k_keyed_fallbackILi2E"]
    for needle in names:
        hits = [k for k in info if needle in k]
        assert len(hits) == 1, (needle, sorted(info))
        k = info[hits[0]]
        assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0, (needle, k)
    # the existing kernels are still one instantiation each (tests/test_isa_guard.py, test_keyset_abi.py)
    rlc = _kernel_info(_asm(os.path.join(CSRC, "k_rlc.hip"), _stamp()))
    for needle in ("k_rlc_accumulate", "k_rlc_scale"):
        hits = [k for k in rlc if needle in k]
        assert len(hits) == 1 and rlc[hits[0]]["scratch"] == 0, (needle, hits)
