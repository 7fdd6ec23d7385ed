"""Key sets by key value on the GPU (dsv_keyset_lookup*, dsv_verify_keyed_lookup*): the lookup against a Python
dict over the registered keys' bytes, duplicates and invalid keys, probes that wrap round the end of the slot
table, collisions at size, closed-set verify against the oracle and against the keyed call at the dict's
indices, and the _dev contract.  Keys and items come from tests/keyed_cases.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import harness as H
import pymodel as M
from keyed_cases import (_check_lookup, _dev, _diff, _expect, _expect_rec, _key_records, _keys, _le, _poison, _scalars,
                         _value_args, _value_batch, _where, _where_rec)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
NONE = 0xFFFFFFFF
Q = M.Q
INVALID, NOT_INITIALIZED = -2, -1


# ---- 1. lookup parity with a dict --------------------------------------------------------------------------
MISS_KINDS = ("other_key", "negated", "mixed_pair", "flip_u0", "flip_v31", "u_plus_q", "zeros", "ones")


def _lookup_items(rng, P0, P1, X0, X1, n):
    """n key rows: registered keys at random indices, roughly one in eight replaced by a miss of each kind in
    turn (applied to the second point of a two-point key every other time); X0 / X1: valid keys not registered"""
    k = len(P0)
    idx = rng.integers(0, k, size=n)
    A = P0[idx].copy()
    B = P1[idx].copy() if P1 is not None else None
    turn = 0
    for i in np.flatnonzero(rng.integers(0, 8, size=n) == 0):
        kind = MISS_KINDS[turn % len(MISS_KINDS)]
        on_b = B is not None and (turn // len(MISS_KINDS)) % 2 == 1
        turn += 1
        T = B if on_b else A
        if kind == "other_key":
            j = int(rng.integers(0, len(X0)))
            A[i] = X0[j]
            if B is not None:
                B[i] = X1[j]
        elif kind == "negated":  # -P: same v, u -> q - u
            T[i, :32] = _le((Q - M.from_le(T[i, :32])) % Q)
        elif kind == "mixed_pair":  # a registered PK with another registered key's second point
            if B is None:
                A[i] = X0[int(rng.integers(0, len(X0)))]
            elif k > 1:
                B[i] = P1[(idx[i] + 1 + int(rng.integers(0, k - 1))) % k]
            else:
                B[i] = X1[0]
        elif kind == "flip_u0":
            T[i, 0] ^= 1
        elif kind == "flip_v31":
            T[i, 63] ^= 1
        elif kind == "u_plus_q":  # the same residue, not canonical (q < 2^255: it fits)
            T[i, :32] = _le(M.from_le(T[i, :32]) + Q)
        elif kind == "zeros":
            T[i] = 0
        else:
            T[i] = 0xFF
    return A, B


@pytest.mark.parametrize("k", (1, 2, 33))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_lookup_matches_dict(engine, scheme, k):
    extra = 8
    _, _, K0, K1 = _keys(engine, scheme, k + extra, 500 + k)
    P0, X0 = np.ascontiguousarray(K0[:k]), K0[k:]
    P1, X1 = (np.ascontiguousarray(K1[:k]), K1[k:]) if K1 is not None else (None, None)
    rng = np.random.default_rng(77 * k + len(scheme))
    with engine.KeySet(scheme, P0, P1) as ks:
        kok = ks.key_ok()
        assert (kok == 1).all()
        where = _where(P0, P1, kok)
        assert len(where) == k
        st = ks.index_stats()
        assert st["capacity"] == max(64, 1 << (2 * k - 1).bit_length()) and st["occupied"] == k
        missed = 0
        for n in (1, 63, 64, 65, 4099):
            A, B = _lookup_items(rng, P0, P1, X0, X1, n)
            want = _check_lookup(ks, where, A, B, (scheme, k, n))
            missed += int((want == NONE).sum())
            if n == 4099:
                assert 300 < (want == NONE).sum() < 800 and len(set(want.tolist())) == k + 1
        assert missed > 0


@pytest.mark.parametrize("scheme", SCHEMES)
def test_lookup_on_sets_of_every_constructor(engine, scheme):
    """the index is built behind all three constructors: a set from the reference's key records (decompressed on
    the device) and one from its key objects (normalised on the device) hold the canonical affine bytes the
    affine constructor is given, so the same key columns look up to the same indices"""
    import mont_cases as MC
    import oracle_lib as O

    k, extra, n = 33, 8, 4099
    _, _, K0, K1 = _keys(engine, scheme, k + extra, 4711)
    P0, X0 = np.ascontiguousarray(K0[:k]), K0[k:]
    P1, X1 = (np.ascontiguousarray(K1[:k]), K1[k:]) if K1 is not None else (None, None)
    rng = np.random.default_rng(len(scheme))
    rec = O.compress(P0) if P1 is None else np.hstack([O.compress(P0), O.compress(P1)])
    limbs = [MC.to_limbs_py(H.projective(P, rng)[0], Q) for P in ([P0] if P1 is None else [P0, P1])]
    A, B = _lookup_items(rng, P0, P1, X0, X1, n)
    where = _where(P0, P1, np.ones(k, np.uint8))
    sets = {"affine": lambda: engine.KeySet(scheme, P0, P1),
            "wire": lambda: engine.KeySet.from_wire(scheme, np.ascontiguousarray(rec)),
            "mont_cols": lambda: engine.KeySet.from_mont_cols(scheme, limbs)}
    for form, make in sets.items():
        with make() as ks:
            assert (ks.key_ok() == 1).all(), form
            st = ks.index_stats()
            assert st["capacity"] == 128 and st["occupied"] == k, (form, st)
            want = _check_lookup(ks, where, A, B, (scheme, form))
            assert 300 < (want == NONE).sum() < 800


# ---- 2. duplicates and invalid keys ------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_duplicates_and_invalid_keys(engine, scheme):
    k = 24
    _, _, P0, P1 = _keys(engine, scheme, k, 909)
    P0 = P0.copy()
    P1 = P1.copy() if P1 is not None else None
    for j in (7, 20):  # the same key at 3, 7 and 20
        P0[j] = P0[3]
        if P1 is not None:
            P1[j] = P1[3]
    off = P1 if P1 is not None else P0  # off the curve: v changed (the second point of a two-point key)
    off[5, 40] ^= 1
    assert not M.on_curve(H.to_int_point(off[5]))
    P0[9, :32] = _le(M.from_le(P0[9, :32]) + Q)  # a coordinate >= q, same residue
    with engine.KeySet(scheme, P0, P1) as ks:
        kok = ks.key_ok()
        assert kok[5] == 0 and kok[9] == 0 and kok.sum() == k - 2
        want = np.arange(k, dtype=np.uint32)
        want[[7, 20]] = 3
        want[[5, 9]] = NONE
        where = _where(P0, P1, kok)
        assert (_expect(where, P0, P1) == want).all()
        got = _check_lookup(ks, where, P0, P1, scheme)
        assert (got == want).all()
        st = ks.index_stats()
        assert st["occupied"] == k - 4 == len(where), st
        assert st["capacity"] == 64


# ---- 3. probes that wrap round the end of the table --------------------------------------------------------
def test_wrap_around(engine):
    k, cap = 24, 64
    _, _, C, _ = _keys(engine, "single", 600, 20261018)
    homes = np.array([engine.keyset_home_slot("single", k, C[j]) for j in range(len(C))])
    assert (homes < cap).all()
    last = np.flatnonzero(homes >= cap - 2)
    assert len(last) >= 3, len(last)  # about 19 of 600 are expected
    used, unused = last[:6], last[6:]
    rest = np.flatnonzero(homes < cap - 2)[:k - len(used)]
    rng = np.random.default_rng(3)
    order = rng.permutation(np.concatenate([used, rest]))
    P0 = np.ascontiguousarray(C[order])
    assert len(P0) == k
    with engine.KeySet("single", P0) as ks:
        where = _where(P0, None, ks.key_ok())
        got = _check_lookup(ks, where, P0, None, "registered")
        assert (got == np.arange(k)).all()
        if len(unused):
            got = _check_lookup(ks, where, np.ascontiguousarray(C[unused]), None, "unused")
            assert (got == NONE).all()
        st = ks.index_stats()
        assert st["capacity"] == cap and st["occupied"] == k
        assert st["longest_probe"] >= 2 and st["displaced"] >= 1, st


# ---- 4. collisions at size ---------------------------------------------------------------------------------
def test_collisions_at_size(engine):
    k = 1500
    _, _, C, _ = _keys(engine, "single", 2 * k, 31337)
    P0 = np.ascontiguousarray(C[:k])
    rng = np.random.default_rng(4)
    items = np.ascontiguousarray(C[rng.permutation(2 * k)])
    with engine.KeySet("single", P0) as ks:
        st = ks.index_stats()
        assert st["capacity"] == 4096 and st["occupied"] == k
        assert st["displaced"] > 0 and st["longest_probe"] >= 2, st
        where = _where(P0, None, ks.key_ok())
        want = _check_lookup(ks, where, items, None, "n = 3000")
        assert (want == NONE).sum() == k and len(set(want.tolist())) == k + 1


# ---- 5. verify by value ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 65, 4099))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_verify_by_value(engine, scheme, n):
    b = _value_batch(engine, scheme)
    with engine.KeySet(scheme, b["P0"], b["P1"]) as ks:
        where = _where(b["P0"], b["P1"], ks.key_ok())
        idx = _expect(where, b["A"][:n], b["B"][:n] if b["B"] is not None else None)
        found = idx != NONE
        nmiss = int((~found).sum())
        want = b["oracle"][:n].astype(np.uint8) & found.astype(np.uint8)
        if n == 4099:
            assert nmiss > 0 and 0 < want.sum() < n
        # the keyed call at the dict's indices (a miss: DSV_KEY_NONE, which reads no table and gives 0)
        pts = [b["R"][:n]] + ([b["Rp"][:n]] if b["Rp"] is not None else [])
        dk = _dev([b["u"][:n]] + pts + [idx, b["m"][:n]])
        ok = _poison(n)
        ws = torch.empty(max(engine.keyed_workspace_bytes(n), 1), dtype=torch.uint8, device=DEV)
        ks.verify_dev(*dk, ok, ws)
        torch.cuda.synchronize()
        keyed = ok.cpu().numpy()
        assert (keyed == want).all(), (scheme, n, "keyed", _diff(keyed, want))
        # _dev form
        args = _value_args(b, n)
        ok = _poison(n)
        ws = torch.empty(engine.keyed_lookup_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        ks.verify_lookup_dev(*_dev(args), ok, ws, misses=misses)
        torch.cuda.synchronize()
        got = ok.cpu().numpy()
        assert (got == want).all(), (scheme, n, "dev", _diff(got, want))
        assert int(misses.item()) == nmiss
        # host form
        got, hm = ks.verify_lookup(*args)
        assert (got == want).all(), (scheme, n, "host", _diff(got, want))
        assert hm == nmiss


def test_verify_by_value_rejects_a_valid_signature_under_an_unregistered_key(engine):
    """the closed-set meaning: the unkeyed verdict is 1, the key is not in the set, the verdict is 0"""
    sk, _, P0, _ = _keys(engine, "single", 5, 2024)
    rng = np.random.default_rng(1)
    n = 40
    idx = rng.integers(0, 5, size=n)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R = engine.sign_single(sk[idx], m, r)
    assert (engine.verify_single(u, R, P0[idx], m) == 1).all()
    with engine.KeySet("single", np.ascontiguousarray(P0[:4])) as ks:
        ok, misses = ks.verify_lookup(u, R, P0[idx], m)
    assert (ok == (idx < 4)).all() and misses == int((idx == 4).sum()) > 0


# ---- 5b. the host forms across a chunk boundary ------------------------------------------------------------
HOST_CHUNK = 1 << 18  # items per chunk of the by-value host forms


def _tiled(a, n):
    return np.ascontiguousarray(np.concatenate([a] * -(-n // len(a)))[:n])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_host_lookups_across_a_chunk_boundary(engine, scheme):
    """dsv_keyset_lookup and dsv_keyset_lookup_wire on 2^18 + 5 host items tiled from 4099: the second chunk
    holds five items; the indices are the dict model's and `misses` is the sum over both chunks"""
    k, extra, base, n = 33, 8, 4099, HOST_CHUNK + 5
    _, _, K0, K1 = _keys(engine, scheme, k + extra, 4711)
    P0, X0 = np.ascontiguousarray(K0[:k]), K0[k:]
    P1, X1 = (np.ascontiguousarray(K1[:k]), K1[k:]) if K1 is not None else (None, None)
    rng = np.random.default_rng(len(scheme))
    A, B = _lookup_items(rng, P0, P1, X0, X1, base)
    # records: registered and unregistered keys at random, every 16th with a flipped byte
    pk = _key_records(K0, K1)[rng.integers(0, k + extra, size=base)].copy()
    pk[::16, 5] ^= 1
    kok = np.ones(k, np.uint8)
    cases = (("affine", _expect(_where(P0, P1, kok), A, B),
              lambda ks: ks.lookup(*[_tiled(c, n) for c in ([A] + ([B] if B is not None else []))])),
             ("wire", _expect_rec(_where_rec(P0, P1, kok), pk), lambda ks: ks.lookup_wire(_tiled(pk, n))))
    with engine.KeySet(scheme, P0, P1) as ks:
        assert (ks.key_ok() == 1).all()
        for form, want, call in cases:
            want = _tiled(want, n)
            nmiss = int((want == NONE).sum())
            assert 0 < nmiss < n, (form, nmiss)
            got, misses = call(ks)
            assert got.shape == (n,) and (got == want).all(), (scheme, form, _diff(got, want))
            assert misses == nmiss, (scheme, form, misses, nmiss)


@pytest.mark.parametrize("scheme", ("single", "double"))
def test_verify_by_value_host_across_a_chunk_boundary(engine, scheme):
    """dsv_verify_keyed_lookup on 2^18 + 5 host items tiled from the parity batch: the second chunk holds five
    items; verdicts and `misses` equal the _dev form's and the tiled expectation"""
    b = _value_batch(engine, scheme)
    base, n = len(b["m"]), HOST_CHUNK + 5
    with engine.KeySet(scheme, b["P0"], b["P1"]) as ks:
        found = _expect(_where(b["P0"], b["P1"], ks.key_ok()), b["A"], b["B"]) != NONE
        want = _tiled(b["oracle"].astype(np.uint8) & found.astype(np.uint8), n)
        nmiss = int((~_tiled(found, n)).sum())
        assert 0 < nmiss < n and 0 < want.sum() < n
        args = [_tiled(c, n) for c in _value_args(b, base)]
        ok = _poison(n)
        ws = torch.empty(engine.keyed_lookup_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        ks.verify_lookup_dev(*_dev(args), ok, ws, misses=misses)
        torch.cuda.synchronize()
        dev = ok.cpu().numpy()
        assert (dev == want).all(), (scheme, "dev", _diff(dev, want))
        assert int(misses.item()) == nmiss
        got, hm = ks.verify_lookup(*args)
        assert (got == dev).all(), (scheme, "host", _diff(got, dev))
        assert hm == nmiss


# ---- 6. the _dev contract ----------------------------------------------------------------------------------
def test_dev_contract(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    b = _value_batch(engine, "double")
    n = 65
    du, dR, dRp, dA, dB, dm = _dev(_value_args(b, n))
    vp, sz, null = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p(None)
    p = lambda t: vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    ws_bytes = engine.keyed_lookup_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    ks = engine.KeySet("double", b["P0"], b["P1"])
    try:
        h = ks._h

        def verify(nn, okt, wsb, Rp=p(dRp), key_b=p(dB)):
            return L.dsv_verify_keyed_lookup_dev(h, p(du), p(dR), Rp, p(dA), key_b, p(dm), sz(nn), p(okt), p(ws),
                                                 sz(wsb), stream, null)

        ok = _poison(n)
        # a workspace one byte short, NULL key_b, NULL Rp_uv: an error, nothing launched
        assert verify(n, ok, ws_bytes - 1) == INVALID
        assert b"workspace" in L.dsv_last_error()
        assert verify(n, ok, ws_bytes, key_b=null) == INVALID
        assert verify(n, ok, ws_bytes, Rp=null) == INVALID
        assert L.dsv_keyset_lookup_dev(h, p(dA), null, sz(n), p(out), null, stream) == INVALID
        assert L.dsv_keyset_lookup_dev(h, p(dA), p(dB), sz(n), null, null, stream) == INVALID
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all() and (out.cpu().numpy() == 0x5A5A5A5A).all()
        with pytest.raises(ValueError):
            ks.verify_lookup_dev(du, dR, dRp, dA, dB, dm, ok, ws[:-1])
        with pytest.raises(ValueError):
            ks.verify_lookup_dev(du, dR, dA, dB, dm, ok, ws)  # single arguments on a double key set
        with pytest.raises(ValueError):
            ks.lookup(b["A"][:n])
        odd = torch.zeros(n * 64 + 8, dtype=torch.uint8, device=DEV)[8:].view(n, 64)  # 8 bytes off a 16-byte boundary
        with pytest.raises(ValueError):
            ks.lookup_dev(odd, dB, out)
        assert L.dsv_keyset_lookup_dev(h, p(odd), p(dB), sz(n), p(out), null, stream) == INVALID
        # n = 0: DSV_OK, nothing touched (no workspace needed)
        assert verify(0, ok, 0) == 0
        assert L.dsv_keyset_lookup_dev(h, p(dA), p(dB), sz(0), p(out), null, stream) == 0
        hm = sz(55)
        assert L.dsv_keyset_lookup(h, null, null, sz(0), null, ctypes.byref(hm)) == 0 and hm.value == 0
        hm = sz(55)
        assert L.dsv_verify_keyed_lookup(h, null, null, null, null, null, null, sz(0), null, ctypes.byref(hm)) == 0
        assert hm.value == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all() and (out.cpu().numpy() == 0x5A5A5A5A).all()
        # the full workspace: the verdicts
        assert verify(n, ok, ws_bytes) == 0, L.dsv_last_error().decode()
        torch.cuda.synchronize()
        where = _where(b["P0"], b["P1"], ks.key_ok())
        found = _expect(where, b["A"][:n], b["B"][:n]) != NONE
        assert (ok.cpu().numpy() == (b["oracle"][:n].astype(np.uint8) & found.astype(np.uint8))).all()
        # two streams, one set, lookups in flight together: both exact
        big = 4099
        rng = np.random.default_rng(12)
        batches = []
        for s in range(2):
            A, B = _lookup_items(rng, b["P0"], b["P1"], b["P0"][::-1], b["P1"], big)
            batches.append((A, B, _dev([A, B]), torch.cuda.Stream(device=DEV),
                            torch.full((big,), 0x5A5A5A5A, dtype=torch.int32, device=DEV),
                            torch.full((1,), 999, dtype=torch.int32, device=DEV)))
        torch.cuda.synchronize()
        for _ in range(4):
            for A, B, cols, st, o, ms in batches:
                ks.lookup_dev(*cols, o, misses=ms, stream=st)
        torch.cuda.synchronize()
        for A, B, cols, st, o, ms in batches:
            want = _expect(where, A, B)
            got = o.cpu().numpy().view(np.uint32)
            assert (got == want).all(), _diff(got, want)
            assert int(ms.item()) == int((want == NONE).sum()) > 0
    finally:
        ks.close()
    # a closed set has no handle left to call with
    with pytest.raises(ValueError):
        ks.lookup(b["A"][:n], b["B"][:n])
    with pytest.raises(ValueError):
        ks.verify_lookup_dev(du, dR, dRp, dA, dB, dm, _poison(n), ws)


def test_by_value_calls_after_shutdown():
    """a process of its own (the session's engine stays up): a set whose device was shut down — the handle is still
    the caller's, the set is dead, and every by-value call says so through the keyed calls' own check"""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
import torch
from schnorr_amd import engine as E, _lib
E.init(0)
L = _lib.load()
sk = np.zeros((2, 32), np.uint8); sk[:, 0] = (3, 5)
pk = E.public_keys(sk)
ks = E.KeySet("single", pk)
idx, misses = ks.lookup(pk[::-1].copy())
assert idx.tolist() == [1, 0] and misses == 0
assert ks.index_stats()["occupied"] == 2
d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
E.shutdown()
h = ks._h
u = np.zeros((1, 32), np.uint8); P = np.zeros((1, 64), np.uint8); out = np.zeros(1, np.uint32); ok = np.zeros(1, np.uint8)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
dp = ctypes.c_void_p(d.data_ptr())
one = ctypes.c_size_t(1)
assert L.dsv_keyset_lookup(h, p(P), None, one, p(out), None) == -1
assert b"key set" in L.dsv_last_error(), L.dsv_last_error()
assert L.dsv_verify_keyed_lookup(h, p(u), p(P), None, p(P), None, p(u), one, p(ok), None) == -1
assert L.dsv_keyset_lookup_dev(h, dp, None, one, dp, None, None) == -1
assert L.dsv_verify_keyed_lookup_dev(h, dp, dp, None, dp, None, dp, one, dp, dp, ctypes.c_size_t(4096), None, None) == -1
stats = (ctypes.c_uint64 * 4)()
assert L.dsv_debug_keyset_index_stats(h, stats) == -1
ks.close()
print("ok")
""" % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
