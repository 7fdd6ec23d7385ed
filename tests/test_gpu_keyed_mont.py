"""The keyed typed-object form on the GPU (dsv_keyset_create_mont_cols, dsv_verify_keyed_mont_*;
KeySet.from_mont_cols / verify_mont_dev / verify_mont_cols / submit_mont_cols): the reference's in-memory objects —
Montgomery limbs, projective points — against a registered key set.  Whole-vector equality everywhere: with the
oracle's verdicts on the limbs of the gathered keys, with the encodings the Rust types cannot hold planted in
items and in keys, from records laid out like the Rust structs, with the set dsv_keyset_create builds, with the
affine keyed call and the unkeyed typed call at 2^20 items; the _dev contract, the host form at the host
pipeline's edges, jobs and lifetime."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import dispatch_edges as D
import mont_cases as MC
import pymodel as M
import keyed_cases as KC
from keyed_cases import _diff, _limbs, _oracle_mont_cols, _poison, _to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
NS = (1, 63, 64, 65, 4099, (1 << 16) + 3)
Q, R_ORDER = M.Q, M.R_ORDER


def _reduced(arr, mod):
    """canonical bytes of the values: the tamper classes u + r / m + q have no limb form"""
    out = arr.copy()
    for i in range(len(out)):
        v = M.from_le(out[i])
        if v >= mod:
            out[i] = np.frombuffer(M.le32(v % mod), np.uint8)
    return out


def _oracle_mont(scheme, b, keys, idx=None, rows=slice(None)):
    """the oracle's typed verify on (u, R[, R'], keys[idx]..., m) in limbs: it alone fixes the expectation"""
    idx = b["idx"] if idx is None else idx
    pts = [b["Rl"]] + ([b["Rpl"]] if scheme == "double" else [])
    cols = [b["ul"]] + pts + [kp[idx] for kp in keys] + [b["ml"]]
    return _oracle_mont_cols(scheme, [c[rows] for c in cols])


_MONT = {}


def _mont_batch(engine, scheme, k, n):
    """keyed_cases._batch in the reference's in-memory form: every point re-represented with a random z,
    everything converted to limbs with Python integers; `want` from the oracle's typed verify"""
    key = (scheme, k, n)
    if key not in _MONT:
        b = KC._batch(engine, scheme, k, n)
        rng = np.random.default_rng(5 * k + n)
        out = {"idx": b["idx"].copy(), "P0": b["P0"], "P1": b["P1"], "R": b["R"], "Rp": b["Rp"],
               "u": _reduced(b["u"], R_ORDER), "m": _reduced(b["m"], Q)}
        out["ul"], out["ml"] = MC.to_limbs_py(out["u"], R_ORDER), MC.to_limbs_py(out["m"], Q)
        out["Rl"] = _limbs(b["R"], rng)
        out["Rpl"] = _limbs(b["Rp"], rng) if scheme == "double" else None
        out["keys"] = [_limbs(b["P0"], rng)] + ([_limbs(b["P1"], rng)] if b["P1"] is not None else [])
        out["want"] = _oracle_mont(scheme, out, out["keys"])
        if len(_MONT) > 3:
            _MONT.pop(next(iter(_MONT)))
        _MONT[key] = out
    return _MONT[key]


def _cols(scheme, b, rows=slice(None), idx=None):
    """(u, R[, R'], idx, m) limb columns of the batch"""
    idx = b["idx"] if idx is None else idx
    pts = [b["Rl"][rows]] + ([b["Rpl"][rows]] if scheme == "double" else [])
    return [b["ul"][rows]] + pts + [idx[rows], b["ml"][rows]]


def _run_dev(engine, ks, darrs, n, stream=None):
    ok = _poison(n)
    ws = torch.empty(max(engine.keyed_mont_workspace_bytes(ks.scheme, n), 1), dtype=torch.uint8, device=DEV)
    ks.verify_mont_dev(*[a[:n] for a in darrs], ok, ws, stream=stream)
    torch.cuda.synchronize()
    return ok.cpu().numpy()


def _mont_dev(engine, ks, cols):
    return _run_dev(engine, ks, [_to_dev(c) for c in cols], len(cols[0]))


# ---- 1. oracle parity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 37, 1000))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_oracle_parity(engine, scheme, k):
    b = _mont_batch(engine, scheme, k, NS[-1])
    want = b["want"]
    assert 0 < want.sum() < len(want)
    with engine.KeySet.from_mont_cols(scheme, b["keys"]) as ks:
        assert ks.k == k and ks.nbytes == engine.keyset_bytes(scheme, k)
        assert (ks.key_ok() == 1).all()
        cols = _cols(scheme, b)
        darrs = [_to_dev(c) for c in cols]
        for n in NS:
            got = _run_dev(engine, ks, darrs, n)
            assert (got == want[:n]).all(), (scheme, k, n, _diff(got, want[:n]))
            host = ks.verify_mont_cols([c[:n] for c in cols])
            assert (host == want[:n]).all(), (scheme, k, n, _diff(host, want[:n]))


# ---- 2. encodings the Rust types cannot hold --------------------------------------------------------------
def _plant_items(scheme, b):
    """z = 0 and a coordinate >= q in every nonce point, m = q, u = r + 5, on items that verify -> (a batch
    with the plants, the planted rows)"""
    p = dict(b)
    for f in ("ul", "ml", "Rl", "Rpl"):
        p[f] = b[f].copy() if b[f] is not None else None
    rows = iter(np.flatnonzero(b["want"] == 1)[5:].tolist())
    planted = []
    for j, f in enumerate(("Rl", "Rpl") if scheme == "double" else ("Rl",)):
        i0, i1, i2 = next(rows), next(rows), next(rows)
        p[f][i0, 64:96] = 0                                             # z = 0
        p[f][i1, 32 * j:32 * j + 32] = 0xFF                             # limbs >= q
        p[f][i2, 64:96] = np.frombuffer(M.le32(Q), np.uint8)            # z: exactly q
        planted += [i0, i1, i2]
    im, iu = next(rows), next(rows)
    p["ml"][im] = np.frombuffer(M.le32(Q), np.uint8)
    p["ul"][iu] = np.frombuffer(M.le32(R_ORDER + 5), np.uint8)
    return p, planted + [im, iu]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_unholdable_items_give_zero(engine, scheme):
    b = _mont_batch(engine, scheme, 37, 4099)
    p, planted = _plant_items(scheme, b)
    want = _oracle_mont(scheme, p, b["keys"])
    expect = b["want"].copy()
    expect[planted] = 0
    assert (want == expect).all() and (b["want"][planted] == 1).all()  # each plant turns a 1 into the oracle's 0
    assert 0 < want.sum() < len(want)
    with engine.KeySet.from_mont_cols(scheme, b["keys"]) as ks:
        cols = _cols(scheme, p)
        got = _mont_dev(engine, ks, cols)
        assert (got == want).all(), _diff(got, want)
        host = ks.verify_mont_cols(cols)
        assert (host == want).all(), _diff(host, want)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_unholdable_keys_give_zero(engine, scheme):
    b = _mont_batch(engine, scheme, 37, 4099)
    npts = len(b["keys"])
    keys = [kp.copy() for kp in b["keys"]]
    last = npts - 1
    keys[0][3, 64:96] = 0                                               # z = 0
    keys[last][5, 0:32] = 0xFF                                          # a coordinate >= q
    keys[last][7, 64:96] = np.frombuffer(M.le32(Q), np.uint8)           # z = q
    # off the curve: u + 1 in the affine point, re-represented
    off = b["P0"][11:12].copy()
    off[0, :32] = np.frombuffer(M.le32((M.from_le(off[0, :32]) + 1) % Q), np.uint8)
    keys[0][11] = _limbs(off, np.random.default_rng(3))[0]
    bad = [3, 5, 7, 11]
    under = np.isin(b["idx"], bad)
    assert all((b["want"][b["idx"] == j] == 1).any() for j in bad)
    expect = b["want"].copy()
    expect[under] = 0
    assert 0 < expect.sum() < len(expect)
    # the oracle on the limb-invalid keys (the off-curve one is no value of the Rust type either)
    limb_bad = np.isin(b["idx"], bad[:3])
    assert (_oracle_mont(scheme, b, keys)[limb_bad] == 0).all()
    with engine.KeySet.from_mont_cols(scheme, keys) as ks:
        ok = ks.key_ok()
        assert (ok[bad] == 0).all() and ok.sum() == 37 - len(bad)
        cols = _cols(scheme, b)
        got = _mont_dev(engine, ks, cols)
        assert (got == expect).all(), _diff(got, expect)
        host = ks.verify_mont_cols(cols)
        assert (host == expect).all(), _diff(host, expect)
    # bad keys that no item references do not matter
    more = [np.concatenate([kp, keys[j][bad]]) for j, kp in enumerate(b["keys"])]
    with engine.KeySet.from_mont_cols(scheme, more) as ks:
        ok = ks.key_ok()
        assert ks.k == 41 and (ok[:37] == 1).all() and (ok[37:] == 0).all()
        got = _mont_dev(engine, ks, _cols(scheme, b))
        assert (got == b["want"]).all(), _diff(got, b["want"])


# ---- 3. records where they lie ----------------------------------------------------------------------------
CALLER_ITEM = np.dtype([("tag", "<u8"), ("key", "<u4"), ("flags", "<u4")])  # key_idx inside a caller's struct


def _unkeyed_cols(scheme, b, keys, rows=slice(None)):
    pts = [b["Rl"][rows]] + ([b["Rpl"][rows]] if scheme == "double" else [])
    return [b["ul"][rows]] + pts + [kp[b["idx"][rows]] for kp in keys] + [b["ml"][rows]]


@pytest.mark.parametrize("scheme", SCHEMES)
def test_records_where_they_lie(engine, scheme):
    b = _mont_batch(engine, scheme, 37, 4099)
    n, k = 4099, 37
    nsig = 2 if scheme == "double" else 1
    sigs, _, msgs, views = MC.as_records(scheme, _unkeyed_cols(scheme, b, b["keys"]))
    assert sigs.dtype.itemsize == (352 if scheme == "double" else 192)
    # the key objects: k records of the Rust key struct, filled through the same layout helper
    zero32, zero96 = np.zeros((k, 32), np.uint8), np.zeros((k, 96), np.uint8)
    _, pks, _, kviews = MC.as_records(scheme, [zero32] + [zero96] * nsig + list(b["keys"]) + [zero32])
    assert pks.dtype.itemsize == (160 if scheme == "single" else 320)
    key_views = kviews[1 + nsig:-1]
    assert all(v.strides[0] == pks.dtype.itemsize for v in key_views)
    items = np.zeros(n, CALLER_ITEM)
    items["tag"], items["key"], items["flags"] = np.arange(n, dtype=np.uint64) * np.uint64(2654435761), b["idx"], 0xFFFFFFFF
    assert items["key"].strides[0] == 16
    cols = views[:1 + nsig] + [items["key"], msgs]
    with engine.KeySet.from_mont_cols(scheme, key_views) as ks, \
            engine.KeySet.from_mont_cols(scheme, b["keys"]) as dense:
        assert (ks.key_ok() == 1).all()
        for key, point, window, digit in ((0, 0, 0, 1), (36, len(key_views) - 1, 31, -128), (17, 0, 13, 77)):
            assert (ks.debug_entry(key, point, window, digit) == dense.debug_entry(key, point, window, digit)).all()
        got = ks.verify_mont_cols(cols)
        assert (got == b["want"]).all(), _diff(got, b["want"])
        assert (dense.verify_mont_cols(_cols(scheme, b)) == got).all()
        job = ks.submit_mont_cols(cols)
        assert (job.wait() == b["want"]).all()


# ---- 4. the same set as dsv_keyset_create on the normalised keys ------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_same_set_as_affine_constructor(engine, scheme):
    b = _mont_batch(engine, scheme, 37, 4099)
    keys = [kp.copy() for kp in b["keys"]]
    P0 = b["P0"].copy()
    off = P0[11:12].copy()
    off[0, 32:] = np.frombuffer(M.le32((M.from_le(off[0, 32:]) + 2) % Q), np.uint8)  # off the curve in both sets
    P0[11] = off[0]
    keys[0][11] = _limbs(off, np.random.default_rng(4))[0]
    npts = len(keys)
    with engine.KeySet.from_mont_cols(scheme, keys) as typed, engine.KeySet(scheme, P0, b["P1"]) as affine:
        assert typed.k == affine.k == 37 and typed.nbytes == affine.nbytes
        ok = typed.key_ok()
        assert (ok == affine.key_ok()).all() and ok[11] == 0 and ok.sum() == 36
        rng = np.random.default_rng(8)
        samples = [(0, 0, 0, 1), (36, npts - 1, 31, 128), (36, npts - 1, 31, -128), (5, 0, 31, 127), (11, 0, 3, 9),
                   (9, npts - 1, 0, -1), (20, 0, 16, 0)]
        samples += [(int(rng.integers(37)), int(rng.integers(npts)), int(rng.integers(32)),
                     int(rng.integers(-128, 129))) for _ in range(24)]
        for s in samples:
            assert (typed.debug_entry(*s) == affine.debug_entry(*s)).all(), s


# ---- 5. equality with what exists, at 2^20 items ----------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_two_pow_20_matches_existing_paths(engine, scheme):
    block, times, k = 1 << 16, 16, 37
    n = block * times
    b = _mont_batch(engine, scheme, k, NS[-1])
    want = np.tile(b["want"][:block], times)
    assert 0 < want.sum() < n
    tile = lambda a: _to_dev(a[:block]).repeat(*([times] + [1] * (a.ndim - 1)))
    typed_cols = [tile(c) for c in _cols(scheme, b)]
    with engine.KeySet.from_mont_cols(scheme, b["keys"]) as ks:
        got = _run_dev(engine, ks, typed_cols, n)
        assert (got == want).all(), _diff(got, want)
        # the affine keyed call on the canonical bytes of the same values
        pts = [b["R"]] + ([b["Rp"]] if scheme == "double" else [])
        affine = KC._run_dev(engine, ks, [tile(c) for c in [b["u"]] + pts + [b["idx"], b["m"]]], n)
        assert (affine == got).all(), _diff(affine, got)
    # the unkeyed typed call with the keys gathered per item
    unkeyed = [tile(c) for c in _unkeyed_cols(scheme, b, b["keys"])]
    ok = _poison(n)
    ws = torch.empty(engine.mont_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    getattr(engine, "verify_%s_mont_dev" % scheme)(*unkeyed, ok, ws)
    torch.cuda.synchronize()
    ref = ok.cpu().numpy()
    assert (ref == got).all(), _diff(ref, got)


# ---- 6. the contract --------------------------------------------------------------------------------------
def test_dev_contract(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    n, k = 4099, 37
    b = _mont_batch(engine, "single", k, n)
    du, dR, didx, dm = [_to_dev(c) for c in _cols("single", b)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    fn = L.dsv_verify_keyed_mont_dev
    with engine.KeySet.from_mont_cols("single", b["keys"]) as ks:
        need = engine.keyed_mont_workspace_bytes("single", n)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        # enqueued on a side stream behind a poison fill on that stream
        side = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(side):
            ok = torch.empty(n, dtype=torch.uint8, device=DEV).fill_(POISON)
            ks.verify_mont_dev(du, dR, didx, dm, ok, ws, stream=side)
        side.synchronize()
        assert (ok.cpu().numpy() == b["want"]).all()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        call = lambda h, u, R, Rp, idx, m, nn, okt, wst, wsb: fn(
            h, vp(u), vp(R), vp(Rp), vp(idx), vp(m), ctypes.c_size_t(nn), vp(okt), vp(wst), ctypes.c_size_t(wsb), stream)
        ok = _poison(n)
        assert call(ks._h, du, dR, None, didx, dm, n, ok, ws, need - 1) == -2      # one byte short
        assert b"workspace" in L.dsv_last_error()
        for hole in range(7):                                                       # NULL pointers with n > 0
            if hole == 2:
                continue                                                            # Rp: ignored by a single set
            args = [du, dR, None, didx, dm, ok, ws]
            args[hole] = None
            assert call(ks._h, *args[:5], n, args[5], args[6], need) == -2, hole
        assert call(None, du, dR, None, didx, dm, n, ok, ws, need) == -2
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()                                   # nothing was launched
        # n = 0
        assert call(ks._h, du, dR, None, didx, dm, 0, ok, ws, 0) == 0
        assert call(ks._h, None, None, None, None, None, 0, None, None, 0) == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        # the exact workspace is enough; Rp is ignored by a single set
        assert call(ks._h, du, dR, dR, didx, dm, n, ok, ws, need) == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == b["want"]).all()
        # indices k, k + 1 and 2^32 - 1 on items that verify: verdict 0
        idx = b["idx"].copy()
        rows = np.flatnonzero(b["want"] == 1)[:3]
        idx[rows] = (k, k + 1, (1 << 32) - 1)
        expect = b["want"].copy()
        expect[rows] = 0
        got = _run_dev(engine, ks, [du, dR, _to_dev(idx), dm], n)
        assert (got == expect).all(), _diff(got, expect)
        assert (ks.verify_mont_cols(_cols("single", b, idx=idx)) == expect).all()
        with pytest.raises(ValueError):
            ks.verify_mont_dev(du, dR, didx, dm, ok, ws[:need - 1])
        with pytest.raises(ValueError):
            ks.verify_mont_dev(du, dR, dR, didx, dm, ok, ws)
        with pytest.raises(ValueError):
            ks.verify_mont_dev(du, dR, didx[:-1], dm, ok, ws)
    # a double set without R'
    d = _mont_batch(engine, "double", k, n)
    du, dR, dRp, didx, dm = [_to_dev(c) for c in _cols("double", d)]
    with engine.KeySet.from_mont_cols("double", d["keys"]) as ks:
        need = engine.keyed_mont_workspace_bytes("double", n)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        ok = _poison(n)
        assert call(ks._h, du, dR, None, didx, dm, n, ok, ws, need) == -2
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        assert call(ks._h, du, dR, dRp, didx, dm, n, ok, ws, need) == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == d["want"]).all()


def test_column_checks(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    n = 64
    b = _mont_batch(engine, "double", 37, 4099)
    cols = [np.ascontiguousarray(c[:n]) for c in _cols("double", b)]
    widths = (32, 96, 96, 4, 32)
    ok = np.full(n, POISON, np.uint8)
    okp = ok.ctypes.data_as(ctypes.c_void_p)

    def columns(fix=None):
        arr = (_lib.Column * 5)()
        for c, a in enumerate(cols):
            arr[c].base, arr[c].stride = a.ctypes.data, a.strides[0]
        if fix:
            fix(arr)
        return arr

    with engine.KeySet.from_mont_cols("double", b["keys"]) as ks:
        for c, w in enumerate(widths):
            for what, fix in (("stride", lambda a: setattr(a[c], "stride", w - 1)),
                              ("null", lambda a: setattr(a[c], "base", None))):
                job = ctypes.c_void_p(1)
                for rc in (L.dsv_verify_keyed_mont_cols(ks._h, columns(fix), ctypes.c_size_t(n), okp),
                           L.dsv_verify_keyed_mont_cols_submit(ks._h, columns(fix), ctypes.c_size_t(n), okp,
                                                               ctypes.byref(job))):
                    assert rc == -2 and ("column %d" % c).encode() in L.dsv_last_error(), (c, what)
                assert job.value is None
        # key indices off their alignment: the base, or a stride that is no multiple of 4
        for fix in (lambda a: setattr(a[3], "base", a[3].base + 2), lambda a: setattr(a[3], "stride", 6)):
            assert L.dsv_verify_keyed_mont_cols(ks._h, columns(fix), ctypes.c_size_t(n), okp) == -2
            assert b"column 3" in L.dsv_last_error()
        assert L.dsv_verify_keyed_mont_cols(ks._h, None, ctypes.c_size_t(n), okp) == -2
        assert L.dsv_verify_keyed_mont_cols(ks._h, columns(), ctypes.c_size_t(n), None) == -2
        assert (ok == POISON).all()
        # n = 0 needs no columns
        assert L.dsv_verify_keyed_mont_cols(ks._h, None, ctypes.c_size_t(0), None) == 0
        assert L.dsv_verify_keyed_mont_cols(ks._h, columns(), ctypes.c_size_t(n), okp) == 0
        assert (ok == b["want"][:n]).all()
        h = ctypes.c_void_p(1)
        bad = columns(lambda a: setattr(a[2], "stride", 95))
        assert L.dsv_keyset_create_mont_cols(1, ctypes.byref(bad, ctypes.sizeof(_lib.Column)), ctypes.c_size_t(n),
                                             ctypes.byref(h)) == -2
        assert b"column 1" in L.dsv_last_error() and h.value is None
    with pytest.raises(ValueError):
        engine.KeySet.from_mont_cols("double", b["keys"][:1])
    with engine.KeySet.from_mont_cols("single", [np.zeros((0, 96), np.uint8)]) as empty:
        assert empty.k == 0 and len(empty.key_ok()) == 0
        one = _cols("single", _mont_batch(engine, "single", 37, 4099), rows=slice(0, 5))
        assert (empty.verify_mont_cols(one) == 0).all()


def test_shutdown_kills_the_typed_calls():
    """a process of its own (the session's engine stays up): after dsv_shutdown the device form, the host form and
    a submitted job on a set that was live report DSV_ERR_NOT_INITIALIZED; destroy still succeeds"""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
import mont_cases as MC, pymodel as M
from schnorr_amd import engine as E, _lib
E.init(0)
L = _lib.load()
sk = np.zeros((2, 32), np.uint8); sk[:, 0] = (3, 5)
pk = E.public_keys(sk)
m = np.zeros((2, 32), np.uint8); m[:, 0] = (9, 11)
r = np.zeros((2, 32), np.uint8); r[:, 0] = (21, 23)
u, R = E.sign_single(sk, m, r)
one = np.tile(np.frombuffer(M.le32(1), np.uint8), (2, 1))
limbs = lambda pts: MC.to_limbs_py(np.hstack([pts, one]), M.Q)     # z = 1
ul, ml, Rl, kl = MC.to_limbs_py(u, M.R_ORDER), MC.to_limbs_py(m, M.Q), limbs(R), limbs(pk)
idx = np.arange(2, dtype=np.uint32)
ks = E.KeySet.from_mont_cols("single", [kl])
assert list(ks.key_ok()) == [1, 1]
assert list(ks.verify_mont_cols([ul, Rl, idx, ml])) == [1, 1]
assert list(ks.verify_mont_cols([ul, Rl, idx[::-1].copy(), ml])) == [0, 0]
assert list(ks.submit_mont_cols([ul, Rl, idx, ml]).wait()) == [1, 1]
E.shutdown()
h = ks._h
ok = np.full(2, 7, np.uint8)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
cols = (_lib.Column * 4)()
for c, a in enumerate((ul, Rl, idx, ml)):
    cols[c].base, cols[c].stride = a.ctypes.data, a.strides[0]
assert L.dsv_verify_keyed_mont_cols(h, cols, ctypes.c_size_t(2), p(ok)) == -1
assert L.dsv_verify_keyed_mont_dev(h, p(ul), p(Rl), None, p(idx), p(ml), ctypes.c_size_t(2), p(ok), p(ok),
                                   ctypes.c_size_t(1 << 20), None) == -1
job = ctypes.c_void_p()
rc = L.dsv_verify_keyed_mont_cols_submit(h, cols, ctypes.c_size_t(2), p(ok), ctypes.byref(job))
assert rc == -1 and job.value is None, rc   # nothing is initialised any more: refused at submit
assert (ok == 7).all()
# with another device context up, the dead set's job is accepted and reports at its wait
E.init(0)
rc = L.dsv_verify_keyed_mont_cols_submit(h, cols, ctypes.c_size_t(2), p(ok), ctypes.byref(job))
assert rc == 0 and job.value is not None, rc
assert L.dsv_job_wait(job) == -1
assert b"shut down" in L.dsv_last_error()
assert (ok == 7).all()
assert L.dsv_keyset_destroy(h) == 0
ks._h = ctypes.c_void_p()
E.shutdown()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr


# ---- 7. host form = device form at the host pipeline's edges ----------------------------------------------
HOST_CASES = [(s, n) for s in SCHEMES for n in D.edges("host/mont_cols/%s" % s)]
_HOST = {}
HOST_BLOCK = 4096


def _host_batch(engine, scheme):
    """one honest block of limbs, tiled to the largest host size (sliced for the others), and its key set"""
    if scheme not in _HOST:
        for v in _HOST.values():
            v["ks"].close()
        _HOST.clear()
        nmax, k = max(D.edges("host/mont_cols/%s" % scheme)), 37
        assert nmax <= D.HOST_MAX
        sk, gen, P0, P1 = KC._keys(engine, scheme, k, 777)
        rng = np.random.default_rng(20261017)
        idx = rng.integers(0, k, size=HOST_BLOCK).astype(np.uint32)
        m = KC._scalars(rng, HOST_BLOCK, 0x3F)
        r = KC._scalars(rng, HOST_BLOCK, 0x07)
        Rp = None
        if scheme == "single":
            u, R = engine.sign_single(sk[idx], m, r)
        elif scheme == "double":
            u, R, Rp = engine.sign_double(sk[idx], m, r)
        else:
            u, R = engine.sign_vargen(sk[idx], gen[idx], m, r)
        times = -(-nmax // HOST_BLOCK)
        tile = lambda a: np.ascontiguousarray(np.tile(a, (times,) + (1,) * (a.ndim - 1))[:nmax])
        pts = [tile(_limbs(R, rng))] + ([tile(_limbs(Rp, rng))] if Rp is not None else [])
        keys = [_limbs(P0, rng)] + ([_limbs(P1, rng)] if P1 is not None else [])
        _HOST[scheme] = {"cols": [tile(MC.to_limbs_py(u, R_ORDER))] + pts + [tile(idx), tile(MC.to_limbs_py(m, Q))],
                         "ks": engine.KeySet.from_mont_cols(scheme, keys)}
    return _HOST[scheme]


@pytest.mark.parametrize("scheme,n", HOST_CASES, ids=["%s-%d" % c for c in HOST_CASES])
def test_host_form_equals_dev_form_at_every_edge(engine, scheme, n):
    b = _host_batch(engine, scheme)
    cols = [c[:n] for c in b["cols"]]
    cols[0] = cols[0].copy()
    # a wrong item at the first item of every sub-batch, whichever plan the call takes
    pos = sorted(set(D.host_parts(n, False)) | set(D.host_parts(n, True)))
    assert pos[0] == 0 and pos[-1] < n
    cols[0][pos, 0] ^= 1  # another u (limbs: u +- 2^-256 mod r)
    dev = _mont_dev(engine, b["ks"], cols)
    # every item of the batch is honest, so the device form's zeros are exactly the planted ones
    assert np.array_equal(np.flatnonzero(dev == 0), np.array(pos)), (np.flatnonzero(dev == 0)[:8], pos[:8])
    host = b["ks"].verify_mont_cols(cols)
    assert np.array_equal(host, dev), _diff(host, dev)


# ---- 8. jobs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_two_jobs_and_a_blocking_call(engine, scheme):
    b = _host_batch(engine, scheme)
    cols = list(b["cols"])
    n = len(cols[0])
    cols[0] = cols[0].copy()
    cols[0][::11, 0] ^= 1
    dev = _mont_dev(engine, b["ks"], cols)
    assert 0 < dev.sum() < n
    los = (0, 12345, 777)
    out, err = [None], []

    def work():
        try:
            out[0] = b["ks"].verify_mont_cols([c[los[2]:] for c in cols])
        except Exception as e:  # noqa: BLE001
            err.append(e)

    jobs = [b["ks"].submit_mont_cols([c[lo:] for c in cols]) for lo in los[:2]]
    th = threading.Thread(target=work)
    th.start()
    got = [j.wait() for j in jobs]
    th.join()
    assert not err, err
    for lo, g in zip(los, got + out):
        assert np.array_equal(g, dev[lo:]), (lo, _diff(g, dev[lo:]))
    assert all(j.done() for j in jobs)


def test_destroy_waits_for_a_running_job(engine):
    from schnorr_amd import _lib

    b = _host_batch(engine, "double")
    cols = b["cols"]
    dev = _mont_dev(engine, b["ks"], cols)
    ks = b["ks"]
    job = ks.submit_mont_cols(cols)
    raw = job._job
    ks.close()  # dsv_keyset_destroy: returns only after the job that holds the set
    assert _lib.load().dsv_job_done(raw) == 1
    got = job.wait()
    assert np.array_equal(got, dev), _diff(got, dev)
    with pytest.raises(ValueError):
        ks.verify_mont_cols(cols)
    _HOST.clear()
