"""The key cache for typed objects on the GPU (dsv_verify_keyed_open_mont_*; KeySet.verify_open_mont_dev /
verify_open_mont_cols / submit_open_mont_cols): the open-set verify over exactly the arguments of
the reference's verify_batch — Montgomery limbs, projective points.  Every expectation comes from the oracle's typed
verify on the item's own limbs (oracle_lib.verify_*_mont), which knows nothing of key sets.  Whole vectors are
compared: the verdicts, the workspace's index column (against KeySet.lookup on the keys' normal form, which the
tests know by construction and re-derive from the limbs with Python integers) and the miss count."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dispatch_edges as D
import mont_cases as MC
import pymodel as M
import torsion_model as TM
from keyed_cases import (FRONT_N, NKEY, NS, NSIG, REG, SCHEMES, _diff, _limbs, _mixture, _open_mont_ws,
                         _oracle_mont_cols, _plants, _poison, _pool, _pool_keyset, _scalars, _sign_items, _to_dev)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
NONE = 0xFFFFFFFF
INVALID = -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (0, 1, 64)
Q, R_ORDER = M.Q, M.R_ORDER
R_INV = pow(1 << 256, -1, Q)


def _limbs_z1(points):
    one = np.tile(np.frombuffer(M.le32(1), np.uint8), (len(points), 1))
    return MC.to_limbs_py(np.hstack([points, one]), Q)


def _normal_form(limbs):
    """limbs [n, 96] -> canonical affine bytes [n, 64], Python integers (z != 0, every group < q)"""
    out = np.zeros((len(limbs), 64), np.uint8)
    for i, row in enumerate(limbs):
        u, v, z = [M.from_le(row[32 * j:32 * j + 32]) * R_INV % Q for j in range(3)]
        zi = pow(z, -1, Q)
        out[i] = np.frombuffer(M.le32(u * zi % Q) + M.le32(v * zi % Q), np.uint8)
    return out


def _open_dev(engine, ks, cols, stream=None):
    """-> (verdicts, the workspace's index column, misses)"""
    n = len(cols[0])
    ok, ws = _poison(n), _open_mont_ws(engine, ks.scheme, n)
    misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
    ks.verify_open_mont_dev(*[_to_dev(c) for c in cols], ok, ws, misses=misses, stream=stream)
    torch.cuda.synchronize()
    idx = ws[:4 * n].cpu().numpy().view(np.uint32).copy()
    return ok.cpu().numpy(), idx, int(misses.item()) & 0xFFFFFFFF


def _expect_idx(ks, affine):
    return ks.lookup(*affine)[0] if ks.k else np.full(len(affine[0]), NONE, np.uint32)


def _check(engine, ks, cols, affine, want, what):
    got, idx, nmiss = _open_dev(engine, ks, cols)
    where = _expect_idx(ks, affine)
    assert (got == want).all(), (what, _diff(got, want))
    assert (idx == where).all(), (what, _diff(idx, where))
    assert nmiss == int((where == NONE).sum()), (what, nmiss)
    return where


# ---- 1. parity with the oracle: sizes x set sizes ------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_parity(engine, scheme, k):
    b = _mixture(engine, scheme, k, NS[-1])
    assert 0 < b["want"].sum() < NS[-1]
    sample = slice(0, 40)
    assert all((_normal_form(c[sample]) == a[sample]).all()
               for c, a in zip(b["cols"][1 + NSIG[scheme]:-1], b["affine"]))
    with _pool_keyset(engine, scheme, k) as ks:
        for n in NS:
            where = _check(engine, ks, [c[:n] for c in b["cols"]], [a[:n] for a in b["affine"]], b["want"][:n],
                           (scheme, k, n))
            if k and n >= 4099:
                hits = where != NONE
                assert 0 < b["want"][:n][hits].sum() < hits.sum() and 0 < b["want"][:n][~hits].sum() < (~hits).sum()
            if k == 0:
                assert (where == NONE).all()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_equals_the_unkeyed_typed_call(engine, scheme):
    n = 4099
    b = _mixture(engine, scheme, 64, NS[-1])
    cols = [c[:n] for c in b["cols"]]
    ok = _poison(n)
    ws = torch.empty(engine.mont_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    getattr(engine, "verify_%s_mont_dev" % scheme)(*[_to_dev(c) for c in cols], ok, ws)
    torch.cuda.synchronize()
    with _pool_keyset(engine, scheme, 64) as ks:
        got = _open_dev(engine, ks, cols)[0]
    assert (got == ok.cpu().numpy()).all(), _diff(got, ok.cpu().numpy())


@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_sixteen_items_per_lane(engine, scheme):
    """2^19 + 5 items (a lane shares its inversion among 16, the last lane is ragged), tiled on the device from one
    block the way the 2^20 typed case tiles its own: equal to dsv_verify_*_mont_dev everywhere, to the oracle on
    the block"""
    block, n = 1 << 15, (1 << 19) + 5
    b = _mixture(engine, scheme, 64, NS[-1])
    times = -(-n // block)
    tile = lambda a: _to_dev(a[:block]).repeat(*([times] + [1] * (a.ndim - 1)))[:n].contiguous()
    dcols = [tile(c) for c in b["cols"]]
    ok, ref = _poison(n), _poison(n)
    misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
    with _pool_keyset(engine, scheme, 64) as ks:
        ks.verify_open_mont_dev(*dcols, ok, _open_mont_ws(engine, scheme, n), misses=misses)
        where = _expect_idx(ks, [a[:block] for a in b["affine"]])
    ws = torch.empty(engine.mont_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    getattr(engine, "verify_%s_mont_dev" % scheme)(*dcols, ref, ws)
    torch.cuda.synchronize()
    got = ok.cpu().numpy()
    assert (got == ref.cpu().numpy()).all(), _diff(got, ref.cpu().numpy())
    assert (got[-5:] == b["want"][:5]).all()                      # the ragged tail: items 0 .. 4 of the block again
    assert (got[:block] == b["want"][:block]).all(), _diff(got[:block], b["want"][:block])
    assert int(misses.item()) == int((np.tile(where == NONE, times)[:n]).sum())


# ---- 2. representations of one registered key ----------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_one_key_in_every_representation(engine, scheme):
    """a set registered from typed objects (random z): key 5 presented with z = 1, with a random z and as the very
    limbs it was registered from gets index 5 every time; a key registered three times gets its lowest index"""
    sk, gen, P0, P1 = _pool(engine, scheme)
    rng = np.random.default_rng(31)
    dup = np.array(list(range(16)) + [3, 3, 9])                  # keys 16, 17 repeat key 3; 18 repeats 9
    A = [np.ascontiguousarray(P[dup]) for P in ([P0] + ([P1] if P1 is not None else []))]
    reg = [_limbs(a, rng) for a in A]
    n = 96
    j = np.array([5, 3, 9] * (n // 3))
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, Rp = _sign_items(engine, scheme, sk[j], gen[j] if gen is not None else None, m, r)
    u[::5, 0] ^= 4
    pts = [R] + ([Rp] if Rp is not None else [])
    keys = []
    for a, regl in zip(A, reg):
        kl = _limbs(a[j], rng)                                   # a random z
        kl[0::6] = _limbs_z1(a[j])[0::6]                         # z = 1
        kl[1::6], kl[2::6], kl[5::6] = regl[j][1::6], regl[j][2::6], regl[j][5::6]  # the registered limbs
        keys.append(kl)
    cols = [MC.to_limbs_py(u, R_ORDER)] + [_limbs(p, rng) for p in pts] + keys + [MC.to_limbs_py(m, Q)]
    want = _oracle_mont_cols(scheme, cols)
    assert (want == (np.arange(n) % 5 != 0)).all()
    with engine.KeySet.from_mont_cols(scheme, reg) as ks:
        got, idx, nmiss = _open_dev(engine, ks, cols)
    assert (got == want).all(), _diff(got, want)
    assert (idx == j).all() and nmiss == 0, idx[:12]


# ---- 3. limbs and z the Rust types cannot hold, in hits and in misses ----------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_unholdable_limbs_give_zero(engine, scheme):
    """each class in turn, planted in a hit and in a miss that verify otherwise, twice at lane distance (the two
    items share one inversion): verdict 0 there, every other item of the lanes as before"""
    n = NS[-1]
    lanes = -(-n // 8)
    b = _mixture(engine, scheme, 64, n)
    nk = NKEY[scheme]
    with _pool_keyset(engine, scheme, 64) as ks:
        where = _expect_idx(ks, b["affine"])
        good = b["want"][:lanes] & b["want"][lanes:2 * lanes]
        hit = np.flatnonzero(good & (where[:lanes] != NONE) & (where[lanes:2 * lanes] != NONE))
        miss = np.flatnonzero(good & (where[:lanes] == NONE) & (where[lanes:2 * lanes] == NONE))
        assert len(hit) > 4 and len(miss) > 4
        for t, (name, c, span, value) in enumerate(_plants(scheme)):
            rows = [hit[t % len(hit)], hit[t % len(hit)] + lanes, miss[t % len(miss)], miss[t % len(miss)] + lanes]
            cols = [x.copy() for x in b["cols"]]
            cols[c][rows, span] = value
            want = b["want"].copy()
            sub = sorted(set(rows) | {x + 1 for x in rows} | {x - 1 for x in rows if x})
            want[sub] = _oracle_mont_cols(scheme, [x[sub] for x in cols])   # (verdicts are per item)
            expect = b["want"].copy()
            expect[rows] = 0
            assert (want == expect).all(), name
            got, idx, nmiss = _open_dev(engine, ks, cols)
            assert (got == want).all(), (name, _diff(got, want))
            key_plant = name.startswith("key")
            expect_idx = where.copy()
            if key_plant:
                expect_idx[rows] = NONE                          # unusable key limbs: a miss
            assert (idx == expect_idx).all(), (name, _diff(idx, expect_idx))
            assert nmiss == int((expect_idx == NONE).sum()), name
    assert nk in (1, 2)


# ---- 4. registered, and still not a hit -----------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_registered_but_not_a_hit(engine, scheme):
    """a set that registered an off-curve key and a z = 0 key (items present those very limbs), and a registered
    PK beside another registered key's second point: every one a miss, with the oracle's verdict"""
    sk, gen, P0, P1 = _pool(engine, scheme)
    rng = np.random.default_rng(41)
    k, n = 16, 128
    A = [np.ascontiguousarray(P[:k]) for P in ([P0] + ([P1] if P1 is not None else []))]
    off = A[0][11:12].copy()
    off[0, :32] = np.frombuffer(M.le32((M.from_le(off[0, :32]) + 1) % Q), np.uint8)
    reg = [_limbs(a, rng) for a in A]
    reg[0][11] = _limbs(off, rng)[0]                             # off the curve
    reg[-1][13, 64:96] = 0                                       # z = 0
    j = rng.integers(0, k, size=n)
    j[:8] = (11, 13, 11, 13, 2, 4, 2, 4)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, Rp = _sign_items(engine, scheme, sk[j], gen[j] if gen is not None else None, m, r)
    pts = [R] + ([Rp] if Rp is not None else [])
    keys = [_limbs(a[j], rng) for a in A]
    affine = [a[j].copy() for a in A]
    for i in range(4):                                           # the registered limbs themselves
        for kl, regl in zip(keys, reg):
            kl[i] = regl[j[i]]
    affine[0][[0, 2]] = off[0]
    mixed = []
    if len(A) == 2:                                              # PK of key 2 beside the second point of key 4
        keys[1][[4, 6]] = _limbs(A[1][[4, 4]], rng)
        affine[1][[4, 6]] = A[1][4]
        mixed = [4, 6]
    cols = [MC.to_limbs_py(u, R_ORDER)] + [_limbs(p, rng) for p in pts] + keys + [MC.to_limbs_py(m, Q)]
    want = _oracle_mont_cols(scheme, cols)
    assert (want[[0, 1, 2, 3] + mixed] == 0).all() and want[8:].all()
    with engine.KeySet.from_mont_cols(scheme, reg) as ks:
        ok = ks.key_ok()
        assert ok[11] == 0 and ok[13] == 0 and ok.sum() == k - 2
        got, idx, nmiss = _open_dev(engine, ks, cols)
    assert (got == want).all(), _diff(got, want)
    expect = j.astype(np.uint32)
    expect[mixed] = NONE
    expect[np.isin(j, (11, 13))] = NONE                          # whatever limbs present them: not registered as valid
    assert (idx == expect).all(), _diff(idx, expect)
    assert nmiss == int((expect == NONE).sum()) > 4 + len(mixed)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_small_order_keys_hit(engine, scheme):
    """the identity and a point of order 8 are valid keys: items under them hit and get the oracle's verdict"""
    sk, gen, P0, P1 = _pool(engine, scheme)
    rng = np.random.default_rng(43)
    ident = np.frombuffer(M.le32(0) + M.le32(1), np.uint8)
    small = np.frombuffer(M.point_bytes(TM.order8_point()), np.uint8)
    k, n = 8, 64
    A = [np.ascontiguousarray(P[:k]).copy() for P in ([P0] + ([P1] if P1 is not None else []))]
    A[0][1], A[0][2] = ident, small
    j = rng.integers(0, k, size=n)
    j[:16] = [1, 2] * 8
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, Rp = _sign_items(engine, scheme, sk[j], gen[j] if gen is not None else None, m, r)
    if scheme != "double":  # under the identity as PK, u*G == R verifies for R = u*G: sign with sk = 0
        z = np.zeros_like(sk[j[:16:2]])
        u[:16:2], R[:16:2] = _sign_items(engine, scheme, z, gen[j[:16:2]] if gen is not None else None, m[:16:2],
                                         r[:16:2])[:2]
    pts = [R] + ([Rp] if Rp is not None else [])
    cols = [MC.to_limbs_py(u, R_ORDER)] + [_limbs(p, rng) for p in pts] + [_limbs(a[j], rng) for a in A] + \
        [MC.to_limbs_py(m, Q)]
    want = _oracle_mont_cols(scheme, cols)
    assert 0 < want.sum() < n
    with engine.KeySet(scheme, *A) as ks:
        assert (ks.key_ok() == 1).all()
        got, idx, nmiss = _open_dev(engine, ks, cols)
    assert (got == want).all(), _diff(got, want)
    assert (idx == j).all() and nmiss == 0


# ---- 5. the _dev contract --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_dev_contract(engine, scheme):
    from schnorr_amd import _lib

    L = _lib.load()
    n = 65
    b = _mixture(engine, scheme, 64, NS[-1])
    cols = [c[:n] for c in b["cols"]]
    d = [_to_dev(c) for c in cols]
    ns, nk = NSIG[scheme], NKEY[scheme]
    vp, sz, null = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p(None)
    p = lambda t: vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    need = engine.keyed_open_mont_workspace_bytes(scheme, n)
    ws = _open_mont_ws(engine, scheme, n)
    base = {"u": p(d[0]), "R": p(d[1]), "Rp": p(d[2]) if ns == 2 else null, "ka": p(d[1 + ns]),
            "kb": p(d[2 + ns]) if nk == 2 else null, "m": p(d[-1]), "ws": p(ws)}
    ks = _pool_keyset(engine, scheme, 64)
    try:
        def verify(h, nn, okt, wsb, **over):
            a = dict(base, **over)
            return L.dsv_verify_keyed_open_mont_dev(h, a["u"], a["R"], a["Rp"], a["ka"], a["kb"], a["m"], sz(nn),
                                                    p(okt) if okt is not None else null, a["ws"], sz(wsb), stream, null)

        ok = _poison(n)
        assert verify(ks._h, n, ok, need - 1) == INVALID
        assert b"workspace" in L.dsv_last_error()
        for hole in base:
            if base[hole].value is None:
                continue                                         # a pointer this scheme ignores
            assert verify(ks._h, n, ok, need, **{hole: null}) == INVALID, hole
            assert b"null" in L.dsv_last_error(), hole
        assert verify(ks._h, n, None, need) == INVALID
        assert verify(None, n, ok, need) == INVALID
        for hole in base:                                        # every input column 8 bytes off a 16-byte boundary
            if hole == "ws" or base[hole].value is None:
                continue
            odd = torch.zeros(n * 96 + 8, dtype=torch.uint8, device=DEV)[8:]
            assert verify(ks._h, n, ok, need, **{hole: p(odd)}) == INVALID, hole
            assert b"aligned" in L.dsv_last_error()
        other = [s for s in SCHEMES if s != scheme and (NSIG[s], NKEY[s]) != (ns, nk)]
        for s in other:                                          # the column count of another scheme
            with pytest.raises(ValueError):
                ks.verify_open_mont_dev(*[_to_dev(c[:n]) for c in _mixture(engine, s, 64, NS[-1])["cols"]], ok, ws)
        with pytest.raises(ValueError):
            ks.verify_open_mont_dev(*d, ok, ws[:need - 1])
        assert verify(ks._h, 0, ok, 0) == 0
        hm = sz(55)
        assert L.dsv_verify_keyed_open_mont_cols(ks._h, null, sz(0), null, ctypes.byref(hm)) == 0 and hm.value == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all() and (ws.cpu().numpy() == 0xA5).all()
        assert verify(ks._h, n, ok, need) == 0, L.dsv_last_error().decode()
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == b["want"][:n]).all()
    finally:
        ks.close()
    with pytest.raises(ValueError):
        ks.verify_open_mont_cols(cols)


# ---- 6. capture and replay -------------------------------------------------------------------------------------
def test_open_mont_capture_and_replay(engine):
    """one captured call, replayed over inputs overwritten in place with no, some and only misses: the list's
    length and the miss count live on the device, so every replay is exact"""
    scheme, n, k = "double", 4099, 8
    sk, gen, P0, P1 = _pool(engine, scheme)
    rng = np.random.default_rng(6)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    base = rng.integers(0, k, size=n)
    batches = []
    for miss in (np.zeros(n, bool), rng.integers(0, 8, size=n) == 0, np.ones(n, bool)):
        j = base + REG * miss
        u, R, Rp = engine.sign_double(sk[j], m, r)
        u[rng.integers(0, 16, size=n) == 0, 0] ^= 8
        cols = [MC.to_limbs_py(u, R_ORDER)] + [_limbs(x, rng) for x in (R, Rp, P0[j], P1[j])] + [MC.to_limbs_py(m, Q)]
        want = _oracle_mont_cols(scheme, cols)
        assert 0 < want.sum() < n
        batches.append((cols, want, int(miss.sum())))
    with _pool_keyset(engine, scheme, k) as ks:
        d = [_to_dev(c) for c in batches[-1][0]]
        ok, ws = _poison(n), _open_mont_ws(engine, scheme, n)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.verify_open_mont_dev(*d, ok, ws, misses=misses)
        torch.cuda.synchronize()
        for cols, want, nmiss in batches:
            for t, c in zip(d, cols):
                t.copy_(_to_dev(c))
            ok.fill_(POISON)
            misses.fill_(999)
            ws.fill_(0xA5)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = ok.cpu().numpy()
            assert (got == want).all(), (nmiss, _diff(got, want))
            assert int(misses.item()) == nmiss
        del g


@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_captured_call_keeps_its_k_and_sees_replaced_keys(engine, scheme):
    """captured when the set held 8 of the batch's 16 keys and replayed after the other 8 were appended: their
    items still take the miss path (verdicts unchanged, misses as at capture).  After key 3 is replaced by an
    unregistered key, a new call misses on key 3's old limbs and hits on the new key's"""
    k0, n = 8, 300
    sk, gen, P0, P1 = _pool(engine, scheme)
    rng = np.random.default_rng(89)
    j = rng.integers(0, 16, size=n)
    j[:16] = rng.permutation(16)
    j[16:24] = REG + 1                                            # the key that will replace key 3
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, Rp = _sign_items(engine, scheme, sk[j], gen[j] if gen is not None else None, m, r)
    u[::8, 0] ^= 8
    pts = [R] + ([Rp] if Rp is not None else [])
    A = [P0] + ([P1] if P1 is not None else [])
    cols = [MC.to_limbs_py(u, R_ORDER)] + [_limbs(x, rng) for x in pts + [a[j] for a in A]] + [MC.to_limbs_py(m, Q)]
    want = _oracle_mont_cols(scheme, cols)
    assert (want == (np.arange(n) % 8 != 0)).all()
    newer = j >= k0
    sl = lambda P, lo, hi: np.ascontiguousarray(P[lo:hi]) if P is not None else None
    d = [_to_dev(c) for c in cols]
    with engine.KeySet.reserved(scheme, 16, sl(P0, 0, k0), sl(P1, 0, k0)) as ks:
        ok, ws = _poison(n), _open_mont_ws(engine, scheme, n)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.verify_open_mont_dev(*d, ok, ws, misses=misses)
        torch.cuda.synchronize()

        def replay(what):
            ok.fill_(POISON)
            misses.fill_(999)
            ws.fill_(0xA5)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = ok.cpu().numpy()
            assert (got == want).all(), (what, _diff(got, want))
            assert int(misses.item()) == int(newer.sum()), what

        replay("before the append")
        assert ks.append(sl(P0, k0, 16), *([sl(P1, k0, 16)] if P1 is not None else [])) == k0
        replay("after the append")
        del g
        got, idx, nmiss = _open_dev(engine, ks, cols)
        assert (got == want).all() and nmiss == 8 and (idx[j < 16] == j[j < 16]).all()
        ks.replace([3], sl(P0, REG + 1, REG + 2), *([sl(P1, REG + 1, REG + 2)] if P1 is not None else []))
        got, idx, nmiss = _open_dev(engine, ks, cols)
        assert (got == want).all(), _diff(got, want)
        expect = j.astype(np.uint32)
        expect[j == 3] = NONE
        expect[j == REG + 1] = 3
        assert (idx == expect).all() and nmiss == int((j == 3).sum())


# ---- 7. the two-launch front gives the same outputs ------------------------------------------------------------
def test_open_mont_two_launch_front_in_a_subprocess(engine):
    """DSV_OPEN_MONT_FUSED=0 and =1 in processes of their own (side by side): the index column, valid, misses and
    ok of the two-launch front (k_normalize_uvz over all points, then k_index_lookup) equal the fused kernel's,
    device form (1, 8 items per lane) and host form (4 per lane).  The same processes then shut the engine down
    under a live set: every call of the family reports DSV_ERR_NOT_INITIALIZED and touches nothing."""
    code = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
from schnorr_amd import engine as E, _lib
import keyed_cases as T
E.init(0)
out = {}
up = lambda x: (x + 255) // 256 * 256
for scheme in T.SCHEMES:
    b = T._mixture(E, scheme, 64, T.FRONT_N)
    big = [np.ascontiguousarray(np.tile(c, (8, 1))[:T.NS[-1]]) for c in b["cols"]]
    # unusable key limbs whose normalised bytes ARE a registered key's: the Montgomery form of key 0's affine
    # coordinates with z = 0 (the normalisation puts 1 in place of an unusable z) — a miss on both paths; and the
    # planted classes of the limb tests in the first rows
    ns, nk = T.NSIG[scheme], T.NKEY[scheme]
    _, _, P0, P1 = T._pool(E, scheme)
    for c, P in zip(range(1 + ns, 1 + ns + nk), (P0, P1)):
        z0 = np.hstack([P[:1], np.zeros((1, 32), np.uint8)])
        big[c][[5, 4100, 9000]] = T.MC.to_limbs_py(z0, T.Q)[0]
    for row, (name, c, span, value) in enumerate(T._plants(scheme)):
        big[c][20 + row, span] = value
    for k in (0, 64):
        with T._pool_keyset(E, scheme, k) as ks:
            for n in (65, T.FRONT_N, T.NS[-1]):
                cols = [c[:n] for c in big]
                ok, ws = T._poison(n), T._open_mont_ws(E, scheme, n)
                misses = torch.full((1,), 999, dtype=torch.int32, device=T.DEV)
                ks.verify_open_mont_dev(*[T._to_dev(c) for c in cols], ok, ws, misses=misses)
                torch.cuda.synchronize()
                w = ws.cpu().numpy()
                total = E.keyed_open_mont_workspace_bytes(scheme, n)
                voff = total - up(n)   # the challenge hash's valid (the front's ANDed in): the workspace's last part
                # the front's own valid column: in front of its prefix products and the keyed workspace
                foff = total - E.keyed_workspace_bytes(n) - up((ns + nk) * (n + 32) * 36) - up(n)
                if k == 64 and n > 5:
                    assert (w[:4 * n].view(np.uint32)[5] == T.NONE) and w[foff + 5] == 0, (scheme, n)
                out["%%s/%%d/%%d" %% (scheme, k, n)] = np.concatenate(
                    [ok.cpu().numpy(), w[:4 * n], w[voff:voff + n], w[foff:foff + n],
                     np.frombuffer(int(misses.item()).to_bytes(4, "little", signed=True), np.uint8)])
            host, hm = ks.verify_open_mont_cols(big)
            out["%%s/%%d/host" %% (scheme, k)] = np.concatenate([host, np.frombuffer(hm.to_bytes(4, "little"), np.uint8)])
np.savez(sys.argv[1], **out)
# a dead set: its device was shut down under it
L = _lib.load()
ks = T._pool_keyset(E, "single", 8)
h = ctypes.c_void_p(ks._h.value)
E.shutdown()
okh = np.full(4, 7, np.uint8)
cols4 = (_lib.Column * 4)()
for c, a in enumerate(T._mixture(E, "single", 64, T.FRONT_N)["cols"]):
    cols4[c].base, cols4[c].stride = a.ctypes.data, a.strides[0]
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
sz = ctypes.c_size_t
assert L.dsv_verify_keyed_open_mont_cols(h, cols4, sz(4), p(okh), None) == -1
assert L.dsv_verify_keyed_open_mont_dev(h, p(okh), p(okh), None, p(okh), None, p(okh), sz(4), p(okh), p(okh), sz(1 << 24),
                                        None, None) == -1
job = ctypes.c_void_p()
assert L.dsv_verify_keyed_open_mont_cols_submit(h, cols4, sz(4), p(okh), ctypes.byref(job)) == -1 and job.value is None
assert (okh == 7).all()
ks._h = ctypes.c_void_p()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    import tempfile

    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        runs = {}
        for fused in ("1", "0"):
            env = dict(os.environ, DSV_OPEN_MONT_FUSED=fused)
            runs[fused] = subprocess.Popen([sys.executable, "-c", code, os.path.join(tmp, "front%s.npz" % fused)],
                                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        for fused, run in runs.items():
            text = run.communicate(timeout=600)[0]
            assert run.returncode == 0 and text.strip().endswith("ok"), text
            got[fused] = dict(np.load(os.path.join(tmp, "front%s.npz" % fused)))
    assert sorted(got["0"]) == sorted(got["1"]) and len(got["1"]) == 24
    for key in got["1"]:
        assert (got["0"][key] == got["1"][key]).all(), (key, _diff(got["0"][key], got["1"][key]))
    b = _mixture(engine, "double", 64, FRONT_N)
    clean = np.ones(FRONT_N, bool)
    clean[[5] + list(range(20, 20 + len(_plants("double"))))] = False  # the rows planted above
    assert (got["1"]["double/64/%d" % FRONT_N][:FRONT_N][clean] == b["want"][clean]).all()
    assert (got["1"]["double/64/%d" % FRONT_N][:FRONT_N][~clean] == 0).all()
    assert (got["1"]["double/64/host"][:FRONT_N][clean] == b["want"][clean]).all()


# ---- 8. the host form ------------------------------------------------------------------------------------------
HOST_CASES = [(s, n) for s in SCHEMES for n in D.edges("host/mont_cols/%s" % s)]
_HOST = {}
HOST_BLOCK = 4096


def _host_batch(engine, scheme):
    """one mixture block as records laid out like the Rust structs (strides larger than the widths), tiled to
    the largest host size, and its key set"""
    if scheme not in _HOST:
        for v in _HOST.values():
            v["ks"].close()
        _HOST.clear()
        nmax = max(D.edges("host/mont_cols/%s" % scheme))
        assert nmax <= D.HOST_MAX
        b = _mixture(engine, scheme, 64, NS[-1])
        times = -(-nmax // HOST_BLOCK)
        tile = lambda a: np.ascontiguousarray(np.tile(a[:HOST_BLOCK], (times,) + (1,) * (a.ndim - 1))[:nmax])
        sigs, pks, msgs, views = MC.as_records(scheme, [tile(c) for c in b["cols"]])
        assert views[1].strides[0] == sigs.dtype.itemsize > 96 and views[1 + NSIG[scheme]].strides[0] >= 160
        ks = _pool_keyset(engine, scheme, 64)
        miss = _expect_idx(ks, [a[:HOST_BLOCK] for a in b["affine"]]) == NONE
        _HOST[scheme] = {"views": views, "hold": (sigs, pks, msgs), "ks": ks, "miss": tile(miss),
                         "want": tile(b["want"])}
    return _HOST[scheme]


@pytest.mark.parametrize("scheme,n", HOST_CASES, ids=["%s-%d" % c for c in HOST_CASES])
def test_open_mont_host_form_at_every_edge(engine, scheme, n):
    b = _host_batch(engine, scheme)
    host, nmiss = b["ks"].verify_open_mont_cols([v[:n] for v in b["views"]])
    assert np.array_equal(host, b["want"][:n]), _diff(host, b["want"][:n])
    assert nmiss == int(b["miss"][:n].sum())


def test_open_mont_column_checks(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    n = 64
    b = _host_batch(engine, "double")
    widths = (32, 96, 96, 96, 96, 32)
    ok = np.full(n, POISON, np.uint8)
    okp = ok.ctypes.data_as(ctypes.c_void_p)
    sz = ctypes.c_size_t

    def columns(fix=None, count=6):
        arr = (_lib.Column * 6)()
        for c, a in enumerate(b["views"][:count]):
            arr[c].base, arr[c].stride = a.ctypes.data, a.strides[0]
        if fix:
            fix(arr)
        return arr

    ks = b["ks"]
    for c, w in enumerate(widths):
        for what, fix in (("stride", lambda a: setattr(a[c], "stride", w - 1)),
                          ("null", lambda a: setattr(a[c], "base", None))):
            job = ctypes.c_void_p(1)
            for rc in (L.dsv_verify_keyed_open_mont_cols(ks._h, columns(fix), sz(n), okp, None),
                       L.dsv_verify_keyed_open_mont_cols_submit(ks._h, columns(fix), sz(n), okp, ctypes.byref(job))):
                assert rc == INVALID and ("column %d" % c).encode() in L.dsv_last_error(), (c, what)
            assert job.value is None
    assert L.dsv_verify_keyed_open_mont_cols(ks._h, None, sz(n), okp, None) == INVALID
    assert L.dsv_verify_keyed_open_mont_cols(ks._h, columns(), sz(n), None, None) == INVALID
    assert L.dsv_verify_keyed_open_mont_cols(None, columns(), sz(n), okp, None) == INVALID
    assert (ok == POISON).all()
    with pytest.raises(ValueError):
        ks.verify_open_mont_cols(b["views"][:5])                  # a var-generator batch's column count
    assert L.dsv_verify_keyed_open_mont_cols(ks._h, columns(), sz(n), okp, None) == 0
    assert (ok == b["want"][:n]).all()


# ---- 9. jobs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_mont_two_jobs_in_flight(engine, scheme):
    b = _host_batch(engine, scheme)
    los = (0, 12345)
    jobs = [b["ks"].submit_open_mont_cols([v[lo:] for v in b["views"]]) for lo in los]
    got = [j.wait() for j in jobs]
    for lo, g in zip(los, got):
        blocking = b["ks"].verify_open_mont_cols([v[lo:] for v in b["views"]])[0]
        assert np.array_equal(g, blocking), (lo, _diff(g, blocking))
        assert np.array_equal(g, b["want"][lo:]), (lo, _diff(g, b["want"][lo:]))
    assert all(j.done() for j in jobs)


def test_open_mont_destroy_waits_for_a_running_job(engine):
    from schnorr_amd import _lib

    b = _host_batch(engine, "vargen")
    ks = b["ks"]
    job = ks.submit_open_mont_cols(b["views"])
    raw = job._job
    ks.close()  # dsv_keyset_destroy: returns only after the job that holds the set
    assert _lib.load().dsv_job_done(raw) == 1
    got = job.wait()
    assert np.array_equal(got, b["want"]), _diff(got, b["want"])
    with pytest.raises(ValueError):
        ks.verify_open_mont_cols(b["views"])
    _HOST.clear()
