"""The key cache for serialized records on the GPU (dsv_keyset_lookup_wire*, dsv_verify_*_keyed_open_wire*): the
wire index of a key set and the open-set verify by compressed key.  The expected verdict is always the CPU
oracle's on the records themselves, O.verify_<scheme>_wire(sig, pk, m) — registering a key never changes it — and
`misses` is the count of a Python dict over O.compress of the keys with key_ok == 1.  Keys and items come from
tests/keyed_cases.py."""
import ctypes

import numpy as np
import pytest
import torch

import edge_sets as ES
import harness as H
import mont_cases as MC
import oracle_lib as O
import pymodel as M
from keyed_cases import (_diff, _enc, _expect_rec, _key_records, _keys, _lookup_dev, _non_squares, _oracle_wire, _poison,
                         _scalars, _sig, _to_dev, _value_batch, _where_rec)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
NONE = 0xFFFFFFFF
INVALID = -2
SCHEMES = ("single", "double", "vargen")
Q = M.Q


# ---- the model: a dict over the canonical records of the valid registered keys, lowest index first ----------
def _where_of_records(records, key_ok):
    """the model of a set built from key RECORDS: the canonical record of every decodable point"""
    pts = [O.decompress(np.ascontiguousarray(records[:, c:c + 32]))[0] for c in range(0, records.shape[1], 32)]
    return _where_rec(pts[0], pts[1] if len(pts) == 2 else None, key_ok)


def _lookup_wire_dev(ks, pk, stream=None):
    """(idx uint32 [n], misses) through KeySet.lookup_wire_dev, idx and the counter poisoned first"""
    out = torch.full((len(pk),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    misses = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    ks.lookup_wire_dev(_to_dev(pk), out, misses=misses, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), int(misses.item())


def _check_lookup_wire(ks, where, pk, what):
    want = _expect_rec(where, pk)
    nmiss = int((want == NONE).sum())
    got, misses = _lookup_wire_dev(ks, pk)
    assert (got == want).all(), (what, "dev", _diff(got, want))
    assert misses == nmiss, (what, "dev", misses, nmiss)
    got, misses = ks.lookup_wire(pk)
    assert (got == want).all(), (what, "host", _diff(got, want))
    assert misses == nmiss, (what, "host", misses, nmiss)
    return want


def _poisoned_ws(engine, scheme, n):
    ws = torch.empty(engine.keyed_open_wire_workspace_bytes(scheme, n), dtype=torch.uint8, device=DEV)
    ws.fill_(0xA5)
    return ws


def _open_wire_dev(engine, ks, sig, pk, m, stream=None):
    """(verdicts, misses) through KeySet.verify_open_wire_dev; ok, the counter and the whole workspace poisoned"""
    n = len(m)
    ok = _poison(n)
    ws = _poisoned_ws(engine, ks.scheme, n)
    misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
    ks.verify_open_wire_dev(_to_dev(sig), _to_dev(pk), _to_dev(m), ok, ws, misses=misses, stream=stream)
    torch.cuda.synchronize()
    return ok.cpu().numpy(), int(misses.item())


def _check(engine, ks, sig, pk, m, want, nmiss, what):
    got, misses = _open_wire_dev(engine, ks, sig, pk, m)
    assert (got == want).all(), (what, "dev", _diff(got, want))
    assert misses == nmiss, (what, "dev", misses, nmiss)
    got, misses = ks.verify_open_wire(sig, pk, m)
    assert (got == want).all(), (what, "host", _diff(got, want))
    assert misses == nmiss, (what, "host", misses, nmiss)


# ---- the items of keyed_cases._value_batch, serialized; the oracle's wire verdicts, computed once -----
_WIRE_VALUE = {}


def _wire_value_batch(engine, scheme):
    if scheme not in _WIRE_VALUE:
        b = _value_batch(engine, scheme)
        sig = _sig(b["u"], b["R"], b["Rp"])
        pk = _key_records(b["A"], b["B"])
        want = np.asarray(_oracle_wire(scheme, sig, pk, b["m"])).astype(np.uint8)
        _WIRE_VALUE[scheme] = {"sig": sig, "pk": pk, "m": b["m"], "want": want, "P0": b["P0"], "P1": b["P1"]}
    return _WIRE_VALUE[scheme]


def _parity_set(engine, scheme, b):
    """the batch's 33 keys, the last four registered as other keys, so honest items miss as well"""
    k = len(b["P0"])
    _, _, Y0, Y1 = _keys(engine, scheme, 4, 8080)
    P0, P1 = b["P0"].copy(), b["P1"].copy() if b["P1"] is not None else None
    P0[k - 4:] = Y0
    if P1 is not None:
        P1[k - 4:] = Y1
    return P0, P1


# ---- 1. parity with the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4099))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_wire_parity(engine, scheme, n):
    b = _wire_value_batch(engine, scheme)
    P0, P1 = _parity_set(engine, scheme, b)
    with engine.KeySet(scheme, P0, P1) as ks:
        assert ks.k == 33
        where = _where_rec(P0, P1, ks.key_ok())
        miss = _expect_rec(where, b["pk"][:n]) == NONE
        want = b["want"][:n]
        if n == 4099:
            assert miss.any() and (~miss).any()
            assert 0 < want[miss].sum() < miss.sum() and 0 < want[~miss].sum() < (~miss).sum()
        _check(engine, ks, b["sig"][:n], b["pk"][:n], b["m"][:n], want, int(miss.sum()), (scheme, n))


# ---- 2. the adversarial base set -----------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_wire_adversarial_base_set(engine, scheme):
    """2273 items, undecodable key and nonce records among them; every unique key record registered from its
    bytes, so some keys get key_ok = 0 and some registered records are not the canonical ones of their points"""
    (sig, pk, m), want = ES.base(scheme, "wire", "mixed")
    want = np.asarray(want).astype(np.uint8)
    uniq = np.ascontiguousarray(np.unique(pk, axis=0))
    assert len(want) == 2273 and 0 < want.sum() < len(want)
    # the oracle alone fixes every expected verdict
    assert (np.asarray(_oracle_wire(scheme, sig, pk, m)).astype(np.uint8) == want).all()
    with engine.KeySet.from_wire(scheme, uniq) as ks:
        kok = ks.key_ok()
        assert ks.k == len(uniq) and (kok == 0).any() and (kok == 1).any()
        where = _where_of_records(uniq, kok)
        miss = _expect_rec(where, pk) == NONE
        assert miss.any() and (~miss).any() and 0 < want[~miss].sum() < (~miss).sum()
        _check(engine, ks, sig, pk, m, want, int(miss.sum()), scheme)


# ---- 3. other encodings --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_wire_other_encodings(engine, scheme):
    """the points (0, 1) and (0, -1) registered: their records with the sign bit set are misses that the unkeyed
    equation decides; an item whose record is a registered UNDECODABLE record is a miss with verdict 0; a
    registered pk beside another registered key's gen is a miss"""
    two = scheme != "single"
    n_honest = 4
    sk, gen, K0, K1 = _keys(engine, scheme, n_honest, 4242)
    zero = np.zeros((1, 32), np.uint8)
    rng = np.random.default_rng(33)
    # the key of the secret 0: PK = (0, 1) (double: PK' too; var-generator: under an honest Gen)
    gen0 = gen[:1] if gen is not None else None
    if scheme == "single":
        Z0, Z1 = engine.public_keys(zero), None
    elif scheme == "double":
        Z0, Z1 = engine.public_keys(zero, 0), engine.public_keys(zero, 1)
    else:
        Z0, Z1 = engine.public_keys(zero, Gen=gen0), gen0
    assert H.to_int_point(Z0[0]) == M.IDENTITY
    second = lambda j: np.ascontiguousarray(O.compress(K1[j:j + 1])[0]) if two else np.zeros(0, np.uint8)
    z_second = np.ascontiguousarray(O.compress(Z1)[0]) if two else np.zeros(0, np.uint8)
    ns = _non_squares(1)[0]
    bad = {"v=q": _enc(Q, 0), "nonsquare": ns, "ones": _enc((1 << 255) - 1, 1)}
    reg = {"id": np.concatenate([_enc(1, 0), z_second]), "order2": np.concatenate([_enc(Q - 1, 0), second(0)])}
    for name, enc in bad.items():
        reg[name] = np.concatenate([enc, second(1)])
    for j in range(n_honest):
        reg["honest%d" % j] = _key_records(K0[j:j + 1], K1[j:j + 1] if two else None)[0]
    names = list(reg)
    records = np.ascontiguousarray(np.stack([reg[k] for k in names]))
    # the items: every registered record as it is, the two special points with the sign bit set, the mixed pair
    items = [(k, reg[k]) for k in names]
    for k in ("id", "order2"):
        flipped = reg[k].copy()
        flipped[31] |= 0x80
        items.append((k + "+sign", flipped))
    if scheme == "vargen":
        items.append(("mixed", np.concatenate([reg["honest0"][:32], reg["honest1"][32:]])))
    n = len(items)
    pk = np.ascontiguousarray(np.stack([r for _, r in items]))
    # signatures: honest ones under the secret 0 where the key is the identity, under the honest keys where it is
    # one of them, and under key 0 everywhere else
    signer = {"id": -1, "id+sign": -1}
    signer.update({"honest%d" % j: j for j in range(n_honest)})
    who = np.array([signer.get(name, 0) for name, _ in items])
    skn = np.where((who < 0)[:, None], zero, sk[np.maximum(who, 0)])
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = engine.sign_single(skn, m, r)
    elif scheme == "double":
        u, R, Rp = engine.sign_double(skn, m, r)
    else:
        u, R = engine.sign_vargen(skn, np.where((who < 0)[:, None], gen0, gen[np.maximum(who, 0)]), m, r)
    sig = _sig(u, R, Rp)
    want = np.asarray(_oracle_wire(scheme, sig, pk, m)).astype(np.uint8)
    at = {name: i for i, (name, _) in enumerate(items)}
    assert want[at["id"]] == 1 and want[at["id+sign"]] == 1  # the sign bit on u = 0 decodes to the same point
    assert all(want[at["honest%d" % j]] == 1 for j in range(n_honest))
    assert all(want[at[k]] == 0 for k in bad)
    with engine.KeySet.from_wire(scheme, records) as ks:
        kok = ks.key_ok()
        assert [int(kok[names.index(k)]) for k in bad] == [0, 0, 0] and kok.sum() == len(names) - 3
        where = _where_of_records(records, kok)
        idx = _expect_rec(where, pk)
        hits = ["id", "order2"] + ["honest%d" % j for j in range(n_honest)]
        for k in hits:
            assert idx[at[k]] == names.index(k), k
        misses = [k for k, _ in items if k not in hits]
        assert len(misses) == (6 if scheme == "vargen" else 5) and all(idx[at[k]] == NONE for k in misses)
        _check_lookup_wire(ks, where, pk, scheme)
        _check(engine, ks, sig, pk, m, want, len(misses), scheme)


# ---- 4. the index --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_wire_index_equals_affine_index_and_wraps(engine, scheme):
    """k = 32 keys in a capacity-32 set: 64 slots, half full, among them a run of keys whose home slots in the
    WIRE index are the last slots of the table, so the walk wraps.  The lookup by record equals the lookup by
    affine bytes and the dict model, for registered keys, unregistered ones and other encodings."""
    k, cap = 32, 64
    _, _, C0, C1 = _keys(engine, scheme, 1500, 20261019)
    recs = _key_records(C0, C1)
    homes = np.array([engine.keyset_wire_home_slot(scheme, k, recs[j]) for j in range(len(recs))])
    assert (homes < cap).all()
    last = np.flatnonzero(homes >= cap - 2)
    assert len(last) >= 4, len(last)  # about 47 of 1500 are expected: more keys than the two slots hold
    used, unused = last[:6], last[6:12]
    rest = np.flatnonzero(homes < cap - 2)[:k - len(used)]
    order = np.random.default_rng(3).permutation(np.concatenate([used, rest]))
    assert len(order) == k and len(used) > 2  # the run is in the input: it overflows the last two slots and wraps
    P0 = np.ascontiguousarray(C0[order])
    P1 = np.ascontiguousarray(C1[order]) if C1 is not None else None
    with engine.KeySet.reserved(scheme, k, P0, P1) as ks:
        assert ks.k == ks.capacity == k and ks.index_stats()["capacity"] == cap
        kok = ks.key_ok()
        assert (kok == 1).all()
        where = _where_rec(P0, P1, kok)
        pk = _key_records(P0, P1)
        got = _check_lookup_wire(ks, where, pk, "registered")
        assert (got == np.arange(k)).all()
        by_bytes, miss_b = _lookup_dev(ks, P0, P1)
        assert (by_bytes == got).all() and miss_b == 0
        # unregistered keys with the same home slots, the negations of registered keys, a flipped byte, zeros
        others = [recs[unused]] if len(unused) else []
        neg = pk.copy()
        neg[:, 31] ^= 0x80
        flip = pk.copy()
        flip[:, 5] ^= 1
        probe = np.ascontiguousarray(np.concatenate(others + [neg, flip, np.zeros_like(pk[:2]), pk]))
        got = _check_lookup_wire(ks, where, probe, "probe")
        assert (got[:-k] == NONE).all() and (got[-k:] == np.arange(k)).all()
        affine = [O.decompress(np.ascontiguousarray(probe[:, c:c + 32]))[0] for c in range(0, probe.shape[1], 32)]
        by_bytes, _ = _lookup_dev(ks, affine[0], affine[1] if len(affine) == 2 else None)
        decodable = np.ones(len(probe), bool)
        for c in range(0, probe.shape[1], 32):
            decodable &= O.decompress(np.ascontiguousarray(probe[:, c:c + 32]))[1] == 1
        assert (by_bytes[decodable] == got[decodable]).all()


# ---- 5. the open meaning -------------------------------------------------------------------------------------
def test_open_wire_accepts_a_valid_signature_under_an_unregistered_key(engine):
    sk, _, P0, _ = _keys(engine, "single", 5, 2024)
    rng = np.random.default_rng(1)
    n = 4099
    idx = rng.integers(0, 5, size=n)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R = engine.sign_single(sk[idx], m, r)
    u[::16, 0] ^= 8
    sig, pk = _sig(u, R), _key_records(P0[idx], None)
    want = np.asarray(_oracle_wire("single", sig, pk, m)).astype(np.uint8)
    assert (want == (np.arange(n) % 16 != 0)).all()
    nmiss = int((idx == 4).sum())
    assert nmiss > 0 and 0 < want[idx == 4].sum() < nmiss
    with engine.KeySet("single", np.ascontiguousarray(P0[:4])) as ks:
        closed, cm = ks.verify_lookup(u, R, P0[idx], m)
        assert (closed == (want & (idx < 4))).all() and cm == nmiss
        _check(engine, ks, sig, pk, m, want, nmiss, "k = 4")
    # an empty reserved set: every item takes the miss path
    with engine.KeySet.reserved("single", 8) as nothing:
        assert nothing.k == 0
        _check(engine, nothing, sig, pk, m, want, n, "k = 0")
        idx0, miss0 = _lookup_wire_dev(nothing, pk)
        assert (idx0 == NONE).all() and miss0 == n


# ---- 6. growth -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_wire_index_grows_with_the_set(engine, scheme):
    """lookup_wire before and after append, append_wire and append_mont_cols; a key appended twice keeps its first
    index; an invalid key takes a row and is never found"""
    _, _, K0, K1 = _keys(engine, scheme, 24, 606)
    two = K1 is not None
    sl = lambda P, lo, hi: np.ascontiguousarray(P[lo:hi]) if P is not None else None
    pk = _key_records(K0, K1)
    rng = np.random.default_rng(8)
    with engine.KeySet.reserved(scheme, 40, sl(K0, 0, 6), sl(K1, 0, 6)) as ks:
        reg0, reg1 = [K0[:6]], [K1[:6]] if two else None

        def check(what):
            P0 = np.concatenate(reg0)
            P1 = np.concatenate(reg1) if two else None
            kok = ks.key_ok()
            assert ks.k == len(P0) == len(kok)
            where = _where_rec(P0, P1, kok)
            return _check_lookup_wire(ks, where, pk, what), kok

        got, _ = check("created")
        assert (got[:6] == np.arange(6)).all() and (got[6:] == NONE).all()
        # affine: keys 6 .. 11, and key 2 again
        a0 = np.concatenate([K0[6:12], K0[2:3]])
        a1 = np.concatenate([K1[6:12], K1[2:3]]) if two else None
        assert (ks.append(a0, a1) if two else ks.append(a0)) == 6
        reg0.append(a0)
        if two:
            reg1.append(a1)
        got, _ = check("append")
        assert (got[:12] == np.arange(12)).all() and (got[12:] == NONE).all()
        # records: keys 12 .. 17, key 7 again, and an undecodable record
        recs = np.concatenate([pk[12:18], pk[7:8], pk[18:19]])
        recs[-1, :32] = _enc(Q, 0)
        assert ks.append_wire(np.ascontiguousarray(recs)) == 13
        dec = [O.decompress(np.ascontiguousarray(recs[:, c:c + 32]))[0] for c in range(0, recs.shape[1], 32)]
        reg0.append(dec[0])
        if two:
            reg1.append(dec[1])
        got, kok = check("append_wire")
        assert kok[20] == 0 and kok.sum() == 20
        assert (got[:12] == np.arange(12)).all() and (got[12:18] == np.arange(13, 19)).all()
        assert (got[18:] == NONE).all()
        # objects: keys 18 .. 23, key 0 again
        o0 = np.concatenate([K0[18:24], K0[0:1]])
        o1 = np.concatenate([K1[18:24], K1[0:1]]) if two else None
        cols = [MC.to_limbs_py(H.projective(p, rng)[0], Q) for p in (o0, o1) if p is not None]
        assert ks.append_mont_cols(cols) == 21
        reg0.append(o0)
        if two:
            reg1.append(o1)
        got, _ = check("append_mont_cols")
        assert (got[:12] == np.arange(12)).all() and (got[12:18] == np.arange(13, 19)).all()
        assert (got[18:] == np.arange(21, 27)).all()
        assert ks.k == 28


@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_wire_captured_graph_keeps_its_k(engine, scheme):
    """a graph of the new call captured when the set held 8 of the batch's 16 keys, replayed after the other 8 were
    appended: the wire lookup reads the newer keys' slots as empty, so their items still take the miss path —
    verdicts unchanged, misses as at capture.  A call enqueued after the append finds all 16."""
    k0, n = 8, 300
    sk, gen, P0, P1 = _keys(engine, scheme, 16, 88 + len(scheme))
    rng = np.random.default_rng(89)
    j = rng.integers(0, 16, size=n)
    j[:16] = rng.permutation(16)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = engine.sign_single(sk[j], m, r)
    elif scheme == "double":
        u, R, Rp = engine.sign_double(sk[j], m, r)
    else:
        u, R = engine.sign_vargen(sk[j], gen[j], m, r)
    u[::8, 0] ^= 8
    sig, pk = _sig(u, R, Rp), _key_records(P0[j], P1[j] if P1 is not None else None)
    want = np.asarray(_oracle_wire(scheme, sig, pk, m)).astype(np.uint8)
    assert (want == (np.arange(n) % 8 != 0)).all()
    newer = j >= k0
    assert 0 < want[newer].sum() < newer.sum()
    sl = lambda P, lo, hi: np.ascontiguousarray(P[lo:hi]) if P is not None else None
    dsig, dpk, dm = _to_dev(sig), _to_dev(pk), _to_dev(m)
    with engine.KeySet.reserved(scheme, 16, sl(P0, 0, k0), sl(P1, 0, k0)) as ks:
        ok = _poison(n)
        ws = _poisoned_ws(engine, scheme, n)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.verify_open_wire_dev(dsig, dpk, dm, ok, ws, misses=misses)
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
        got, nmiss = _open_wire_dev(engine, ks, sig, pk, m)
        assert (got == want).all() and nmiss == 0
        del g


# ---- 7. capture and replay -----------------------------------------------------------------------------------
def test_open_wire_capture_and_replay(engine):
    """one captured call, replayed over inputs overwritten in place whose miss counts differ — none, some, all:
    the length of the list lives on the device, so every replay is exact"""
    scheme, n, k = "double", 4099, 8
    sk, _, K0, K1 = _keys(engine, scheme, 2 * k, 707)
    rng = np.random.default_rng(6)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    base = rng.integers(0, k, size=n)
    batches = []
    for miss in (np.zeros(n, bool), rng.integers(0, 8, size=n) == 0, np.ones(n, bool)):
        j = base + k * miss
        u, R, Rp = engine.sign_double(sk[j], m, r)
        wrong = rng.integers(0, 16, size=n) == 0
        u[wrong, 0] ^= 8
        sig, pk = _sig(u, R, Rp), _key_records(K0[j], K1[j])
        want = np.asarray(_oracle_wire(scheme, sig, pk, m)).astype(np.uint8)
        assert (want == ~wrong).all() and 0 < want.sum() < n
        batches.append((sig, pk, want, int(miss.sum())))
    assert batches[0][3] == 0 and 300 < batches[1][3] < 800 and batches[2][3] == n
    with engine.KeySet(scheme, np.ascontiguousarray(K0[:k]), np.ascontiguousarray(K1[:k])) as ks:
        dsig, dpk, dm = _to_dev(batches[-1][0]), _to_dev(batches[-1][1]), _to_dev(m)  # captured over the all-miss batch
        ok = _poison(n)
        ws = _poisoned_ws(engine, scheme, n)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.verify_open_wire_dev(dsig, dpk, dm, ok, ws, misses=misses)
        torch.cuda.synchronize()
        for sig, pk, want, nmiss in batches:
            dsig.copy_(_to_dev(sig))
            dpk.copy_(_to_dev(pk))
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


# ---- 8. the contract -----------------------------------------------------------------------------------------
def test_open_wire_dev_contract(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    b = _wire_value_batch(engine, "double")
    n = 65
    dsig, dpk, dm = _to_dev(b["sig"][:n]), _to_dev(b["pk"][:n]), _to_dev(b["m"][:n])
    vp, sz, null = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p(None)
    p = lambda t: vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    ws_bytes = engine.keyed_open_wire_workspace_bytes("double", n)
    ws = _poisoned_ws(engine, "double", n)
    ks = engine.KeySet("double", b["P0"], b["P1"])
    try:
        h = ks._h

        def verify(nn, okt, wsb, fn="double", sig=p(dsig), pk=p(dpk), m=p(dm), work=p(ws)):
            return getattr(L, "dsv_verify_%s_keyed_open_wire_dev" % fn)(
                h, sig, pk, m, sz(nn), p(okt), work, sz(wsb), stream, null)

        ok = _poison(n)
        assert verify(n, ok, ws_bytes - 1) == INVALID
        assert b"workspace" in L.dsv_last_error()
        for fn in ("single", "vargen"):  # a set of another scheme
            assert verify(n, ok, ws_bytes, fn=fn) == INVALID
            assert b"scheme" in L.dsv_last_error()
        assert verify(n, ok, ws_bytes, sig=null) == INVALID
        assert verify(n, ok, ws_bytes, pk=null) == INVALID
        assert verify(n, ok, ws_bytes, m=null) == INVALID
        assert verify(n, ok, ws_bytes, work=null) == INVALID
        odd_sig = torch.zeros(n * 96 + 8, dtype=torch.uint8, device=DEV)[8:].view(n, 96)  # 8 bytes off a 16-byte boundary
        odd_pk = torch.zeros(n * 64 + 8, dtype=torch.uint8, device=DEV)[8:].view(n, 64)
        assert verify(n, ok, ws_bytes, sig=p(odd_sig)) == INVALID
        assert b"aligned" in L.dsv_last_error()
        assert verify(n, ok, ws_bytes, pk=p(odd_pk)) == INVALID
        assert b"aligned" in L.dsv_last_error()
        idx_out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        assert L.dsv_keyset_lookup_wire_dev(h, p(odd_pk), sz(n), p(idx_out), null, stream) == INVALID
        assert b"aligned" in L.dsv_last_error()
        assert L.dsv_keyset_lookup_wire_dev(h, null, sz(n), p(idx_out), null, stream) == INVALID
        assert L.dsv_keyset_lookup_wire_dev(h, p(dpk), sz(n), null, null, stream) == INVALID
        with pytest.raises(ValueError):
            ks.verify_open_wire_dev(odd_sig, dpk, dm, ok, ws)
        with pytest.raises(ValueError):
            ks.verify_open_wire_dev(dsig, odd_pk, dm, ok, ws)
        with pytest.raises(ValueError):
            ks.verify_open_wire_dev(dsig, dpk, dm, ok, ws[:-1])
        with pytest.raises(ValueError):
            ks.verify_open_wire_dev(dsig[:, :64], dpk, dm, ok, ws)  # single records on a double key set
        with pytest.raises(ValueError):
            ks.lookup_wire_dev(odd_pk, idx_out)
        # n = 0: DSV_OK, nothing touched (no workspace needed)
        assert verify(0, ok, 0) == 0
        hm = sz(55)
        assert L.dsv_verify_double_keyed_open_wire(h, null, null, null, sz(0), null, ctypes.byref(hm)) == 0
        assert hm.value == 0
        assert L.dsv_keyset_lookup_wire_dev(h, null, sz(0), null, null, stream) == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        assert (idx_out.cpu().numpy() == 0x5A5A5A5A).all()
        assert (ws.cpu().numpy() == 0xA5).all()
        # the full workspace: the verdicts
        assert verify(n, ok, ws_bytes) == 0, L.dsv_last_error().decode()
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == b["want"][:n]).all()
    finally:
        ks.close()
    # a closed set has no handle left to call with
    with pytest.raises(ValueError):
        ks.verify_open_wire(b["sig"][:n], b["pk"][:n], b["m"][:n])
    with pytest.raises(ValueError):
        ks.verify_open_wire_dev(dsig, dpk, dm, _poison(n), ws)
    with pytest.raises(ValueError):
        ks.lookup_wire(b["pk"][:n])


# ---- 9. host form equals device form -------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_wire_host_form_equals_dev_form(engine, scheme):
    """2^18 + 5 items tiled from the parity batch: the host form's second chunk holds five items"""
    b = _wire_value_batch(engine, scheme)
    n = (1 << 18) + 5
    reps = -(-n // len(b["m"]))
    sig, pk, m = [np.ascontiguousarray(np.concatenate([a] * reps)[:n]) for a in (b["sig"], b["pk"], b["m"])]
    want = np.tile(b["want"], reps)[:n]
    P0, P1 = _parity_set(engine, scheme, b)
    with engine.KeySet(scheme, P0, P1) as ks:
        where = _where_rec(P0, P1, ks.key_ok())
        nmiss = int(np.tile(_expect_rec(where, b["pk"]) == NONE, reps)[:n].sum())
        assert 0 < nmiss < n
        host, hm = ks.verify_open_wire(sig, pk, m)
        dev, dm = _open_wire_dev(engine, ks, sig, pk, m)
    assert (host == dev).all(), _diff(host, dev)
    assert (host == want).all(), _diff(host, want)
    assert hm == dm == nmiss
