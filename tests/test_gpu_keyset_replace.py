"""Keys replaced in place on the GPU (dsv_keyset_replace*, the key cache's eviction): a set with keys replaced equals
the set dsv_keyset_create builds over the final key list — key_ok, table entries, lookups by value and by record,
by-index verdicts against the CPU oracle —, both indices have the canonical layout of tests/keyset_index_model.py
(clusters, wrap-around, duplicates, invalid keys), the open-set forms return the unkeyed verdicts before and after, a
captured graph keeps its k, a full set never fills up, refused calls change nothing, and verify calls run beside
replaces.  Keys and items come from tests/keyed_cases.py; every batch holds valid and invalid
items.  Shapes: capacity 8 (the smallest index: 64 slots), 16, and 40 (128 slots)."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import keyset_index_model as IM
import oracle_lib as O
import pymodel as M
from keyed_cases import _dev, _diff, _keys, _le, _oracle, _poison, _scalars, _sign_items

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
NONE = 0xFFFFFFFF
INVALID = "dsv error -2"
SCHEMES = ("single", "double", "vargen")
Q = M.Q


def _c(a):
    return np.ascontiguousarray(a) if a is not None else None


def _cols(P0, P1, rows=slice(None)):
    return [_c(P0[rows])] + ([_c(P1[rows])] if P1 is not None else [])


def _items(engine, scheme, sk, gen, P0, P1, j, seed):
    """len(j) items, item i signed under key j[i] of the pool (sk, gen, P0, P1); every 8th has a bit of u flipped,
    every 8th + 3 a bit of m; A / B: the items' own key columns"""
    rng = np.random.default_rng(seed)
    n = len(j)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, Rp = _sign_items(engine, scheme, _c(sk[j]), _c(gen[j]) if gen is not None else None, m, r)
    u[::8, 0] ^= 8
    m[3::8, 0] ^= 1
    return {"scheme": scheme, "u": u, "R": R, "Rp": Rp, "m": m, "A": _c(P0[j]), "B": _c(P1[j]) if P1 is not None else None,
            "j": j}


def _pts(w):
    return [w["R"]] + ([w["Rp"]] if w["Rp"] is not None else [])


def _keycols(w):
    return [w["A"]] + ([w["B"]] if w["B"] is not None else [])


def _sig(w):
    return _c(np.hstack([w["u"]] + [O.compress(p) for p in _pts(w)]))


def _unkeyed(engine, w):
    """the unkeyed call's verdict vector on the items' own key bytes"""
    s = w["scheme"]
    if s == "single":
        return np.asarray(engine.verify_single(w["u"], w["R"], w["A"], w["m"])).astype(np.uint8)
    if s == "double":
        return np.asarray(engine.verify_double(w["u"], w["R"], w["Rp"], w["A"], w["B"], w["m"])).astype(np.uint8)
    return np.asarray(engine.verify_vargen(w["u"], w["R"], w["A"], w["B"], w["m"])).astype(np.uint8)


def _by_index(engine, ks, w, idx, stream=None):
    n = len(idx)
    ok = _poison(n)
    ws = torch.empty(engine.keyed_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    ks.verify_dev(*_dev([w["u"]] + _pts(w) + [idx.astype(np.uint32), w["m"]]), ok, ws, stream=stream)
    torch.cuda.synchronize()
    return ok.cpu().numpy()


def _open_calls(engine, ks, w):
    """{form: (verdicts, misses)} of the open-set _dev forms on the batch w: by affine key value and by key record"""
    scheme, n = w["scheme"], len(w["j"])
    out = {}
    ok, ms = _poison(n), torch.full((1,), 999, dtype=torch.int32, device=DEV)
    ws = torch.empty(engine.keyed_open_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    call = ks.verify_vargen_open_dev if scheme == "vargen" else ks.verify_open_dev
    call(*_dev([w["u"]] + _pts(w) + _keycols(w) + [w["m"]]), ok, ws, misses=ms)
    torch.cuda.synchronize()
    out["affine"] = (ok.cpu().numpy(), int(ms.item()))
    ok, ms = _poison(n), torch.full((1,), 999, dtype=torch.int32, device=DEV)
    ws = torch.empty(engine.keyed_open_wire_workspace_bytes(scheme, n), dtype=torch.uint8, device=DEV)
    ks.verify_open_wire_dev(*_dev([_sig(w), IM.records_of(w["A"], w["B"]), w["m"]]), ok, ws, misses=ms)
    torch.cuda.synchronize()
    out["record"] = (ok.cpu().numpy(), int(ms.item()))
    return out


def _check_slots(engine, ks, scheme, P0, P1, what=""):
    """both slot arrays equal the model's over the set's current keys P0 [, P1] (k rows) and its own key_ok"""
    kok = ks.key_ok()
    assert len(kok) == ks.k == len(P0)
    for form in IM.FORMS:
        want = IM.canonical_slots(engine, scheme, P0, P1, kok, ks.capacity, form)
        got = engine.keyset_slots(ks, form)
        assert got.shape == want.shape, (what, form, got.shape, want.shape)
        assert (got == want).all(), (what, form, np.flatnonzero(got != want)[:8].tolist(), got[got != want][:8].tolist(),
                                     want[got != want][:8].tolist())
    assert ks.index_stats()["occupied"] == int((want != NONE).sum())


def _expect_lookup(F0, F1, kok, L0, L1):
    where = {}
    row = lambda A, B, i: bytes(A[i]) + (bytes(B[i]) if B is not None else b"")
    for j in range(len(F0)):
        if kok[j]:
            where.setdefault(row(F0, F1, j), j)
    return np.array([where.get(row(L0, L1, i), NONE) for i in range(len(L0))], dtype=np.uint32)


# ---- 1. / 2. a set with keys replaced equals the set built at once over the final keys ----------------------------
K = 40
REPLACED = np.array([0, 7, 39], dtype=np.uint32)
_CASES = {}


def _case(engine, scheme):
    """58 keys: 0 .. 39 registered, 40 the new key, 41 the base of the invalid one, 42 .. 57 never registered.  The
    call replaces key 0 by key 40, key 7 by a copy of key 5, key 39 by an invalid key (u + q: the same residue, not
    canonical).  F: the final key list; a 256-item batch signed under it with the oracle's verdicts."""
    if scheme in _CASES:
        return _CASES[scheme]
    sk, gen, P0, P1 = _keys(engine, scheme, K + 2 + 16, 5100 + len(scheme))
    two = P1 is not None
    bad = P0[41].copy()
    bad[:32] = _le(M.from_le(bad[:32]) + Q)
    A0 = _c(np.stack([P0[40], P0[5], bad]))
    A1 = _c(np.stack([P1[40], P1[5], P1[41]])) if two else None
    F0, F1 = P0[:K].copy(), (P1[:K].copy() if two else None)
    F0[REPLACED] = A0
    if two:
        F1[REPLACED] = A1
    src = np.arange(K)
    src[REPLACED] = (40, 5, 41)  # whose secret signs under the final key at an index
    rng = np.random.default_rng(77 + len(scheme))
    j = rng.integers(0, K, size=256)
    j[:8] = (0, 7, 39, 5, 1, 6, 8, 38)
    w = _items(engine, scheme, sk[src], gen[src] if gen is not None else None, F0, F1, j, 99)
    want = np.asarray(_oracle(scheme, w["u"], w["R"], w["Rp"], w["A"], w["B"], w["m"])).astype(np.uint8)
    assert (want[j == 39] == 0).all() and 0 < want.sum() < len(j) and want[1] == 1
    # lookups: the final keys, the evicted keys, 16 keys that were never registered
    L0 = _c(np.concatenate([F0, P0[REPLACED], P0[42:58]]))
    L1 = _c(np.concatenate([F1, P1[REPLACED], P1[42:58]])) if two else None
    kok = np.ones(K, np.uint8)
    kok[39] = 0
    hits = _expect_lookup(F0, F1, kok, L0, L1)
    assert hits[7] == 5 and hits[39] == NONE and (hits[K:] == NONE).all() and int((hits == NONE).sum()) == 20
    assert (IM.records_of(P0[:K]) == O.compress(_c(P0[:K]))).all()  # the model's records are the reference's
    c = {"P0": P0, "P1": P1, "A0": A0, "A1": A1, "F0": _c(F0), "F1": _c(F1), "w": w, "want": want, "L0": L0, "L1": L1,
         "kok": kok, "hits": hits}
    _CASES[scheme] = c
    return c


def _replaced_and_fresh(engine, scheme, form, c):
    """(the set of keys 0 .. 39 with [0, 7, 39] replaced through `form`, the set built at once over the final list)"""
    ks = engine.KeySet(scheme, *_cols(c["P0"], c["P1"], slice(0, K)))
    if form == "affine":
        ks.replace(REPLACED, *_cols(c["A0"], c["A1"]))
        return ks, engine.KeySet(scheme, c["F0"], c["F1"])
    new = IM.records_of(c["A0"], c["A1"])
    new[2, :32] = _le(Q + 1)  # v = q + 1: a record from_bytes rejects
    final = IM.records_of(c["F0"], c["F1"])
    final[REPLACED] = new
    ks.replace_wire(REPLACED, new)
    return ks, engine.KeySet.from_wire(scheme, final)


@pytest.mark.parametrize("form", ("affine", "wire"))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_replaced_set_equals_fresh_set(engine, scheme, form):
    c = _case(engine, scheme)
    ks, fresh = _replaced_and_fresh(engine, scheme, form, c)
    with ks, fresh:
        assert ks.k == ks.capacity == fresh.k == K and ks.nbytes == fresh.nbytes
        assert (ks.key_ok() == c["kok"]).all() and (fresh.key_ok() == c["kok"]).all()
        # (the affine bytes of an undecodable record are the decoder's business: its table is not compared)
        for key in (0, 1, 6, 7, 8, 38) + ((39,) if form == "affine" else ()):
            for point in range(1 if scheme == "single" else 2):
                for window, digit in ((0, 1), (15, -128), (31, 77)):
                    a, b = ks.debug_entry(key, point, window, digit), fresh.debug_entry(key, point, window, digit)
                    assert (a == b).all(), (key, point, window, digit)
                    if key == 7:
                        assert (a == ks.debug_entry(5, point, window, digit)).all()
        for s in (ks, fresh):
            got, misses = s.lookup(*_cols(c["L0"], c["L1"]))
            assert (got == c["hits"]).all() and misses == 20, (s is ks, _diff(got, c["hits"]), misses)
            got, misses = s.lookup_wire(IM.records_of(c["L0"], c["L1"]))
            assert (got == c["hits"]).all() and misses == 20, (s is ks, "wire", _diff(got, c["hits"]), misses)
            got = _by_index(engine, s, c["w"], c["w"]["j"])
            assert (got == c["want"]).all(), (s is ks, _diff(got, c["want"]))


@pytest.mark.parametrize("form", ("affine", "wire"))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_replaced_set_has_the_canonical_layout(engine, scheme, form):
    c = _case(engine, scheme)
    ks, fresh = _replaced_and_fresh(engine, scheme, form, c)
    with ks, fresh:
        assert len(engine.keyset_slots(ks, 0)) == len(engine.keyset_slots(ks, "record")) == 128
        _check_slots(engine, ks, scheme, c["F0"], c["F1"], "replaced")
        # (the fresh set holds the same keys in its slots, but the lanes of one append launch claim slots as they
        # come: only the order inside a cluster may differ from the canonical one)
        for f in IM.FORMS:
            got = engine.keyset_slots(ks, f)
            assert sorted(got.tolist()) == sorted(engine.keyset_slots(fresh, f).tolist())
            assert 5 in got and 7 not in got and 39 not in got


# ---- 3. clusters and wrap-around -------------------------------------------------------------------------------------
def test_replacing_the_head_of_a_wrapping_cluster(engine):
    """capacity 8: the smallest index there is, 64 slots (the cluster therefore wraps from slot 63, not 15).  Four
    keys at home in the last slot, registered first, and two at home in slot 0, appended, fill slots 63, 0, 1, 2 and
    3, 4.  The first key of the cluster is replaced by a key with a home elsewhere: the walks of the five keys
    behind it must not be cut (a cleared slot) nor keep meeting the evicted key (a slot that kept its occupant);
    afterwards the layout is the canonical one, slot for slot."""
    capacity = 8
    _, _, C, _ = _keys(engine, "single", 900, 20261020)
    cap = IM.cap_of(capacity)
    homes = np.array([engine.keyset_home_slot("single", capacity, C[i]) for i in range(len(C))])
    last, zero = np.flatnonzero(homes == cap - 1)[:4], np.flatnonzero(homes == 0)[:2]
    assert len(last) == 4 and len(zero) == 2  # about 14 of 900 per slot
    other = int(np.flatnonzero((homes > 16) & (homes < 48))[0])
    keys = _c(C[np.concatenate([last, zero])])
    with engine.KeySet.reserved("single", capacity, _c(keys[:4])) as ks:
        assert len(engine.keyset_slots(ks, "affine")) == cap == 64
        assert ks.append(_c(keys[4:])) == 4
        slots = engine.keyset_slots(ks, "affine")  # (inside one append launch the lanes claim slots as they come)
        assert sorted(slots[[cap - 1, 0, 1, 2]].tolist()) == [0, 1, 2, 3] and sorted(slots[3:5].tolist()) == [4, 5]
        ks.replace([0], _c(C[other:other + 1]))
        assert ks.k == 6
        now = keys.copy()
        now[0] = C[other]
        got, misses = ks.lookup(_c(np.concatenate([now, keys[:1]])))
        assert got.tolist() == [0, 1, 2, 3, 4, 5, NONE] and misses == 1
        got, misses = ks.lookup_wire(IM.records_of(np.concatenate([now, keys[:1]])))
        assert got.tolist() == [0, 1, 2, 3, 4, 5, NONE] and misses == 1
        slots = engine.keyset_slots(ks, "affine")
        assert slots[cap - 1] == 1 and slots[:5].tolist() == [2, 3, 4, 5, NONE] and slots[homes[other]] == 0
        _check_slots(engine, ks, "single", now, None, "after")
        # and back: the evicted key returns to index 0 and to the head of its cluster
        ks.replace([0], _c(keys[:1]))
        slots = engine.keyset_slots(ks, "affine")
        assert slots[cap - 1] == 0 and slots[:5].tolist() == [1, 2, 3, 4, 5] and slots[homes[other]] == NONE
        _check_slots(engine, ks, "single", keys, None, "back")


# ---- 4. the open-set forms across an eviction ------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_set_verdicts_across_eviction(engine, scheme):
    """22 keys: 0 .. 15 registered, 16 and 17 take the places of keys 2 and 9, 18 .. 21 are never registered.  300
    items under all of them: both open-set forms return the unkeyed call's vector before and after; misses counts
    the items under the new and the unregistered keys before, under the evicted and the unregistered keys after."""
    sk, gen, P0, P1 = _keys(engine, scheme, 22, 5200 + len(scheme))
    rng = np.random.default_rng(5)
    j = rng.integers(0, 22, size=300)
    j[:22] = rng.permutation(22)
    w = _items(engine, scheme, sk, gen, P0, P1, j, 6)
    want = _unkeyed(engine, w)
    bad = np.zeros(300, bool)
    bad[::8] = bad[3::8] = True
    assert (want == ~bad).all()
    count = lambda keys: int(np.isin(j, keys).sum())
    with engine.KeySet(scheme, *_cols(P0, P1, slice(0, 16))) as ks:
        for name, (got, misses) in _open_calls(engine, ks, w).items():
            assert (got == want).all(), ("before", name, _diff(got, want))
            assert misses == count([16, 17, 18, 19, 20, 21]), ("before", name, misses)
        ks.replace([2, 9], *_cols(P0, P1, slice(16, 18)))
        for name, (got, misses) in _open_calls(engine, ks, w).items():
            assert (got == want).all(), ("after", name, _diff(got, want))
            assert misses == count([2, 9, 18, 19, 20, 21]), ("after", name, misses)
        # by index the new keys decide: items of key 16 under index 2, of key 17 under index 9
        idx = np.where(j == 16, 2, np.where(j == 17, 9, np.where(np.isin(j, [2, 9]) | (j > 17), NONE, j)))
        got = _by_index(engine, ks, w, idx)
        closed = want & (idx != NONE).astype(np.uint8)
        assert (got == closed).all() and closed[j == 16].sum() > 0, _diff(got, closed)


# ---- 5. a captured graph keeps its k ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ("single", "double"))
def test_captured_graph_keeps_its_k_across_a_replace(engine, scheme):
    """capacity 16, a graph over lookup_dev and verify_open_dev captured at k = 8; then 8 keys are appended and keys
    3 (below the graph's k) and 12 replaced.  Replayed, the graph still finds every unreplaced key below 8 at its
    index, misses the old key 3 and every key from index 8 on — the new key 12 too — and finds the new key 3 at 3;
    its open-set verdicts are the unkeyed call's."""
    sk, gen, P0, P1 = _keys(engine, scheme, 18, 5300 + len(scheme))  # 16, 17: the new keys 3 and 12
    rng = np.random.default_rng(8)
    j = rng.integers(0, 18, size=300)
    j[:18] = rng.permutation(18)
    w = _items(engine, scheme, sk, gen, P0, P1, j, 9)
    want = _unkeyed(engine, w)
    assert 0 < want.sum() < 300
    first8 = lambda: [_c(P0[:8])] + ([_c(P1[:8])] if P1 is not None else [])
    with engine.KeySet.reserved(scheme, 16, *first8()) as ks:
        keys = _dev(_cols(P0, P1))
        idx_out = torch.full((18,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        miss_l = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        args = _dev([w["u"]] + _pts(w) + _keycols(w) + [w["m"]])
        ok, miss_o = _poison(300), torch.full((1,), 999, dtype=torch.int32, device=DEV)
        ws = torch.empty(engine.keyed_open_workspace_bytes(300), dtype=torch.uint8, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.lookup_dev(*keys, idx_out, misses=miss_l)
            ks.verify_open_dev(*args, ok, ws, misses=miss_o)
        torch.cuda.synchronize()

        def replay(what, hits):
            idx_out.fill_(0x5A5A5A5A)
            ok.fill_(POISON)
            miss_l.fill_(999)
            miss_o.fill_(999)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = idx_out.cpu().numpy().view(np.uint32)
            assert got.tolist() == hits, (what, got.tolist())
            assert int(miss_l.item()) == hits.count(NONE), what
            verdicts = ok.cpu().numpy()
            assert (verdicts == want).all(), (what, _diff(verdicts, want))
            seen = [h for h in hits if h != NONE]
            found = np.isin(j, [i for i in range(18) if hits[i] != NONE])
            assert int(miss_o.item()) == int((~found).sum()) and len(seen) == 8, what

        before = list(range(8)) + [NONE] * 10
        replay("captured", before)
        assert ks.append(*_cols(P0, P1, slice(8, 16))) == 8
        replay("after the append", before)
        ks.replace([3, 12], *_cols(P0, P1, slice(16, 18)))
        assert ks.k == 16
        after = [0, 1, 2, NONE, 4, 5, 6, 7] + [NONE] * 8 + [3, NONE]
        replay("after the replace", after)
        now0, now1 = P0[:16].copy(), (P1[:16].copy() if P1 is not None else None)
        now0[[3, 12]] = P0[16:18]
        if now1 is not None:
            now1[[3, 12]] = P1[16:18]
        _check_slots(engine, ks, scheme, now0, now1, "after the replace")
        # a call enqueued now sees all 16 current keys
        got, misses = ks.lookup(*_cols(P0, P1))
        assert got.tolist() == [0, 1, 2, NONE] + list(range(4, 12)) + [NONE, 13, 14, 15, 3, 12] and misses == 2
        del g


# ---- 6. it never fills up ----------------------------------------------------------------------------------------------
def test_a_full_set_takes_replaces_for_ever(engine):
    """200 single-key replaces on a full capacity-8 set, cycling through 24 keys: a slot that merely kept its old
    occupant, or an index that collected tombstones, would fill the 64 slots after 56 of them"""
    _, _, C, _ = _keys(engine, "single", 24, 5400)
    cur = C[:8].copy()
    with engine.KeySet("single", _c(cur)) as ks:
        assert ks.k == ks.capacity == 8
        for t in range(200):
            key = (8 + t) % 24
            ks.replace([t % 8], _c(C[key:key + 1]))  # raises unless DSV_OK
            cur[t % 8] = C[key]
        assert ks.k == 8 and (ks.key_ok() == 1).all()
        assert len({bytes(r) for r in cur}) == 8
        _check_slots(engine, ks, "single", cur, None, "after 200 replaces")
        assert ks.index_stats()["occupied"] <= 8
        got, misses = ks.lookup(_c(cur))
        assert got.tolist() == list(range(8)) and misses == 0
        got, misses = ks.lookup_wire(IM.records_of(cur))
        assert got.tolist() == list(range(8)) and misses == 0


# ---- 7. argument checks with a device ----------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ("single", "double"))
def test_refused_replaces_change_nothing(engine, scheme):
    from schnorr_amd import _lib

    L = _lib.load()
    _, _, P0, P1 = _keys(engine, scheme, 8, 5500 + len(scheme))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    sz = ctypes.c_size_t
    new0, new1 = _c(P0[6:8]), (_c(P1[6:8]) if P1 is not None else None)
    with engine.KeySet.reserved(scheme, 8, *_cols(P0, P1, slice(0, 6))) as ks:
        def state():
            return ([engine.keyset_slots(ks, f).tolist() for f in IM.FORMS], ks.key_ok().tolist(), ks.k,
                    ks.debug_entry(1, 0, 3, 5).tolist(), ks.debug_entry(5, 0, 31, -128).tolist())

        before = state()

        def refused(indices, a=new0, b=new1, m=2):
            idx = np.asarray(indices, dtype=np.uint32) if indices is not None else None
            rc = L.dsv_keyset_replace(ks._h, p(idx), p(a), p(b), sz(m))
            assert rc == -2, (indices, rc, L.dsv_last_error())
            rc = L.dsv_keyset_replace_wire(ks._h, p(idx), p(IM.records_of(a, b)) if a is not None else None, sz(m))
            assert rc == -2, (indices, "wire", rc, L.dsv_last_error())
            assert state() == before, indices

        refused([1, 6])        # k = 6: an index >= k (below the capacity)
        refused([8, 1])        # ... and one past the capacity
        refused([NONE, 0])
        refused([1, 1])        # an index given twice
        refused([2, 5], a=None, b=None)   # NULL keys
        refused(None)          # NULL indices
        if P1 is not None:
            rc = L.dsv_keyset_replace(ks._h, p(np.array([2, 5], np.uint32)), p(new0), None, sz(2))
            assert rc == -2 and state() == before
        with pytest.raises(_lib.DsvError, match=INVALID):
            ks.replace([0, 7], new0, *([new1] if new1 is not None else []))
        assert L.dsv_keyset_replace(ks._h, None, None, None, sz(0)) == 0   # m = 0: DSV_OK, whatever the pointers
        assert L.dsv_keyset_replace_wire(ks._h, None, None, sz(0)) == 0
        assert state() == before
        assert L.dsv_keyset_replace(None, p(np.array([0], np.uint32)), p(new0), p(new1), sz(1)) == -2
        assert state() == before
        ks.replace([5, 0], new0, *([new1] if new1 is not None else []))     # and the accepted call does change it
        assert state() != before and ks.k == 6


# ---- 8. beside a verifier ------------------------------------------------------------------------------------------------
def test_replaces_run_beside_a_verifier(engine):
    """one thread issues 50 by-index calls of 4096 items over keys 0 .. 3 on a stream of its own, the main thread
    replaces key 7 ten times meanwhile: every verdict vector is the oracle's"""
    sk, gen, P0, _ = _keys(engine, "single", 18, 5600)
    rng = np.random.default_rng(11)
    j = rng.integers(0, 4, size=256)
    w = _items(engine, "single", sk, gen, P0, None, j, 12)
    want = np.tile(np.asarray(_oracle("single", w["u"], w["R"], None, w["A"], None, w["m"])).astype(np.uint8), 16)
    assert 0 < want.sum() < len(want)
    tile = lambda a: _c(np.tile(a, (16, 1)))
    n = 4096
    args = _dev([tile(w["u"]), tile(w["R"]), np.tile(j, 16).astype(np.uint32), tile(w["m"])])
    errors, seen = [], []
    with engine.KeySet("single", _c(P0[:8])) as ks:
        def verifier():
            try:
                torch.cuda.set_device(0)
                st = torch.cuda.Stream(device=DEV)
                ws = torch.empty(engine.keyed_workspace_bytes(n), dtype=torch.uint8, device=DEV)
                ok = _poison(n)
                st.wait_stream(torch.cuda.current_stream())
                for _ in range(50):
                    ks.verify_dev(*args, ok, ws, stream=st)
                    st.synchronize()
                    seen.append(ok.cpu().numpy().copy())
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        torch.cuda.synchronize()
        t = threading.Thread(target=verifier)
        t.start()
        try:
            for i in range(10):
                ks.replace([7], _c(P0[8 + i:9 + i]))
        finally:
            t.join()
        assert not errors, errors
        assert len(seen) == 50
        for got in seen:
            assert (got == want).all(), _diff(got, want)
        got, misses = ks.lookup(_c(P0[:18]))
        assert got.tolist() == list(range(7)) + [NONE] * 10 + [7] and misses == 10
