"""Key sets that grow on the GPU (dsv_keyset_create_reserved, dsv_keyset_append*): a set built by appending equals
the set dsv_keyset_create builds over the same keys — key_ok, table entries, every keyed verdict vector, all equal
to the CPU oracle's —, the index keeps its invariants across appends (clusters that span calls, wrap-around,
duplicates, invalid keys), a full set refuses and stays as it was, a captured graph keeps the k of its capture
(the stale-k rule of the lookup kernel), and verify calls run beside appends.  Keys and items come from
tests/keyed_cases.py; every batch holds valid and invalid items."""
import ctypes
import threading

import numpy as np
import pytest
import torch

import harness as H
import mont_cases as MC
import oracle_lib as O
import pymodel as M
from keyed_cases import _check_lookup, _dev, _diff, _expect, _keys, _le, _oracle, _poison, _scalars, _where

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
NONE = 0xFFFFFFFF
TOO_LARGE = "dsv error -5"
SCHEMES = ("single", "double", "vargen")
N = 300            # items per call: no multiple of 64 or 256
APPENDS = (1, 65)  # keys per append: rows cross the 64-lane build block (two keys per block) and the lookup block
K0_MAX = 63
Q = M.Q

_WORLDS = {}


def _world(engine, scheme, nkeys, seed):
    """nkeys keys and N items signed under them (key j[i]); every 8th item has a bit of u flipped, every 8th + 3 a
    bit of m.  The oracle's verdicts on the items' own key bytes, computed once and shared."""
    key = (scheme, nkeys, seed)
    if key in _WORLDS:
        return _WORLDS[key]
    sk, gen, P0, P1 = _keys(engine, scheme, nkeys, seed)
    rng = np.random.default_rng(seed + 1)
    j = rng.integers(0, nkeys, size=N)
    j[:nkeys] = rng.permutation(nkeys)[:N]  # every key signs at least once (nkeys <= N)
    m, r = _scalars(rng, N, 0x3F), _scalars(rng, N, 0x07)
    Rp = None
    if scheme == "single":
        u, R = engine.sign_single(sk[j], m, r)
    elif scheme == "double":
        u, R, Rp = engine.sign_double(sk[j], m, r)
    else:
        u, R = engine.sign_vargen(sk[j], gen[j], m, r)
    u[::8, 0] ^= 8
    m[3::8, 0] ^= 1
    A = np.ascontiguousarray(P0[j])
    B = np.ascontiguousarray(P1[j]) if P1 is not None else None
    want = np.asarray(_oracle(scheme, u, R, Rp, A, B, m)).astype(np.uint8)
    bad = np.zeros(N, bool)
    bad[::8] = bad[3::8] = True
    assert (want == ~bad).all()
    w = {"scheme": scheme, "P0": P0, "P1": P1, "j": j, "u": u, "R": R, "Rp": Rp, "A": A, "B": B, "m": m,
         "want": want}
    _WORLDS[key] = w
    return w


def _pts(w):
    return [w["R"]] + ([w["Rp"]] if w["Rp"] is not None else [])


def _key_cols(w):
    return [w["A"]] + ([w["B"]] if w["B"] is not None else [])


def _records(P0, P1):
    """the reference's key records of affine keys"""
    return np.ascontiguousarray(O.compress(P0) if P1 is None else np.hstack([O.compress(P0), O.compress(P1)]))


def _sl(P, lo, hi):
    return np.ascontiguousarray(P[lo:hi]) if P is not None else None


def _grow(engine, scheme, P0, P1, k0, appends, form, capacity):
    """a reserved set of the first k0 keys, the rest appended in calls of `appends` keys in the given key form;
    every first_index is the k before its call"""
    ks = engine.KeySet.reserved(scheme, capacity, _sl(P0, 0, k0), _sl(P1, 0, k0))
    assert ks.k == k0 and ks.capacity == capacity and ks.nbytes == engine.keyset_bytes(scheme, capacity)
    at = k0
    rng = np.random.default_rng(at)
    for m in appends:
        a, b = _sl(P0, at, at + m), _sl(P1, at, at + m)
        if form == "affine":
            first = ks.append(a, b) if b is not None else ks.append(a)
        elif form == "wire":
            first = ks.append_wire(_records(a, b))
        else:
            first = ks.append_mont_cols([MC.to_limbs_py(H.projective(p, rng)[0], Q) for p in (a, b) if p is not None])
        assert first == at and ks.k == at + m
        at += m
    assert at == len(P0)
    return ks


def _keyed_calls(engine, ks, w, idx):
    """every keyed _dev form on the batch of w at the key indices idx -> {form: verdicts}"""
    scheme, two = w["scheme"], w["Rp"] is not None
    out = {}
    by_idx = _dev([w["u"]] + _pts(w) + [idx, w["m"]])
    by_val = _dev([w["u"]] + _pts(w) + _key_cols(w) + [w["m"]])

    def run(name, fn, args, ws_bytes, **kw):
        ok = _poison(N)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        fn(*args, ok, ws, **kw)
        torch.cuda.synchronize()
        out[name] = ok.cpu().numpy()

    run("keyed", ks.verify_dev, by_idx, engine.keyed_workspace_bytes(N))
    run("lookup", ks.verify_lookup_dev, by_val, engine.keyed_lookup_workspace_bytes(N))
    if scheme != "vargen":
        run("open", ks.verify_open_dev, by_val, engine.keyed_open_workspace_bytes(N))
    sig = np.hstack([w["u"], O.compress(w["R"])] + ([O.compress(w["Rp"])] if two else []))
    run("wire", ks.verify_wire_dev, _dev([np.ascontiguousarray(sig), idx, w["m"]]),
        engine.keyed_wire_workspace_bytes(scheme, N))
    run("rlc", ks.verify_rlc_dev, by_idx, engine.keyed_rlc_workspace_bytes(N, ks.k, 8), window_bits=8)
    return out


# ---- 1. a set built by appending equals the set built at once -----------------------------------------------
@pytest.mark.parametrize("form", ("affine", "wire"))
@pytest.mark.parametrize("k0", (0, 1, K0_MAX))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_appended_set_equals_set_built_at_once(engine, scheme, k0, form):
    w = _world(engine, scheme, K0_MAX + sum(APPENDS), 4100 + len(scheme))
    off = K0_MAX - k0  # the case's keys are the world's from `off` on: items under earlier keys are not in the set
    P0, P1 = _sl(w["P0"], off, None), _sl(w["P1"], off, None)
    k = k0 + sum(APPENDS)
    in_set = w["j"] >= off
    assert (k0 == K0_MAX) == bool(in_set.all())
    idx = np.where(in_set, w["j"] - off, NONE).astype(np.uint32)
    closed = w["want"] & in_set.astype(np.uint8)
    assert 0 < closed.sum() < N
    with _grow(engine, scheme, P0, P1, k0, APPENDS, form, k + 5) as grown, engine.KeySet(scheme, P0, P1) as whole:
        assert grown.k == whole.k == k
        assert (grown.key_ok() == whole.key_ok()).all() and (whole.key_ok() == 1).all()
        for key in range(k0, k):
            for point in range(1 if scheme == "single" else 2):
                for window in (0, 15, 31):
                    for digit in (-128, -1, 1, 128):
                        a = grown.debug_entry(key, point, window, digit)
                        b = whole.debug_entry(key, point, window, digit)
                        assert (a == b).all(), (key, point, window, digit)
        got, ref = _keyed_calls(engine, grown, w, idx), _keyed_calls(engine, whole, w, idx)
        for name in ref:
            want = w["want"] if name == "open" else closed
            assert (ref[name] == want).all(), (name, "built at once", _diff(ref[name], want))
            assert (got[name] == want).all(), (name, "appended", _diff(got[name], want))


def test_appended_typed_objects(engine):
    """append_mont_cols and verify_mont_dev: key objects appended to a reserved double set, signature objects
    verified by key index"""
    scheme, k0 = "double", 1
    w = _world(engine, scheme, K0_MAX + sum(APPENDS), 4100 + len(scheme))
    off = K0_MAX - k0
    P0, P1 = _sl(w["P0"], off, None), _sl(w["P1"], off, None)
    in_set = w["j"] >= off
    idx = np.where(in_set, w["j"] - off, NONE).astype(np.uint32)
    closed = w["want"] & in_set.astype(np.uint8)
    rng = np.random.default_rng(9)
    limbs = [MC.to_limbs_py(w["u"], M.R_ORDER)] + [MC.to_limbs_py(H.projective(p, rng)[0], Q) for p in _pts(w)]
    args = _dev(limbs + [idx, MC.to_limbs_py(w["m"], Q)])
    with _grow(engine, scheme, P0, P1, k0, APPENDS, "mont_cols", len(P0)) as grown, \
            engine.KeySet(scheme, P0, P1) as whole:
        assert (grown.key_ok() == 1).all()
        for ks in (grown, whole):
            ok = _poison(N)
            ws = torch.empty(engine.keyed_mont_workspace_bytes(scheme, N), dtype=torch.uint8, device=DEV)
            ks.verify_mont_dev(*args, ok, ws)
            torch.cuda.synchronize()
            got = ok.cpu().numpy()
            assert (got == closed).all(), _diff(got, closed)


# ---- 2. the index across appends ----------------------------------------------------------------------------
def test_index_across_appends(engine):
    """capacity 40: 128 slots.  One cluster holds keys of the constructor and of an appended batch, another wraps
    from slot 127 to slot 0; a key appended again keeps its old index, a key given twice in one append gets the
    lower one, an appended key with a coordinate >= q or off the curve is recorded with key_ok = 0 and its bytes
    miss"""
    capacity, cap = 40, 128
    _, _, C, _ = _keys(engine, "single", 900, 20261019)
    homes = np.array([engine.keyset_home_slot("single", capacity, C[i]) for i in range(len(C))])
    assert (homes < cap).all()
    counts = np.bincount(homes[(homes > 4) & (homes < cap - 8)], minlength=cap)
    h = int(np.argmax(counts))
    cluster = np.flatnonzero(homes == h)[:4]      # about 7 of 900 share the fullest home slot
    wrap = np.flatnonzero(homes >= cap - 2)[:6]   # about 14 of 900 are at home in the last two slots
    assert len(cluster) == 4 and len(wrap) == 6
    others = np.setdiff1d(np.flatnonzero((homes < cap - 8) & (homes != h)), cluster)[:12]
    first = np.concatenate([cluster[:2], wrap[:3], others[:4]])                    # 9 keys, the constructor's
    batch = np.concatenate([cluster[2:], wrap[3:], others[4:8], others[4:5], first[:1]])   # 11 keys: one twice,
    P_first, P_batch = np.ascontiguousarray(C[first]), np.ascontiguousarray(C[batch])      # one registered already
    bad = np.ascontiguousarray(C[others[8:10]])
    bad[0, :32] = _le(M.from_le(bad[0, :32]) + Q)   # the same residue, not canonical
    bad[1, 40] ^= 1
    assert not M.on_curve(H.to_int_point(bad[1]))
    P_batch = np.ascontiguousarray(np.concatenate([P_batch, bad]))
    allkeys = np.ascontiguousarray(np.concatenate([P_first, P_batch]))
    with engine.KeySet.reserved("single", capacity, P_first) as ks:
        st = ks.index_stats()
        assert st["capacity"] == cap and st["occupied"] == 9
        assert ks.append(P_batch) == 9 and ks.k == 22 == len(allkeys)
        kok = ks.key_ok()
        assert (kok[:20] == 1).all() and (kok[20:] == 0).all()
        where = _where(allkeys, None, kok)
        want = _expect(where, allkeys, None)
        assert want[19] == 0                    # registered already: its old index
        assert want[18] == 9 + 2 + 3 == want[14]   # given twice in one append: the lower index
        assert (want[20:] == NONE).all()        # invalid keys: never inserted
        assert (want[:18] == np.arange(18)).all()
        got = _check_lookup(ks, where, allkeys, None, "after the append")
        assert (got == want).all()
        st = ks.index_stats()
        assert st["capacity"] == cap and st["occupied"] == len(where) == 18
        assert 2 <= st["longest_probe"] <= ks.k and st["displaced"] >= 3 + 2, st
        # a second append into the same clusters: more of the wrap keys' neighbours
        more = np.ascontiguousarray(C[np.setdiff1d(np.flatnonzero(homes >= cap - 2), wrap)[:3]])
        if len(more):
            assert ks.append(more) == 22
            allkeys = np.ascontiguousarray(np.concatenate([allkeys, more]))
            where = _where(allkeys, None, ks.key_ok())
            _check_lookup(ks, where, allkeys, None, "after the second append")
            st = ks.index_stats()
            assert st["occupied"] == len(where) and st["longest_probe"] <= ks.k


# ---- 3. a full set --------------------------------------------------------------------------------------------
def test_append_past_capacity_changes_nothing(engine):
    from schnorr_amd import _lib

    w = _world(engine, "single", 16, 77)
    P0 = w["P0"]
    idx = np.where(w["j"] < 10, w["j"], NONE).astype(np.uint32)
    closed = w["want"] & (w["j"] < 10).astype(np.uint8)
    args = _dev([w["u"], w["R"], idx, w["m"]])

    def state(ks):
        ok = _poison(N)
        ws = torch.empty(engine.keyed_workspace_bytes(N), dtype=torch.uint8, device=DEV)
        ks.verify_dev(*args, ok, ws)
        torch.cuda.synchronize()
        return ks.k, ks.key_ok().tolist(), ks.lookup(np.ascontiguousarray(P0))[0].tolist(), ok.cpu().numpy().tolist()

    with engine.KeySet.reserved("single", 12, _sl(P0, 0, 10)) as ks:
        before = state(ks)
        assert before[0] == 10 and before[2] == list(range(10)) + [NONE] * 6 and before[3] == closed.tolist()
        with pytest.raises(_lib.DsvError, match=TOO_LARGE):
            ks.append(_sl(P0, 10, 13))  # 10 + 3 > 12
        assert state(ks) == before
        # key_ok with less room than keys: `room` bytes written and no more, the k they belong to reported
        buf = np.full(16, POISON, np.uint8)
        seen = ctypes.c_size_t(99)
        rc = _lib.load().dsv_keyset_key_ok_n(ks._h, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(4),
                                             ctypes.byref(seen))
        assert rc == 0 and seen.value == 10 and (buf[:4] == 1).all() and (buf[4:] == POISON).all()
        assert ks.append(_sl(P0, 10, 12)) == 10 and ks.k == 12  # exactly full
        assert len(ks.key_ok()) == 12
        with pytest.raises(_lib.DsvError, match=TOO_LARGE):
            ks.append(_sl(P0, 12, 13))
        assert ks.append(_sl(P0, 0, 0)) == 12  # nothing appended: DSV_OK
    with engine.KeySet("single", _sl(P0, 0, 10)) as plain:
        assert plain.capacity == plain.k == 10
        before = state(plain)
        with pytest.raises(_lib.DsvError, match=TOO_LARGE):
            plain.append(_sl(P0, 10, 11))
        assert state(plain) == before


# ---- 4. the stale-k rule: a captured graph keeps the k of its capture ----------------------------------------
@pytest.mark.parametrize("scheme", ("single", "double"))
def test_captured_graph_keeps_its_k(engine, scheme):
    """a graph over the open-set and the closed-set call by key value, captured when the set held 8 of the batch's
    16 keys.  Replayed after the other 8 were appended it must decide as before: the lookup reads the newer keys'
    slots as empty, so the open call still sends their items down the unkeyed path (without the guard they would
    come back from the keyed kernel with index >= k and verdict 0, and never reach the miss list), and the closed
    call still rejects them.  A call enqueued after the append decides them by the tables."""
    k0 = 8
    w = _world(engine, scheme, 16, 88 + len(scheme))
    newer = w["j"] >= k0
    want_open, want_closed = w["want"], w["want"] & (~newer).astype(np.uint8)
    assert 0 < want_open[newer].sum() < newer.sum() and 0 < want_closed.sum()
    args = _dev([w["u"]] + _pts(w) + _key_cols(w) + [w["m"]])
    with engine.KeySet.reserved(scheme, 16, _sl(w["P0"], 0, k0), _sl(w["P1"], 0, k0)) as ks:
        ok_o, ok_c = _poison(N), _poison(N)
        ws_o = torch.empty(engine.keyed_open_workspace_bytes(N), dtype=torch.uint8, device=DEV)
        ws_c = torch.empty(engine.keyed_lookup_workspace_bytes(N), dtype=torch.uint8, device=DEV)
        miss_o = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        miss_c = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.verify_open_dev(*args, ok_o, ws_o, misses=miss_o)
            ks.verify_lookup_dev(*args, ok_c, ws_c, misses=miss_c)
        torch.cuda.synchronize()

        def replay(what):
            for t in (ok_o, ok_c):
                t.fill_(POISON)
            for t in (miss_o, miss_c):
                t.fill_(999)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got_o, got_c = ok_o.cpu().numpy(), ok_c.cpu().numpy()
            assert (got_o == want_open).all(), (what, "open", _diff(got_o, want_open))
            assert (got_c == want_closed).all(), (what, "closed", _diff(got_c, want_closed))
            assert int(miss_o.item()) == int(miss_c.item()) == int(newer.sum()), what

        replay("before the append")
        assert ks.append(_sl(w["P0"], k0, 16), *([_sl(w["P1"], k0, 16)] if w["P1"] is not None else [])) == k0
        replay("after the append")
        # a fresh call sees all 16 keys
        for call, ok, ws, ms in ((ks.verify_open_dev, ok_o, ws_o, miss_o), (ks.verify_lookup_dev, ok_c, ws_c, miss_c)):
            ok.fill_(POISON)
            ms.fill_(999)
            call(*args, ok, ws, misses=ms)
            torch.cuda.synchronize()
            got = ok.cpu().numpy()
            assert (got == want_open).all(), _diff(got, want_open)
            assert int(ms.item()) == 0
        del g


# ---- 5. verify calls beside appends ---------------------------------------------------------------------------
def test_verify_open_runs_beside_appends(engine):
    """one thread appends 8 keys one at a time, another issues 32 open-set calls on a stream of its own over a
    batch under all 16 keys, synchronising after each: whatever k a call sees, its verdicts are the unkeyed ones"""
    k0 = 8
    w = _world(engine, "single", 16, 88 + len("single"))
    args = _dev([w["u"], w["R"], w["A"], w["m"]])
    errors, seen = [], []
    with engine.KeySet.reserved("single", 16, _sl(w["P0"], 0, k0)) as ks:
        def appender():
            try:
                for i in range(k0, 16):
                    assert ks.append(_sl(w["P0"], i, i + 1)) == i
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def verifier():
            try:
                torch.cuda.set_device(0)
                st = torch.cuda.Stream(device=DEV)
                ws = torch.empty(engine.keyed_open_workspace_bytes(N), dtype=torch.uint8, device=DEV)
                ms = torch.full((1,), 999, dtype=torch.int32, device=DEV)
                ok = _poison(N)
                st.wait_stream(torch.cuda.current_stream())
                for _ in range(32):
                    ks.verify_open_dev(*args, ok, ws, misses=ms, stream=st)
                    st.synchronize()
                    seen.append((ok.cpu().numpy().copy(), int(ms.item())))
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        torch.cuda.synchronize()
        threads = [threading.Thread(target=verifier), threading.Thread(target=appender)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert ks.k == 16 and len(seen) == 32
        per_key = np.bincount(w["j"], minlength=16)
        allowed = {int(per_key[k:].sum()) for k in range(k0, 17)}  # the misses of a call that saw k keys
        for got, misses in seen:
            assert (got == w["want"]).all(), _diff(got, w["want"])
            assert misses in allowed, (misses, sorted(allowed))
