"""Key sets as a key cache on the GPU (dsv_verify_keyed_open*, dsv_verify_vargen_keyed_open*): the open-set form of
verify by key value, for all three schemes (KeySet.verify_open[_dev] for single and double keys,
KeySet.verify_vargen_open[_dev] for (PK, Gen) pairs; keyed_cases.OPEN holds what differs).  The expected verdict is
always the CPU oracle's on the item's own key bytes — registering a key never changes it — and `misses` is the count
of a Python dict over the registered keys' bytes.  Keys and items come from tests/keyed_cases.py; every test checks
the _dev form (ok and the counter poisoned first) and the host form."""
import ctypes

import numpy as np
import pytest
import torch

import edge_sets as ES
import harness as H
import pymodel as M
from keyed_cases import (OPEN, SCHEMES, _dev, _diff, _expect, _keys, _open_dev, _oracle, _poison, _scalars, _sign_items,
                         _value_args, _value_batch, _where)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
NONE = 0xFFFFFFFF
INVALID = -2
S = "vargen"
SECOND_KEY = {"single": None, "double": "PKp", "vargen": "Gen"}  # the second key column's name in edge_sets.FIELDS
TOP = np.full(32, 0xFF, np.uint8)


def _check(engine, ks, args, want, nmiss, what):
    got, misses = _open_dev(engine, ks, args)
    assert (got == want).all(), (what, "dev", _diff(got, want))
    assert misses == nmiss, (what, "dev", misses, nmiss)
    got, misses = getattr(ks, OPEN[ks.scheme]["open"])(*args)
    assert (got == want).all(), (what, "host", _diff(got, want))
    assert misses == nmiss, (what, "host", misses, nmiss)


def _verdicts(scheme, u, R, Rp, A, B, m):
    return np.asarray(_oracle(scheme, u, R, Rp, A, B, m)).astype(np.uint8)


# ---- items that exist twice: under a registered key and under an unregistered one ----------------------------
_DUAL = {}
DUAL_KEYS = 8


def _dual(engine, scheme, n, seed):
    """position i signed twice over the same m: version 0 under one of DUAL_KEYS keys that tests register, version
    1 under one of as many that they do not; of each version a wrong signature too (a bit of u flipped).  The
    oracle's verdicts on all four, computed once."""
    key = (scheme, n, seed)
    if key in _DUAL:
        return _DUAL[key]
    k = DUAL_KEYS
    sk, gen, K0, K1 = _keys(engine, scheme, 2 * k, seed)
    rng = np.random.default_rng(seed + 1)
    idx = rng.integers(0, k, size=n)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    ver = []
    for v in (0, 1):
        j = idx + v * k
        u, R, Rp = _sign_items(engine, scheme, sk[j], gen[j] if gen is not None else None, m, r)
        ub = u.copy()
        ub[:, 0] ^= 8
        A = K0[j].copy()
        B = K1[j].copy() if K1 is not None else None
        good, bad = _verdicts(scheme, u, R, Rp, A, B, m), _verdicts(scheme, ub, R, Rp, A, B, m)
        assert good.all() and not bad.any()
        ver.append({"u": u, "ub": ub, "R": R, "Rp": Rp, "A": A, "B": B, "good": good, "bad": bad})
    out = {"scheme": scheme, "n": n, "m": m, "ver": ver,
           "P0": np.ascontiguousarray(K0[:k]), "P1": np.ascontiguousarray(K1[:k]) if K1 is not None else None,
           "X0": np.ascontiguousarray(K0[k:]), "X1": np.ascontiguousarray(K1[k:]) if K1 is not None else None}
    _DUAL[key] = out
    return out


def _pick(d, miss, wrong):
    """the batch in which position i is the unregistered version where miss[i] and a wrong signature where
    wrong[i] -> (host arrays in entry-point order, the oracle's verdicts)"""
    v0, v1 = d["ver"]
    sel = lambda name: np.ascontiguousarray(np.where(miss[:, None], v1[name], v0[name]))
    u = np.ascontiguousarray(np.where(wrong[:, None], sel("ub"), sel("u")))
    has = OPEN[d["scheme"]]
    args = [u, sel("R")] + ([sel("Rp")] if has["Rp"] else []) + [sel("A")] + ([sel("B")] if has["B"] else []) + [d["m"]]
    want = np.where(wrong, np.where(miss, v1["bad"], v0["bad"]), np.where(miss, v1["good"], v0["good"]))
    return args, want.astype(np.uint8)


def _three_of(rng, positions):
    """three of the positions, or none when the group is too small to lose three and still show both verdicts"""
    out = np.zeros(0, dtype=np.int64)
    if len(positions) >= 6:
        out = rng.choice(positions, size=3, replace=False)
    return out


# ---- 1. parity with the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, 4099))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_parity(engine, scheme, n):
    """_value_batch: every 16th item tampered, some key rows become other registered keys, some leave the set;
    the last four of its 33 keys are registered as other keys, so honest items miss as well"""
    b = _value_batch(engine, scheme)
    k = len(b["P0"])
    _, _, Y0, Y1 = _keys(engine, scheme, 4, 8080)
    P0, P1 = b["P0"].copy(), b["P1"].copy() if b["P1"] is not None else None
    P0[k - 4:] = Y0
    if P1 is not None:
        P1[k - 4:] = Y1
    with engine.KeySet(scheme, P0, P1) as ks:
        assert ks.k == 33
        where = _where(P0, P1, ks.key_ok())
        idx = _expect(where, b["A"][:n], b["B"][:n] if b["B"] is not None else None)
        miss = idx == NONE
        want = np.asarray(b["oracle"][:n]).astype(np.uint8)
        if n == 4099:
            assert miss.any() and (~miss).any()
            assert 0 < want[miss].sum() < miss.sum() and 0 < want[~miss].sum() < (~miss).sum()
        _check(engine, ks, _value_args(b, n), want, int(miss.sum()), (scheme, n))


# ---- 2. the meaning ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ("single", "vargen"))
def test_open_accepts_a_valid_signature_under_an_unregistered_key(engine, scheme):
    """the open-set meaning, on the set and the items of the closed-set test: the unkeyed verdict is 1, the key is
    not in the set — verify_lookup says 0, the open form says 1"""
    sk, gen, P0, P1 = _keys(engine, scheme, 5, 2024)
    rng = np.random.default_rng(1)
    n = 40
    idx = rng.integers(0, 5, size=n)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, Rp = _sign_items(engine, scheme, sk[idx], gen[idx] if gen is not None else None, m, r)
    args = [u, R] + ([Rp] if Rp is not None else []) + [P0[idx]] + ([P1[idx]] if P1 is not None else []) + [m]
    assert (getattr(engine, OPEN[scheme]["unkeyed"])(*args) == 1).all()
    nmiss = int((idx == 4).sum())
    assert nmiss > 0
    first4 = lambda P: np.ascontiguousarray(P[:4]) if P is not None else None
    with engine.KeySet(scheme, first4(P0), first4(P1)) as ks:
        closed, cm = ks.verify_lookup(*args)
        opened, om = getattr(ks, OPEN[scheme]["open"])(*args)
        dev, dm = _open_dev(engine, ks, args)
    assert (closed == (idx < 4)).all() and cm == nmiss
    assert (opened == 1).all() and om == nmiss
    assert (dev == 1).all() and dm == nmiss


# ---- 3. miss patterns ----------------------------------------------------------------------------------------
def _patterns(n):
    none, every = np.zeros(n, bool), np.ones(n, bool)
    out = {"no_miss": none, "all_miss": every, "every_other": np.arange(n) % 2 == 1}
    for p in (0, 63, 64, n - 1):
        one = none.copy()
        one[p] = True
        out["only_%d" % p] = one
    return out


@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_miss_patterns(engine, scheme):
    n = 193
    d = _dual(engine, scheme, n, 31 + len(scheme))
    rng = np.random.default_rng(5)
    empty = lambda a: a[:0].copy() if a is not None else None
    with engine.KeySet(scheme, d["P0"], d["P1"]) as ks, engine.KeySet(scheme, d["X0"], d["X1"]) as unrelated, \
            engine.KeySet(scheme, empty(d["P0"]), empty(d["P1"])) as nothing:
        assert nothing.k == 0
        for name, miss in _patterns(n).items():
            wrong = np.zeros(n, bool)
            wrong[_three_of(rng, np.flatnonzero(miss))] = True
            wrong[_three_of(rng, np.flatnonzero(~miss))] = True
            args, want = _pick(d, miss, wrong)
            assert want.sum() == n - wrong.sum()
            _check(engine, ks, args, want, int(miss.sum()), (scheme, name))
            if name.startswith("only_"):  # the one miss as a wrong signature too
                wrong = wrong.copy()
                wrong[np.flatnonzero(miss)] = True
                args, want = _pick(d, miss, wrong)
                _check(engine, ks, args, want, 1, (scheme, name, "wrong"))
        # everything misses: through a set of unrelated keys, and through the empty set
        none = np.zeros(n, bool)
        wrong = none.copy()
        wrong[rng.choice(n, size=6, replace=False)] = True
        args, want = _pick(d, none, wrong)  # items under P0 / P1, which neither set holds
        assert want.sum() == n - 6
        _check(engine, unrelated, args, want, n, (scheme, "unrelated"))
        _check(engine, nothing, args, want, n, (scheme, "empty"))


# ---- 4. pairs ------------------------------------------------------------------------------------------------
def test_vargen_open_registered_pk_beside_another_keys_gen(engine):
    """the key is the PAIR: registered key a's PK beside registered key b's Gen is a miss, decided by the unkeyed
    equation on those bytes.  With Gen_j = g_j * G and PK_a = sk_a * Gen_a the secret of PK_a over Gen_b is
    sk_a * g_a / g_b mod r, so the mixed items carry valid signatures as well as wrong ones: a miss that the
    closed-set call rejects and the oracle accepts."""
    k, n = 6, 97
    rng = np.random.default_rng(404)
    sk, g = _scalars(rng, k, 0x07), _scalars(rng, k, 0x07)
    gen = engine.public_keys(g)
    PK = engine.public_keys(sk, Gen=gen)
    a = rng.integers(0, k, size=n)
    b = (a + 1 + rng.integers(0, k - 1, size=n)) % k
    mixed = np.arange(n) % 3 != 0  # the rest: honest items under the pair (a, a)
    b = np.where(mixed, b, a)
    x = np.zeros((n, 32), np.uint8)  # the secret of PK_a over Gen_b
    for i in range(n):
        ska, ga, gb = (M.from_le(v) for v in (sk[a[i]], g[a[i]], g[b[i]]))
        x[i] = np.frombuffer(M.le32(ska * ga * pow(gb, -1, M.R_ORDER) % M.R_ORDER), np.uint8)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    Gb = np.ascontiguousarray(gen[b])
    u, R = engine.sign_vargen(x, Gb, m, r)
    u[np.arange(n) % 5 == 0, 0] ^= 8  # wrong signatures among both kinds
    A = np.ascontiguousarray(PK[a])
    args = [u, R, A, Gb, m]
    want = _verdicts(S, u, R, None, A, Gb, m)
    assert (want == (np.arange(n) % 5 != 0)).all()
    assert 0 < want[mixed].sum() < mixed.sum() and 0 < want[~mixed].sum() < (~mixed).sum()
    with engine.KeySet(S, PK, gen) as ks:
        idx = _expect(_where(PK, gen, ks.key_ok()), A, Gb)
        assert ((idx == NONE) == mixed).all()
        _check(engine, ks, args, want, int(mixed.sum()), "pairs")
        closed, cm = ks.verify_lookup(*args)
        assert (closed == (want & ~mixed)).all() and cm == mixed.sum()


# ---- 5. registered but not usable ----------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_open_registered_but_not_usable(engine, scheme):
    """the adversarial base set (tests/edge_sets.py) with every one of its key rows registered — among them keys
    with a coordinate >= q, the identity, the points of order 2 and 4 and points with a small-order component —
    plus a key off the curve; and items under each.  Invalid keys are never inserted: their items are misses and
    the unkeyed equation rejects them; the valid special points are hits."""
    arrs, base_want = ES.base(scheme, "affine", "mixed")
    d = {f: a.copy() for f, a in zip(ES.FIELDS[scheme], arrs)}
    second = SECOND_KEY[scheme]
    # extra rows from honest items of the base set: a key off the curve, u >= r on a hit, u >= r on a miss
    honest = np.flatnonzero(np.asarray(base_want) == 1)[:3]
    assert len(honest) == 3
    extra = {f: a[honest].copy() for f, a in d.items()}
    off = second or "PK"
    extra[off][0, 40] ^= 1
    assert not M.on_curve(H.to_int_point(extra[off][0]))
    extra["u"][1] = TOP
    _, _, Y0, Y1 = _keys(engine, scheme, 1, 99)  # a valid key that is not registered
    extra["PK"][2] = Y0[0]
    if second:
        extra[second][2] = Y1[0]
    extra["u"][2] = TOP
    d = {f: np.concatenate([d[f], extra[f]]) for f in d}
    args = [d[f] for f in ES.FIELDS[scheme]]
    extra_want = _verdicts(scheme, extra["u"], extra["R"], extra.get("Rp"), extra["PK"], extra.get(second), extra["m"])
    assert not extra_want.any()
    want = np.concatenate([np.asarray(base_want).astype(np.uint8), extra_want])
    # the set: every key row of the batch but the unregistered one
    rows = np.hstack([d["PK"], d[second]]) if second else d["PK"]
    uniq = np.unique(rows[:-1], axis=0)
    P0 = np.ascontiguousarray(uniq[:, :64])
    P1 = np.ascontiguousarray(uniq[:, 64:]) if second else None
    with engine.KeySet(scheme, P0, P1) as ks:
        kok = ks.key_ok()
        where = _where(P0, P1, kok)
        idx = _expect(where, d["PK"], d[second] if second else None)
        miss = idx == NONE
        # what the set holds: invalid keys of both kinds, not inserted; the special points, inserted
        ints = [[H.to_int_point(P[j]) for j in range(len(P0))] for P in ([P0, P1] if second else [P0])]
        canonical = np.array([all(p[j][0] < M.Q and p[j][1] < M.Q for p in ints) for j in range(len(P0))])
        on_curve = np.array([all(M.on_curve(p[j]) for p in ints) for j in range(len(P0))])
        assert (~canonical).any() and (canonical & ~on_curve).any()
        assert (kok == (canonical & on_curve)).all()
        holders = ints if scheme == S else ints[:1]  # a pair holds a special point as PK or as Gen
        for special in (M.IDENTITY, (0, M.Q - 1)):
            at = [j for j in range(len(P0)) if any(p[j] == special for p in holders) and kok[j]]
            assert at, special
            assert any((idx == j).any() for j in at), special
        assert miss[-3] and not miss[-2] and miss[-1]          # off the curve; u >= r on a hit; on a miss
        assert miss.sum() > 3 and 0 < want[~miss].sum() < (~miss).sum()
        _check(engine, ks, args, want, int(miss.sum()), scheme)
    unkeyed = getattr(engine, OPEN[scheme]["unkeyed"])(*args)
    assert (unkeyed == want).all(), _diff(unkeyed, want)


# ---- 6. more misses than one pass of the grid ----------------------------------------------------------------
@pytest.mark.parametrize("scheme", ("single", "vargen"))
def test_open_more_misses_than_one_grid_pass(engine, scheme):
    """2^18 + 65 items, all under unregistered keys: the list is longer than the 4096 x 64 lanes of the launch,
    so the listed kernel's grid-stride loop wraps.  The whole vector against the unkeyed _dev call on the same
    columns, a sample that holds every tampered position against the oracle."""
    n, k = (1 << 18) + 65, DUAL_KEYS
    assert n > 4096 * 64
    sk, gen, K0, K1 = _keys(engine, scheme, 2 * k, 616)
    rng = np.random.default_rng(18)
    idx = k + rng.integers(0, k, size=n)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, _ = _sign_items(engine, scheme, sk[idx], gen[idx] if gen is not None else None, m, r)
    tampered = np.unique(np.concatenate([np.arange(0, n, 4096), [n - 1]]))
    u[tampered, 0] ^= 8
    A = np.ascontiguousarray(K0[idx])
    B = np.ascontiguousarray(K1[idx]) if K1 is not None else None
    dargs = _dev([u, R, A] + ([B] if B is not None else []) + [m])
    ok_u = _poison(n)
    ws_u = torch.empty(engine.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    getattr(engine, OPEN[scheme]["unkeyed"] + "_dev")(*dargs, ok_u, ws_u)
    ok = _poison(n)
    ws = torch.empty(engine.keyed_open_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
    first = lambda P: np.ascontiguousarray(P[:k]) if P is not None else None
    with engine.KeySet(scheme, first(K0), first(K1)) as ks:
        getattr(ks, OPEN[scheme]["open"] + "_dev")(*dargs, ok, ws, misses=misses)
        torch.cuda.synchronize()
    got, unkeyed = ok.cpu().numpy(), ok_u.cpu().numpy()
    assert int(misses.item()) == n
    assert (got == unkeyed).all(), _diff(got, unkeyed)
    rest = np.setdiff1d(np.arange(n), tampered)
    sample = np.sort(np.concatenate([tampered, rng.choice(rest, size=512 - len(tampered), replace=False)]))
    assert len(sample) == 512
    want = _verdicts(scheme, u[sample], R[sample], None, A[sample], B[sample] if B is not None else None, m[sample])
    assert (want == ~np.isin(sample, tampered)).all()
    assert (got[sample] == want).all(), _diff(got[sample], want)


# ---- 7. capture and replay -----------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ("double", "vargen"))
def test_open_capture_and_replay(engine, scheme):
    """one captured call, replayed over inputs overwritten in place whose miss counts differ: the length of the
    list lives on the device, so every replay is exact"""
    n = 4099
    d = _dual(engine, scheme, n, 77)
    rng = np.random.default_rng(6)
    batches = []
    for miss in (np.zeros(n, bool), rng.integers(0, 8, size=n) == 0, np.ones(n, bool)):
        wrong = rng.integers(0, 16, size=n) == 0
        args, want = _pick(d, miss, wrong)
        assert 0 < want.sum() < n
        batches.append((args, want, int(miss.sum())))
    assert batches[0][2] == 0 and 300 < batches[1][2] < 800 and batches[2][2] == n
    with engine.KeySet(scheme, d["P0"], d["P1"]) as ks:
        bufs = _dev(batches[-1][0])  # (captured over the all-miss batch: nothing of it may stick)
        ok = _poison(n)
        ws = torch.empty(engine.keyed_open_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            getattr(ks, OPEN[scheme]["open"] + "_dev")(*bufs, ok, ws, misses=misses)
        torch.cuda.synchronize()
        for args, want, nmiss in batches:
            for buf, a in zip(bufs, _dev(args)):
                buf.copy_(a)
            ok.fill_(POISON)
            misses.fill_(999)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = ok.cpu().numpy()
            assert (got == want).all(), (nmiss, _diff(got, want))
            assert int(misses.item()) == nmiss
        del g


# ---- 8. append: the stale-k rule -----------------------------------------------------------------------------
def test_vargen_open_captured_graph_keeps_its_k(engine):
    """a graph over the open call, captured when a reserved set held 8 of the batch's 16 pairs.  Replayed after
    the other 8 were appended it decides as before — the lookup reads the newer keys' slots as empty, their items
    still take the unkeyed path, `misses` is the count at capture — and a fresh call reports the smaller count
    with the same verdicts.  (tests/test_gpu_keyset_append.py pins the same rule for single and double sets.)"""
    n, k0 = 1031, DUAL_KEYS
    d = _dual(engine, S, n, 88)
    rng = np.random.default_rng(9)
    miss, wrong = rng.integers(0, 2, size=n) == 0, rng.integers(0, 16, size=n) == 0
    args, want = _pick(d, miss, wrong)  # `miss`: under the pairs that are appended later
    assert 0 < want[miss].sum() < miss.sum() and 0 < want[~miss].sum() < (~miss).sum()
    dargs = _dev(args)
    with engine.KeySet.reserved(S, 2 * k0, d["P0"], d["P1"]) as ks:
        assert ks.k == k0
        ok = _poison(n)
        ws = torch.empty(engine.keyed_open_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.verify_vargen_open_dev(*dargs, ok, ws, misses=misses)
        torch.cuda.synchronize()

        def replay(what):
            ok.fill_(POISON)
            misses.fill_(999)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got = ok.cpu().numpy()
            assert (got == want).all(), (what, _diff(got, want))
            assert int(misses.item()) == int(miss.sum()), what

        replay("before the append")
        assert ks.append(d["X0"], d["X1"]) == k0 and ks.k == 2 * k0
        replay("after the append")
        _check(engine, ks, args, want, 0, "a fresh call")  # sees all 16 pairs
        del g


# ---- 9. the contract -----------------------------------------------------------------------------------------
def _two_calls_in_flight(engine, scheme):
    """two streams, one set, two calls in flight together, each with its own workspace: both exact"""
    big = 4099
    d = _dual(engine, scheme, big, 77)
    rng = np.random.default_rng(12)
    calls = []
    with engine.KeySet(scheme, d["P0"], d["P1"]) as shared:
        for share in (8, 2):
            miss, wrong = rng.integers(0, share, size=big) == 0, rng.integers(0, 16, size=big) == 0
            args, want = _pick(d, miss, wrong)
            calls.append((_dev(args), want, int(miss.sum()), torch.cuda.Stream(device=DEV), _poison(big),
                          torch.empty(engine.keyed_open_workspace_bytes(big), dtype=torch.uint8, device=DEV),
                          torch.full((1,), 999, dtype=torch.int32, device=DEV)))
        torch.cuda.synchronize()
        for _ in range(3):
            for dargs, want, nmiss, st, o, w, ms in calls:
                getattr(shared, OPEN[scheme]["open"] + "_dev")(*dargs, o, w, misses=ms, stream=st)
        torch.cuda.synchronize()
        for dargs, want, nmiss, st, o, w, ms in calls:
            got = o.cpu().numpy()
            assert (got == want).all(), _diff(got, want)
            assert int(ms.item()) == nmiss > 0


def test_open_dev_contract(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    b = _value_batch(engine, "double")
    n = 65
    du, dR, dRp, dA, dB, dm = _dev(_value_args(b, n))
    vp, sz, null = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p(None)
    p = lambda t: vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    ws_bytes = engine.keyed_open_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ks = engine.KeySet("double", b["P0"], b["P1"])
    try:
        h = ks._h

        def verify(nn, okt, wsb, Rp=p(dRp), key_a=p(dA), key_b=p(dB)):
            return L.dsv_verify_keyed_open_dev(h, p(du), p(dR), Rp, key_a, key_b, p(dm), sz(nn), p(okt), p(ws),
                                               sz(wsb), stream, null)

        ok = _poison(n)
        assert verify(n, ok, ws_bytes - 1) == INVALID
        assert b"workspace" in L.dsv_last_error()
        assert verify(n, ok, ws_bytes, key_b=null) == INVALID
        assert verify(n, ok, ws_bytes, Rp=null) == INVALID
        odd = torch.zeros(n * 64 + 8, dtype=torch.uint8, device=DEV)[8:].view(n, 64)  # 8 bytes off a 16-byte boundary
        assert verify(n, ok, ws_bytes, key_a=p(odd)) == INVALID
        assert b"aligned" in L.dsv_last_error()
        with pytest.raises(ValueError):
            ks.verify_open_dev(du, dR, dRp, odd, dB, dm, ok, ws)
        with pytest.raises(ValueError):
            ks.verify_open_dev(du, dR, dRp, dA, dB, dm, ok, ws[:-1])
        with pytest.raises(ValueError):
            ks.verify_open_dev(du, dR, dA, dB, dm, ok, ws)  # single arguments on a double key set
        # n = 0: DSV_OK, nothing touched (no workspace needed)
        assert verify(0, ok, 0) == 0
        hm = sz(55)
        assert L.dsv_verify_keyed_open(h, null, null, null, null, null, null, sz(0), null, ctypes.byref(hm)) == 0
        assert hm.value == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        # the full workspace: the verdicts
        assert verify(n, ok, ws_bytes) == 0, L.dsv_last_error().decode()
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == np.asarray(b["oracle"][:n]).astype(np.uint8)).all()
        # a var-generator set has no open form
        _, gen, V0, V1 = _keys(engine, "vargen", 3, 5)
        with engine.KeySet("vargen", V0, V1) as vs:
            ok = _poison(n)
            rc = L.dsv_verify_keyed_open_dev(vs._h, p(du), p(dR), null, p(dA), p(dB), p(dm), sz(n), p(ok), p(ws),
                                             sz(ws_bytes), stream, null)
            assert rc == INVALID and b"var-generator" in L.dsv_last_error()
            with pytest.raises(_lib.DsvError, match="var-generator"):
                vs.verify_open(b["u"][:n], b["R"][:n], b["A"][:n], b["B"][:n], b["m"][:n])
            torch.cuda.synchronize()
            assert (ok.cpu().numpy() == POISON).all()
        _two_calls_in_flight(engine, "double")
    finally:
        ks.close()
    # a closed set has no handle left to call with
    with pytest.raises(ValueError):
        ks.verify_open(*_value_args(b, n))
    with pytest.raises(ValueError):
        ks.verify_open_dev(du, dR, dRp, dA, dB, dm, _poison(n), ws)


def test_vargen_open_dev_contract(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    b = _value_batch(engine, S)
    n = 65
    host = _value_args(b, n)
    du, dR, dA, dB, dm = _dev(host)
    vp, sz, null = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p(None)
    p = lambda t: vp(t.data_ptr())
    stream = vp(torch.cuda.current_stream().cuda_stream)
    ws_bytes = engine.keyed_open_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ks = engine.KeySet(S, b["P0"], b["P1"])
    try:
        def verify(h, nn, okt, wsb, PK=p(dA), Gen=p(dB)):
            return L.dsv_verify_vargen_keyed_open_dev(h, p(du), p(dR), PK, Gen, p(dm), sz(nn), p(okt), p(ws), sz(wsb),
                                                      stream, null)

        h = ks._h
        ok = _poison(n)
        assert verify(h, n, ok, ws_bytes - 1) == INVALID
        assert b"workspace" in L.dsv_last_error()
        assert verify(h, n, ok, ws_bytes, Gen=null) == INVALID
        odd = torch.zeros(n * 64 + 8, dtype=torch.uint8, device=DEV)[8:].view(n, 64)  # 8 bytes off a 16-byte boundary
        for kw in ({"PK": p(odd)}, {"Gen": p(odd)}):
            assert verify(h, n, ok, ws_bytes, **kw) == INVALID
            assert b"aligned" in L.dsv_last_error()
        with pytest.raises(ValueError):
            ks.verify_vargen_open_dev(du, dR, dA, odd, dm, ok, ws)
        with pytest.raises(ValueError):
            ks.verify_vargen_open_dev(du, dR, dA, dB, dm, ok, ws[:-1])
        with pytest.raises(ValueError):
            ks.verify_vargen_open_dev(du, dR, dA, dm, ok, ws)  # single arguments
        with pytest.raises(ValueError):
            ks.verify_vargen_open(*host[:-1])
        # a single or a double set: refused, nothing launched, the message names the call that takes them
        _, _, S0, _ = _keys(engine, "single", 3, 5)
        _, _, D0, D1 = _keys(engine, "double", 3, 5)
        with engine.KeySet("single", S0) as one, engine.KeySet("double", D0, D1) as two:
            for other in (one, two):
                assert verify(other._h, n, ok, ws_bytes) == INVALID
                assert b"dsv_verify_keyed_open" in L.dsv_last_error()
                hm = sz(55)
                rc = L.dsv_verify_vargen_keyed_open(other._h, *[vp(a.ctypes.data) for a in host], sz(n), null,
                                                    ctypes.byref(hm))
                assert rc == INVALID and b"dsv_verify_keyed_open" in L.dsv_last_error() and hm.value == 55
                with pytest.raises(_lib.DsvError, match="dsv_verify_keyed_open"):
                    other.verify_vargen_open(*host)
        # n = 0: DSV_OK, nothing touched (no workspace needed)
        assert verify(h, 0, ok, 0) == 0
        hm = sz(55)
        assert L.dsv_verify_vargen_keyed_open(h, null, null, null, null, null, sz(0), null, ctypes.byref(hm)) == 0
        assert hm.value == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        # the full workspace: the verdicts
        assert verify(h, n, ok, ws_bytes) == 0, L.dsv_last_error().decode()
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == np.asarray(b["oracle"][:n]).astype(np.uint8)).all()
        _two_calls_in_flight(engine, S)
    finally:
        ks.close()
    # a closed set has no handle left to call with
    with pytest.raises(ValueError):
        ks.verify_vargen_open(*host)
    with pytest.raises(ValueError):
        ks.verify_vargen_open_dev(du, dR, dA, dB, dm, _poison(n), ws)
