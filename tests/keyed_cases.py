"""Builders and runners the key-set GPU suites share (tests/test_gpu_keyset*.py, test_gpu_keyed_*.py): keys and
items signed through the engine, the CPU oracle's verdicts on them (computed once per batch and cached here, in the
one copy of this module every suite imports), the dict models of the lookups, device copies and poisoned outputs.
Child processes of those suites import this module too."""
import numpy as np
import torch

import edge_sets as ES
import harness as H
import mont_cases as MC
import oracle_lib as O
import pymodel as M

DEV = "cuda:0"
POISON = 7
NONE = 0xFFFFFFFF
SCHEMES = ("single", "double", "vargen")
Q, R_ORDER = M.Q, M.R_ORDER


# ---- keys, items and the oracle (tests/test_gpu_keyset.py) --------------------------------------------------
def _scalars(rng, n, top_mask):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= top_mask
    return s


def _keys(engine, scheme, k, seed):
    """(PK, second point or None) of k random keys: PK' for double, Gen for var-generator; and the secrets"""
    rng = np.random.default_rng(seed)
    sk = _scalars(rng, k, 0x07)  # < 2^251 < r
    if scheme == "single":
        return sk, None, engine.public_keys(sk), None
    if scheme == "double":
        return sk, None, engine.public_keys(sk, 0), engine.public_keys(sk, 1)
    gen = engine.public_keys(_scalars(rng, k, 0x07))
    return sk, gen, engine.public_keys(sk, Gen=gen), gen


def _sign_items(engine, scheme, sk, gen, m, r):
    """(u, R, Rp or None)"""
    if scheme == "single":
        return engine.sign_single(sk, m, r) + (None,)
    if scheme == "double":
        return engine.sign_double(sk, m, r)
    return engine.sign_vargen(sk, gen, m, r) + (None,)


def _oracle(scheme, u, R, Rp, P0, P1, m):
    if scheme == "single":
        return O.verify_single(u, R, P0, m, nthreads=16)
    if scheme == "double":
        return O.verify_double(u, R, Rp, P0, P1, m, nthreads=16)
    return O.verify_vargen(u, R, P0, P1, m, nthreads=16)


_BATCHES = {}


def _batch(engine, scheme, k, n, seed=0):
    """n items signed under k keys (uniform indices), every 16th tampered (harness.tamper) -> dict with the key
    arrays P0 / P1, the items u, R, Rp, idx, m and the oracle's verdicts on the gathered keys"""
    key = (scheme, k, n, seed)
    if key in _BATCHES:
        return _BATCHES[key]
    sk, gen, P0, P1 = _keys(engine, scheme, k, 1000 * k + 7 + seed)
    rng = np.random.default_rng(k * 31 + n + seed)
    idx = rng.integers(0, k, size=n).astype(np.uint32)
    m = _scalars(rng, n, 0x3F)   # < 2^254 < q
    r = _scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = engine.sign_single(sk[idx], m, r)
    elif scheme == "double":
        u, R, Rp = engine.sign_double(sk[idx], m, r)
    else:
        u, R = engine.sign_vargen(sk[idx], gen[idx], m, r)
    b = {"u": u, "R": R, "PK": P0[idx].copy(), "m": m}
    H.tamper(b, kind_single=scheme == "single", period=16)
    # a tampered PK row that is another registered key becomes that key's index; any other stays the row's key
    where = {P0[j].tobytes(): j for j in range(k)}
    changed = np.flatnonzero((b["PK"] != P0[idx]).any(axis=1))
    for i in changed:
        idx[i] = where.get(b["PK"][i].tobytes(), idx[i])
    g1 = P1[idx] if P1 is not None else None
    want = _oracle(scheme, b["u"], b["R"], Rp, P0[idx], g1, b["m"])
    out = {"P0": P0, "P1": P1, "u": b["u"], "R": b["R"], "Rp": Rp, "idx": idx, "m": b["m"], "want": want}
    if len(_BATCHES) > 4:
        _BATCHES.pop(next(iter(_BATCHES)))
    _BATCHES[key] = out
    return out


def _items(b, lo=0, hi=None):
    """(u, R[, Rp], idx, m) host arrays of items [lo, hi)"""
    s = slice(lo, hi)
    pts = [b["R"][s]] + ([b["Rp"][s]] if b["Rp"] is not None else [])
    return [b["u"][s]] + pts + [b["idx"][s], b["m"][s]]


def _dev(arrs):
    out = []
    for a in arrs:
        t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a))
        out.append(t.to(DEV))
    return out


def _to_dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)


def _poison(n):
    return torch.full((n,), POISON, dtype=torch.uint8, device=DEV)


def _run_dev(engine, ks, darrs, n, stream=None):
    ok = _poison(n)
    ws = torch.empty(max(engine.keyed_workspace_bytes(n), 1), dtype=torch.uint8, device=DEV)
    ks.verify_dev(*[a[:n] for a in darrs], ok, ws, stream=stream)
    torch.cuda.synchronize()
    return ok.cpu().numpy()


def _diff(got, want):
    got, want = [np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (got, want)]
    bad = np.flatnonzero(got != want)
    return "%d verdicts differ, first at %s (got %s, want %s)" % (
        len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def _keyset(engine, scheme, b):
    return engine.KeySet(scheme, b["P0"], b["P1"])


# ---- lookups by key value: a dict over the bytes of the valid registered keys, lowest index first -----------
# (tests/test_gpu_keyset_lookup.py)
def _row(A, B, i):
    return A[i].tobytes() + (B[i].tobytes() if B is not None else b"")


def _where(P0, P1, key_ok):
    d = {}
    for j in range(len(P0)):
        if key_ok[j]:
            d.setdefault(_row(P0, P1, j), j)
    return d


def _expect(where, A, B):
    return np.array([where.get(_row(A, B, i), NONE) for i in range(len(A))], dtype=np.uint32)


def _lookup_dev(ks, A, B, stream=None):
    """(idx uint32 [n], misses) through KeySet.lookup_dev, idx and the counter poisoned first"""
    cols = _dev([A] + ([B] if B is not None else []))
    out = torch.full((len(A),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    misses = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    ks.lookup_dev(*cols, out, misses=misses, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), int(misses.item())


def _check_lookup(ks, where, A, B, what):
    want = _expect(where, A, B)
    nmiss = int((want == NONE).sum())
    got, misses = _lookup_dev(ks, A, B)
    assert (got == want).all(), (what, "dev", _diff(got, want))
    assert misses == nmiss, (what, "dev", misses, nmiss)
    got, misses = ks.lookup(*([A] + ([B] if B is not None else [])))
    assert (got == want).all(), (what, "host", _diff(got, want))
    assert misses == nmiss, (what, "host", misses, nmiss)
    return want


def _le(x):
    return np.frombuffer(M.le32(x), np.uint8)


_VALUE_BATCHES = {}


def _value_batch(engine, scheme, k=33, n=4099):
    """n items signed under k keys, every 16th tampered (harness.tamper: some key rows become other registered
    keys, some leave the set) -> the key arrays, the items with their own key columns, the oracle's verdicts on
    those key bytes, computed once per scheme"""
    if scheme in _VALUE_BATCHES:
        return _VALUE_BATCHES[scheme]
    sk, gen, P0, P1 = _keys(engine, scheme, k, 1000 * k + 11)
    rng = np.random.default_rng(k * 37 + n)
    idx = rng.integers(0, k, size=n)
    m = _scalars(rng, n, 0x3F)
    r = _scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = engine.sign_single(sk[idx], m, r)
    elif scheme == "double":
        u, R, Rp = engine.sign_double(sk[idx], m, r)
    else:
        u, R = engine.sign_vargen(sk[idx], gen[idx], m, r)
    b = {"u": u, "R": R, "PK": P0[idx].copy(), "m": m}
    H.tamper(b, kind_single=scheme == "single", period=16)
    B = P1[idx].copy() if P1 is not None else None
    oracle = _oracle(scheme, b["u"], b["R"], Rp, b["PK"], B, b["m"])
    out = {"P0": P0, "P1": P1, "u": b["u"], "R": b["R"], "Rp": Rp, "A": b["PK"], "B": B, "m": b["m"],
           "oracle": oracle}
    _VALUE_BATCHES[scheme] = out
    return out


def _value_args(b, n):
    pts = [b["R"][:n]] + ([b["Rp"][:n]] if b["Rp"] is not None else [])
    keys = [b["A"][:n]] + ([b["B"][:n]] if b["B"] is not None else [])
    return [b["u"][:n]] + pts + keys + [b["m"][:n]]


# ---- the open-set calls: what differs between the schemes (tests/test_gpu_keyset_open.py) -------------------
# open: the KeySet method of the host form (the _dev form is the same name + "_dev"); unkeyed: the engine's call
# on the same columns (likewise); Rp / B: whether a second nonce point / a second key column exists
OPEN = {"single": {"open": "verify_open", "unkeyed": "verify_single", "Rp": False, "B": False},
        "double": {"open": "verify_open", "unkeyed": "verify_double", "Rp": True, "B": True},
        "vargen": {"open": "verify_vargen_open", "unkeyed": "verify_vargen", "Rp": False, "B": True}}


def _open_dev(engine, ks, args, stream=None):
    """(verdicts, misses) through the scheme's KeySet.verify_*open_dev, ok and the counter poisoned first"""
    n = len(args[0])
    ok = _poison(n)
    ws = torch.empty(engine.keyed_open_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
    getattr(ks, OPEN[ks.scheme]["open"] + "_dev")(*_dev(args), ok, ws, misses=misses, stream=stream)
    torch.cuda.synchronize()
    return ok.cpu().numpy(), int(misses.item())


# ---- serialized records (tests/test_gpu_keyed_wire.py, test_gpu_keyset_open_wire.py) ------------------------
def _sig(u, R, Rp=None):
    """Signature*::to_bytes: u, then the nonce points compressed"""
    cols = [u, O.compress(R)] + ([O.compress(Rp)] if Rp is not None else [])
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def _key_records(P0, P1):
    """PublicKey*::to_bytes of the keys"""
    return np.ascontiguousarray(O.compress(P0) if P1 is None else np.hstack([O.compress(P0), O.compress(P1)]))


def _oracle_wire(scheme, sig, pk, m):
    fn = getattr(O, "verify_%s_wire" % scheme)
    if len(m) < 64:
        return fn(sig, pk, m)
    return ES._par(fn, sig, pk, m)


def _enc(v, sign):
    b = bytearray(M.le32(v))
    b[31] |= sign << 7
    return np.frombuffer(bytes(b), np.uint8)


def _non_squares(count):
    """encodings v whose u^2 = (v^2 - 1) / (1 + d v^2) has no root, by the oracle's decoder"""
    cand = np.stack([_enc(v, v & 1) for v in range(2, 200)])
    _, ok = O.decompress(cand)
    bad = cand[ok == 0]
    assert len(bad) >= count
    return bad[:count]


def _where_rec(P0, P1, key_ok):
    rec = _key_records(P0, P1)
    d = {}
    for j in range(len(rec)):
        if key_ok[j]:
            d.setdefault(rec[j].tobytes(), j)
    return d


def _expect_rec(where, pk):
    return np.array([where.get(pk[i].tobytes(), NONE) for i in range(len(pk))], dtype=np.uint32)


# ---- typed objects: Montgomery limbs, projective points (tests/test_gpu_keyed_mont.py, ..._open_mont.py) ----
def _limbs(points, rng):
    """affine [n, 64] -> Montgomery limbs [n, 96] of the same points with a fresh random z each"""
    return MC.to_limbs_py(H.projective(points, rng)[0], Q)


def _oracle_mont_cols(scheme, cols):
    O.lib()  # (loaded on this thread, before the row blocks go to a pool)
    fn = getattr(O, "verify_%s_mont" % scheme)
    cols = [np.ascontiguousarray(c) for c in cols]
    return np.asarray(fn(*cols) if len(cols[0]) < 64 else ES._par(fn, *cols)).astype(np.uint8)


# ---- the open-set typed suite's mixtures, which its child processes build as well ---------------------------
# 2^15 + 3: the first size at which a lane shares its inversion among 8 items, with a ragged last lane
NS = (1, 63, 64, 65, 4099, (1 << 15) + 3)
NSIG = {"single": 1, "double": 2, "vargen": 1}
NKEY = {"single": 1, "double": 2, "vargen": 2}
FRONT_N = 4099  # the block both processes build; tiled to NS[-1] for the lanes that share an inversion
REG, UNREG = 64, 8
_POOL, _MIX = {}, {}


def _pool(engine, scheme):
    """REG keys to register and UNREG valid keys nobody registers"""
    if scheme not in _POOL:
        _POOL[scheme] = _keys(engine, scheme, REG + UNREG, 9100 + len(scheme))
    return _POOL[scheme]


def _mixture(engine, scheme, k, n, seed=0):
    """n items: about 3/4 under the first k registered keys (k = 0: none), each key presented with a fresh random
    z, the rest under valid unregistered keys; a period-7 share tampered (harness.tamper: both kinds of key) ->
    dict(cols: the limb columns u, R[, R'], PK[, PK' | Gen], m; affine: the keys' normal form per item; want: the
    oracle's verdicts on the limbs)"""
    key = (scheme, k, n, seed)
    if key in _MIX:
        return _MIX[key]
    sk, gen, P0, P1 = _pool(engine, scheme)
    rng = np.random.default_rng(77 * n + k + seed)
    j = REG + rng.integers(0, UNREG, size=n)
    if k:
        reg = rng.integers(0, 4, size=n) != 0
        j[reg] = rng.integers(0, k, size=int(reg.sum()))
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R, Rp = _sign_items(engine, scheme, sk[j], gen[j] if gen is not None else None, m, r)
    b = {"u": u, "R": R, "PK": P0[j].copy(), "m": m}
    H.tamper(b, kind_single=scheme == "single", period=7)
    for f, mod in (("u", R_ORDER), ("m", Q)):  # the classes u + r / m + q have no limb form: the residue
        for i in range(n):
            v = M.from_le(b[f][i])
            if v >= mod:
                b[f][i] = np.frombuffer(M.le32(v % mod), np.uint8)
    affine = [b["PK"]] + ([np.ascontiguousarray(P1[j])] if P1 is not None else [])
    pts = [b["R"]] + ([Rp] if Rp is not None else [])
    cols = [MC.to_limbs_py(b["u"], R_ORDER)] + [_limbs(p, rng) for p in pts + affine] + [MC.to_limbs_py(b["m"], Q)]
    out = {"cols": cols, "affine": affine, "want": _oracle_mont_cols(scheme, cols), "j": j}
    if len(_MIX) > 6:
        _MIX.pop(next(iter(_MIX)))
    _MIX[key] = out
    return out


def _pool_keyset(engine, scheme, k, **kw):
    _, _, P0, P1 = _pool(engine, scheme)
    return engine.KeySet(scheme, np.ascontiguousarray(P0[:k]),
                         np.ascontiguousarray(P1[:k]) if P1 is not None else None, **kw)


def _open_mont_ws(engine, scheme, n):
    return torch.full((max(engine.keyed_open_mont_workspace_bytes(scheme, n), 4),), 0xA5, dtype=torch.uint8,
                      device=DEV)


def _plants(scheme):
    """(name, column, byte range, value) of every edge class"""
    top, zero = np.full(32, 0xFF, np.uint8), np.zeros(32, np.uint8)
    out = [("u >= r", 0, slice(0, 32), np.frombuffer(M.le32(R_ORDER + 5), np.uint8)),
           ("m >= q", -1, slice(0, 32), np.frombuffer(M.le32(Q), np.uint8))]
    for c in range(1, 1 + NSIG[scheme]):
        out += [("nonce %d limbs >= q" % c, c, slice(32, 64), top), ("nonce %d z = 0" % c, c, slice(64, 96), zero)]
    for c in range(1 + NSIG[scheme], 1 + NSIG[scheme] + NKEY[scheme]):
        out += [("key %d limbs >= q" % c, c, slice(0, 32), top), ("key %d z = 0" % c, c, slice(64, 96), zero),
                ("key %d z = q" % c, c, slice(64, 96), np.frombuffer(M.le32(Q), np.uint8))]
    return out
