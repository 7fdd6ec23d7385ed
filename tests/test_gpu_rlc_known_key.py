"""The batch fast accept's aggregate under a KNOWN weight key (GPU; tests/gpu_probe/rlc_probe.hip).

The engine draws the ChaCha key of its weights per call and never shows it, so through the public entry
points the weights can only be tested statistically.  The probe library runs ONE group's aggregate — the
engine's own launchers and kernels, nothing copied — under a key the test chooses:

1. everything the prep kernels write (digit rows, fixed-base scalars, eligibility, the stored points, the keyed
   pass's per-key chunk sums) equals a Python-integer model (tests/rlc_weights.py) word for word;
2. the aggregate accepts EXACTLY when  sum_i z_i (u_i G + c_i PK_i - R_i)  is the identity for the model's
   z_i: a forgery whose two defects are z_j X and -z_i X is accepted under the key, and rejected with exactly
   kRlcSum under a key that differs in one bit or when any one bit of the weight it was built from is flipped
   — every term (fixed-base, long, short, keyed) carries the same, full-width weight;
3. two draws of the engine's own key source differ.
"""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import forgery_sets as F
import oracle_lib as O
import pymodel as M
import rlc_weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHEMES = ("single", "double", "vargen")
CODE = {"single": 0, "double": 1, "vargen": 2}
Q, R_ORDER = M.Q, M.R_ORDER
KEY = (0x9E3779B9, 0x7F4A7C15, 0xF39CC060, 0x5CEDC834, 0x1082276B, 0xF3A27251, 0xF86C6A11, 0xD0C18E95)
TOP = np.full(32, 0xFF, np.uint8)


class Args(ctypes.Structure):
    _fields_ = [("scheme", ctypes.c_int32), ("window_bits", ctypes.c_int32), ("groups", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("n", ctypes.c_uint64), ("boundary", ctypes.c_uint64),
                ("key", ctypes.c_uint32 * 8)] + \
               [(k, ctypes.c_void_p) for k in ("u", "R", "Rp", "PK", "PKp", "Gen", "m", "c", "valid", "keyset", "key_idx",
                                               "flags", "ok", "digits", "fsc", "pts", "ksum", "touched")]


class Probe:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        for name in ("dsv_rlcprobe_geometry", "dsv_rlcprobe_geometry_keyed", "dsv_rlcprobe_run", "dsv_rlcprobe_run_keyed",
                     "dsv_rlcprobe_random_keys"):
            getattr(self.lib, name).restype = ctypes.c_int

    def run(self, scheme, cols, bits, groups=1, key=KEY, c=None, valid=None, keyset=None, boundary=0, detail=False):
        """cols: host arrays by name (u, R, ..., m; idx for the keyed form) -> dict(flags [G, 4], ok [n], and with
        detail: digits [G, rows, row_stride], fsc [G, fsc_stride], pts [G, pts_stride], ksum, touched, sub)"""
        from schnorr_amd import _lib
        n = len(cols["u"])
        keep = []

        def dev(a):
            t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
            keep.append(t)
            return t.data_ptr()

        a = Args(scheme=CODE[scheme], window_bits=bits, groups=groups, n=n, boundary=boundary)
        a.key = (ctypes.c_uint32 * 8)(*key)
        for name in ("u", "R", "Rp", "PK", "PKp", "Gen", "m"):
            if cols.get(name) is not None:
                setattr(a, name, dev(cols[name]))
        if c is not None:
            a.c, a.valid = dev(c), dev(valid)
        keyed = keyset is not None
        if keyed:
            a.keyset = keyset._handle().value
            a.key_idx = dev(cols["idx"].view(np.int32))
        geo = (ctypes.c_uint64 * 8)()
        _lib.check(getattr(self.lib, "dsv_rlcprobe_geometry" + ("_keyed" if keyed else ""))(ctypes.byref(a), geo))
        G, sub, pts_stride, fsc_stride, digits_stride, rows, row_stride, ksum_words = [int(x) for x in geo]
        out = {"flags": np.zeros((G, 4), np.uint32), "ok": np.full(n, 9, np.uint8), "sub": sub, "groups": G}
        if detail:
            out["digits"] = np.zeros((G, digits_stride), np.uint16)
            out["fsc"] = np.zeros((G, fsc_stride), np.uint32)
            out["pts"] = np.zeros((G, pts_stride), np.uint32)
            if keyed:
                out["ksum"] = np.zeros((G, ksum_words), np.uint64)
                out["touched"] = np.zeros((G, keyset.k), np.uint32)
        for name in ("flags", "ok", "digits", "fsc", "pts", "ksum", "touched"):
            if name in out:
                setattr(a, name, out[name].ctypes.data)
        _lib.check(getattr(self.lib, "dsv_rlcprobe_run" + ("_keyed" if keyed else ""))(ctypes.byref(a)))
        if detail:
            out["digits"] = out["digits"][:, :rows * row_stride].reshape(G, rows, row_stride)
        return out


@pytest.fixture(scope="module")
def probe(engine):
    from schnorr_amd import build as B
    lib = B.rlc_probe_path()
    assert os.path.exists(lib), "run `__graft_entry__.build()` first: it makes the fast-accept probe libdsv_rlcprobe.so"
    return Probe(lib)


def _int(row):
    return M.from_le(bytes(row))


def _words(x, count=8):
    return [(x >> (32 * j)) & 0xFFFFFFFF for j in range(count)]


def _below(row, mod):
    return all(_int(row[k:k + 32]) < mod for k in range(0, len(row), 32))


def _sub_of(gi, sub, n):
    g = gi // sub
    return g, gi - g * sub, min(sub, n - g * sub)


# ---- 1. the prep kernels against the model -------------------------------------------------------------------
N1 = 777
EDGE_C = (0, 1, (1 << 250) - 1)


def _prep_batch(scheme, seed):
    """777 items: honest ones, u in {0, 1, r - 1}, malformed rows, one eligible point off the curve; the supplied
    challenges: random 250-bit ones and {0, 1, 2^250 - 1}; the supplied validity bytes: one zero"""
    rnd = random.Random(seed)
    a = {k: v[:N1].copy() for k, v in F.base(scheme).items() if k != "sk"}
    for at, u in ((10, 0), (330, 1), (650, R_ORDER - 1)):
        a["u"][at] = F.le(u)
    a["u"][30] = TOP                                   # u >= r
    a["u"][31] = F.le(R_ORDER)                          # exactly r
    a["PK"][32, 32:] = TOP                             # a key coordinate >= q
    a["R"][33, :32] = F.le(Q)                           # a nonce coordinate == q
    second = {"double": "PKp", "vargen": "Gen"}.get(scheme)
    if second:
        a[second][34, :32] = TOP
    if scheme == "double":
        a["Rp"][35, 32:] = TOP
    a["m"][36] = TOP                                   # m >= q: the hash's validity byte is 0
    a["PK"][700, 0] ^= 1                               # canonical coordinates, not on the curve, item eligible
    c = np.stack([F.le(rnd.randrange(1 << 250)) for _ in range(N1)])
    for at, x in zip((20, 340, 660), EDGE_C):
        c[at] = F.le(x)
    valid = np.ones(N1, np.uint8)
    valid[37] = 0
    return a, c, valid


def _eligible(scheme, a, i, valid):
    good = bool(valid[i]) and _int(a["u"][i]) < R_ORDER
    for k in F.FIELDS[scheme][1:-1]:
        good = good and _below(a[k][i], Q)
    return good


def _check_prep(scheme, a, chal, valid, got, bits, keyed_keys=None):
    """digit rows, fsc, ok and the stored points of an unkeyed (keyed_keys: (k, key_ok)) pass against the model"""
    n = len(a["u"])
    keyed = keyed_keys is not None
    g = W.geometry(scheme, bits, keyed)
    sub, G = got["sub"], got["groups"]
    want_digits = np.zeros_like(got["digits"])
    slots = ([] if keyed else {"single": ["PK"], "double": ["PK", "PKp"], "vargen": ["PK", "Gen"]}[scheme]) + \
            (["R", "Rp"] if scheme == "double" else ["R"])
    items = []
    for gi in range(n):
        sg, i, total = _sub_of(gi, sub, n)
        if keyed:
            k, key_ok = keyed_keys
            idx = int(a["idx"][gi])
            good = bool(valid[gi]) and idx < k and bool(key_ok[idx]) and _int(a["u"][gi]) < R_ORDER and \
                _below(a["R"][gi], Q) and (scheme != "double" or _below(a["Rp"][gi], Q))
        else:
            good = _eligible(scheme, a, gi, valid)
        assert got["ok"][gi] == (1 if good else 0), gi
        u, c = _int(a["u"][gi]), _int(chal[gi])
        it = W.item(scheme, KEY, gi, bits, u if good else 0, c if good else 0, good, keyed)
        items.append((good, it))
        for row, d in it["rows"].items():
            want_digits[sg, row, i] = d
        for eq, f in enumerate(it["f"]):
            at = (eq * total + i) * 8
            assert [int(x) for x in got["fsc"][sg, at:at + 8]] == _words(f), (gi, eq)
        for slot, name in enumerate(slots):
            if not _below(a[name][gi], Q):
                continue                                      # (a coordinate >= q: the item is out, its slot holds junk)
            at = (slot * total + i) * 32
            p, t2d = W.decode_pt(got["pts"][sg, at:at + 27])
            src = F.as_point(a[name][gi])
            if name in ("R", "Rp"):
                src = M.pneg(src)
            assert p == src and t2d == W.t2d_of(src), (gi, name)
    for sg in range(G):
        total = min(sub, n - sg * sub)
        assert np.array_equal(got["digits"][sg, :, :total], want_digits[sg, :, :total]), "digit rows of sub-group %d" % sg
    return items


def _hash_model(scheme, a):
    """(c, valid) as the challenge hash leaves them: valid = every hashed coordinate and m below q"""
    n = len(a["u"])
    names = ("R", "Rp") if scheme == "double" else ("R",)
    valid = np.array([_below(a["m"][i], Q) and all(_below(a[k][i], Q) for k in names) for i in range(n)], np.uint8)
    safe = {k: a[k].copy() for k in names + ("m",)}
    for k in safe:
        safe[k][valid == 0] = 0
    c = O.challenge_double(safe["R"], safe["Rp"], safe["m"]) if scheme == "double" else O.challenge_single(safe["R"], safe["m"])
    return c, valid


@pytest.mark.parametrize("groups", (1, 3))
@pytest.mark.parametrize("bits", (8, 12))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_prep_is_the_model_word_for_word(probe, scheme, bits, groups):
    a, c, valid = _prep_batch(scheme, 100 + bits + groups)
    got = probe.run(scheme, a, bits, groups, c=c, valid=valid, detail=True)
    assert got["groups"] == groups
    _check_prep(scheme, a, c, valid, got, bits)
    # the point off the curve flags its own sub-group, and only that one
    for sg in range(groups):
        mine = _sub_of(700, got["sub"], N1)[0] == sg
        assert bool(got["flags"][sg, 0] & W.OFF_CURVE) == mine, sg
        assert got["flags"][sg, 1] == 1
    # the same items with the challenges hashed on the device
    hc, hvalid = _hash_model(scheme, a)
    assert not hvalid[36] and not hvalid[33] and hvalid.sum() == N1 - (3 if scheme == "double" else 2)
    got = probe.run(scheme, a, bits, groups, detail=True)
    _check_prep(scheme, a, hc, hvalid, got, bits)


def _keyed_prep_batch(scheme, k, seed):
    rnd = random.Random(seed)
    b = F.keyed_base(scheme, k, n=N1)
    a = {name: b[name] for name in ("u", "R", "Rp", "idx", "m")}
    P0 = b["P0"].copy()
    # two keys the items do reference (300 keys over 777 items leave some without any)
    bad_key = int(a["idx"][100])
    quiet_key = int(next(x for x in a["idx"][101:] if x != bad_key))
    P0[bad_key, :32] = TOP                              # key_ok = 0: its items are out
    valid = np.ones(N1, np.uint8)
    valid[a["idx"] == quiet_key] = 0                    # a key referenced by ineligible items only
    assert (a["idx"] == quiet_key).any() and (a["idx"] == bad_key).any()
    a["u"][30] = TOP
    a["R"][33, :32] = F.le(Q)
    a["idx"][40], a["idx"][41] = k, 0xFFFFFFFF          # no such key
    for at, u in ((10, 0), (330, 1), (650, R_ORDER - 1)):
        a["u"][at] = F.le(u)
    c = np.stack([F.le(rnd.randrange(1 << 250)) for _ in range(N1)])
    for at, x in zip((20, 340, 660), EDGE_C):
        c[at] = F.le(x)
    return a, c, valid, (P0, b["P1"]), bad_key, quiet_key


def _check_key_sums(scheme, a, items, got, k, n):
    ns = 1 if scheme == "single" else 2
    sub, G = got["sub"], got["groups"]
    per = [[[[] for _ in range(ns)] for _ in range(k)] for _ in range(G)]
    for gi, (good, it) in enumerate(items):
        if good:
            for s in range(ns):
                per[gi // sub][int(a["idx"][gi])][s].append(it["ksc"][s])
    for sg in range(G):
        for key in range(k):
            want = [x for s in range(ns) for x in W.chunk_sums(per[sg][key][s])]
            at = key * ns * 8
            assert [int(x) for x in got["ksum"][sg, at:at + ns * 8]] == want, (sg, key)
            assert got["touched"][sg, key] == (1 if per[sg][key][0] else 0), (sg, key)


@pytest.mark.parametrize("groups", (1, 3))
@pytest.mark.parametrize("k", (5, 300))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_keyed_prep_and_key_sums_are_the_model(engine, probe, scheme, k, groups):
    """k = 5: per-workgroup sums in LDS; k = 300: global atomics"""
    a, c, valid, (P0, P1), bad_key, quiet_key = _keyed_prep_batch(scheme, k, 200 + k + groups)
    with (engine.KeySet(scheme, P0, P1) if scheme != "single" else engine.KeySet(scheme, P0)) as ks:
        key_ok = [int(x) for x in ks.key_ok()]
        assert not key_ok[bad_key] and sum(key_ok) == k - 1
        got = probe.run(scheme, a, 8, groups, c=c, valid=valid, keyset=ks, detail=True)
        items = _check_prep(scheme, a, c, valid, got, 8, keyed_keys=(k, key_ok))
        _check_key_sums(scheme, a, items, got, k, N1)
        assert not got["touched"][:, [bad_key, quiet_key]].any()


def test_key_sums_at_their_largest_carries(engine, probe):
    """all 777 items under ONE key with c = 2^250 - 1: the chunk sums and their reduction mod r at the largest
    carries a group of this size reaches.  The items satisfy u G + c PK == R for that c, so the sums are also
    checked end to end: the aggregate accepts."""
    scheme, k, key = "single", 5, 2
    b = F.keyed_base(scheme, k, n=N1)
    cmax = (1 << 250) - 1
    rnd = random.Random(77)
    u = [rnd.randrange(R_ORDER) for _ in range(N1)]
    G = np.tile(F.pt_row(M.GEN), (N1, 1))
    R = O.scalar_mul(np.stack([F.le((x + cmax * b["sk"][key]) % R_ORDER) for x in u]), G)
    a = {"u": np.stack([F.le(x) for x in u]), "R": R, "Rp": None, "idx": np.full(N1, key, np.uint32), "m": b["m"]}
    c = np.tile(F.le(cmax), (N1, 1))
    valid = np.ones(N1, np.uint8)
    with engine.KeySet(scheme, b["P0"]) as ks:
        got = probe.run(scheme, a, 8, 1, c=c, valid=valid, keyset=ks, detail=True)
        items = _check_prep(scheme, a, c, valid, got, 8, keyed_keys=(k, [int(x) for x in ks.key_ok()]))
        _check_key_sums(scheme, a, items, got, k, N1)
        assert int(got["ksum"][0, key * 8:key * 8 + 8].max()) > 700 << 31
        assert list(got["flags"][0, :2]) == [0, 1]
        a["u"][400] = F.le((u[400] + 1) % R_ORDER)
        got = probe.run(scheme, a, 8, 1, c=c, valid=valid, keyset=ks)
        assert list(got["flags"][0, :2]) == [W.SUM, 1]


# ---- 2. accepted exactly when the weighted sum is the identity -----------------------------------------------
N2 = F.N
FLIP_BITS = (0, 31, 32, 63, 64, 127)
# (the double scheme's u-pair is off by +-t G in the first and +-t G' in the second equation: no pair of weights
#  cancels both, G and G' being independent — its R-pair touches the first equation only)
WEIGHTED = {"single": ("u", "R", "PK"), "double": ("R", "cross"), "vargen": ("u", "R", "PK", "Gen")}


def _flags(got):
    return [[int(x) for x in row[:2]] for row in got["flags"]]


def _other_key(bit):
    k = list(KEY)
    k[bit // 32] ^= 1 << (bit % 32)
    return tuple(k)


def _weights_of(kind, pair, bits):
    """(wi, wj) that make forge(kind, pair, wi, wj) cancel under KEY: the positions' own weights"""
    zi = W.weights(KEY, pair[0], bits)
    if kind == "cross":
        return zi[0], zi[1]
    return zi[0], W.weights(KEY, pair[1], bits)[0]


def _run_weighted(probe, scheme, f, bits, key=KEY, groups=1, boundary=0):
    cols = {k: f.forged[k] for k in F.FIELDS[scheme]}
    got = probe.run(scheme, cols, bits, groups, key=key, boundary=boundary)
    assert got["ok"].all()
    return _flags(got)


WCASES = [(s, kind) for s in SCHEMES for kind in WEIGHTED[s]]
WPAIRS = ((5, 69), (3, N2 - 1))   # the second: the last item of the prep kernel's ragged last workgroup
WPAIR_IDS = ["%d-%d" % p for p in WPAIRS]


@pytest.mark.parametrize("pair", WPAIRS, ids=WPAIR_IDS)
@pytest.mark.parametrize("bits", (8, 12))
@pytest.mark.parametrize("scheme,kind", WCASES, ids=["%s-%s" % c for c in WCASES])
def test_accepts_exactly_when_the_weighted_sum_is_the_identity(probe, scheme, kind, bits, pair):
    if kind == "cross":
        pair = (pair[1], pair[1])
    wi, wj = _weights_of(kind, pair, bits)
    f = F.forge(scheme, kind, pair, wi=wi, wj=wj)
    assert _run_weighted(probe, scheme, f, bits) == [[0, 1]], (pair, "not accepted under the key it was built for")
    assert _run_weighted(probe, scheme, f, bits, key=_other_key(pair[0] % 256)) == [[W.SUM, 1]], pair
    # one bit of the weight off, in every part of it: never the identity
    for b in FLIP_BITS:
        flips = [(wi ^ (1 << b), wj)] + ([(wi, wj ^ (1 << b))] if kind == "cross" else [])
        for fi, fj in flips:
            g = F.forge(scheme, kind, pair, wi=fi, wj=fj)
            assert _run_weighted(probe, scheme, g, bits) == [[W.SUM, 1]], (pair, b)


def test_the_weight_follows_the_item_number_across_sub_groups_and_ranges(probe):
    """three sub-groups with the pair in the last one, and the bucket pass in two ranges with the pair across
    them: the keystream counter is the item's place in the GROUP (base + i), not in its sub-group or range"""
    plan_sub = 576                                   # 1543 items in three sub-groups of 64-item multiples
    for kind in ("u", "R"):
        pair = (2 * plan_sub + 48, N2 - 1)
        wi, wj = _weights_of(kind, pair, 8)
        f = F.forge("single", kind, pair, wi=wi, wj=wj)
        cols = {k: f.forged[k] for k in F.FIELDS["single"]}
        got = probe.run("single", cols, 8, 3)
        assert got["sub"] == plan_sub and got["groups"] == 3
        assert _flags(got) == [[0, 1]] * 3, kind
        g = F.forge("single", kind, pair, wi=wi ^ 2, wj=wj)
        assert _run_weighted(probe, "single", g, 8, groups=3) == [[0, 1], [0, 1], [W.SUM, 1]], kind
        boundary = 768
        pair = (5, boundary + 5)
        wi, wj = _weights_of(kind, pair, 8)
        f = F.forge("single", kind, pair, wi=wi, wj=wj)
        assert _run_weighted(probe, "single", f, 8, boundary=boundary) == [[0, 1]], kind
        g = F.forge("single", kind, pair, wi=wi, wj=wj ^ (1 << 70))
        assert _run_weighted(probe, "single", g, 8, boundary=boundary) == [[W.SUM, 1]], kind


@pytest.mark.parametrize("pair", WPAIRS, ids=WPAIR_IDS)
@pytest.mark.parametrize("bits", (8, 12))
@pytest.mark.parametrize("k", (37, 300))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_keyed_key_pair_under_the_known_key(engine, probe, scheme, k, bits, pair):
    """the registered keys' terms carry the weights too: P + (z_j / c_i) D and P - (z_i / c_j) D cancel under the
    key, not under another, not with one bit of a weight flipped.  ONE key set per case: the k keys of the base,
    then the two forged keys of every variant (the true weights, then z_i with one bit flipped); a variant's
    batch differs from the others in the two items' key indices only."""
    wi, wj = _weights_of("key", pair, bits)
    variants = [(wi, wj)] + [(wi ^ (1 << b), wj) for b in FLIP_BITS]
    forged = [F.forge_keyed(scheme, "key", k, pair, wi=w0, wj=w1) for w0, w1 in variants]
    first = forged[0]
    P0, P1 = first.keys[0][:k], (first.keys[1][:k] if first.keys[1] is not None else None)
    batches = []
    for v, f in enumerate(forged):
        assert np.array_equal(f.keys[0][:k], P0) and list(f.forged["idx"][list(pair)]) == [k, k + 1]
        assert all(f.forged[c] is None or np.array_equal(f.forged[c], first.forged[c]) for c in ("u", "R", "Rp", "idx", "m"))
        a = dict(f.forged, idx=f.forged["idx"].copy())
        a["idx"][list(pair)] = [k + 2 * v, k + 2 * v + 1]
        batches.append(a)
    P0 = np.concatenate([P0] + [f.keys[0][k:] for f in forged])
    if P1 is not None:
        P1 = np.concatenate([P1] + [f.keys[1][k:] for f in forged])
    assert len(P0) == k + 2 * len(variants)

    with (engine.KeySet(scheme, P0, P1) if scheme != "single" else engine.KeySet(scheme, P0)) as ks:
        def flags(a, key=KEY):
            got = probe.run(scheme, a, bits, 1, key=key, keyset=ks)
            assert got["ok"].all()
            return _flags(got)

        assert flags(batches[0]) == [[0, 1]], "not accepted under the key it was built for"
        assert flags(batches[0], key=_other_key(200)) == [[W.SUM, 1]]
        for b, a in zip(FLIP_BITS, batches[1:]):
            assert flags(a) == [[W.SUM, 1]], b


# ---- 3. the engine's key source ------------------------------------------------------------------------------
def test_two_draws_of_the_weight_key_differ(probe):
    from schnorr_amd import _lib
    out = (ctypes.c_uint32 * 16)()
    _lib.check(probe.lib.dsv_rlcprobe_random_keys(out))
    a, b = list(out[:8]), list(out[8:])
    assert a != b and any(a) and any(b)
