"""Forged batches whose defects CANCEL in an unweighted sum — TEST INFRASTRUCTURE, no GPU use.

The batch fast accept (schnorr_amd/csrc/k_rlc.hip, keyed_rlc.h) tests  sum_i z_i (u_i G + c_i PK_i - R_i) == O
with secret, distinct 128-bit weights z_i.  A batch with ONE wrong item is rejected for any non-zero weight;
the batches built here are rejected only if the weights do their job: exactly the forged items are wrong
(per-item verdict 0 by the oracle) and the PLAIN sum of their defects  u G + c PK - R  is the identity, so
equal weights — a constant z, two items that share a keystream block, z' == z in the double scheme — would
accept them.

Every point added is D = d G with random d: all forged points stay in the prime-order subgroup and on the
curve, so neither the subgroup test nor the curve check rejects in the weights' place.

Constructions (item i signed with secret sk_i and nonce r_i; `pair` = (i, j)):
  u       u_i += t, u_j -= t                       defects +-t G (var-generator: +-t Gen, i and j share Gen)
  R       R_i = r_i G + D, R_j = r_j G - D, c = H(R, m) recomputed, u = r - c sk         defects -+D
  PK      PK_i += D / c_i, PK_j -= D / c_j          (single, var-generator)              defects +-D
  Gen     Gen_i += D / u_i, Gen_j -= D / u_j        (var-generator)                      defects +-D
  cross   ONE double item: R = r G + D, R' = r G' - D, c = H(R, R', m)     defects -D (first equation), +D (second)
Keyed (a registered key set, items carry key indices):
  key     two items under one secret; the set gets P + D / c_i and P - D / c_j appended, the items their indices
  u, R    as above, both items under one key (`same_key`) or under two
Every builder returns a Forgery: the forged batch, the same batch with the forgery undone (all valid) and
the forged items' indices.
"""
import random

import numpy as np

import oracle_lib as O
import pymodel as M

R_ORDER = M.R_ORDER
FIELDS = {"single": ("u", "R", "PK", "m"), "double": ("u", "R", "Rp", "PK", "PKp", "m"),
          "vargen": ("u", "R", "PK", "Gen", "m")}
KINDS = {"single": ("u", "R", "PK"), "double": ("u", "R", "cross"), "vargen": ("u", "R", "PK", "Gen")}
KEYED_KINDS = ("key", "u", "R")
N = 1543                      # prime: seven workgroups of the prep kernel with a ragged tail
PAIRS = ((0, 1), (5, 69), (7, 263), (3, N - 1))
KEY_COUNTS = (1, 37, 300)     # one key; per-workgroup sums in LDS; beyond kKeyedLdsKeys = 256: global atomics


def unkeyed_cases(scheme):
    """(kind, pair): every construction of the scheme at (5, 69), the u- and R-pair at every pair"""
    out = [(kind, (5, 5) if kind == "cross" else (5, 69)) for kind in KINDS[scheme]]
    return out + [(kind, pair) for kind in ("u", "R") for pair in PAIRS if pair != (5, 69)]


def keyed_cases(scheme, k):
    """(kind, same_key) at pair (5, 69): the key-pair, the u- and R-pair under one key and (k > 1) under two —
    the var-generator u-pair under one only: +-t Gen cancel over one generator"""
    out = [("key", True), ("u", True), ("R", True)]
    if k > 1:
        out += [("R", False)] + ([("u", False)] if scheme != "vargen" else [])
    return out


class Forgery:
    def __init__(self, scheme, forged, honest, items, keys=None):
        self.scheme, self.forged, self.honest, self.items, self.keys = scheme, forged, honest, list(items), keys


def le(x):
    return np.frombuffer(M.le32(x), np.uint8)


def pt_row(P):
    return np.frombuffer(M.point_bytes(P), np.uint8)


def as_int(row):
    return M.from_le(bytes(row))


def as_point(row):
    return (M.from_le(bytes(row[:32])), M.from_le(bytes(row[32:])))


def _inv(x):
    return pow(x, -1, R_ORDER)


def challenge_of(scheme, a, i):
    if scheme == "double":
        return M.challenge_double(as_point(a["R"][i]), as_point(a["Rp"][i]), as_int(a["m"][i]))
    return M.challenge(as_point(a["R"][i]), as_int(a["m"][i]))


def defects(scheme, a, i, keys=None):
    """u G + c PK - R of item i, one point per equation (pymodel's affine law); keys: (P0, P1) of a key set"""
    u, c = as_int(a["u"][i]), challenge_of(scheme, a, i)
    if keys is not None:
        k = int(a["idx"][i])
        pk, second = as_point(keys[0][k]), (as_point(keys[1][k]) if keys[1] is not None else None)
    else:
        pk = as_point(a["PK"][i])
        second = as_point(a["PKp"][i]) if scheme == "double" else (as_point(a["Gen"][i]) if scheme == "vargen" else None)
    gen = second if scheme == "vargen" else M.GEN
    out = [M.padd(M.padd(M.pmul(gen, u), M.pmul(pk, c)), M.pneg(as_point(a["R"][i])))]
    if scheme == "double":
        out.append(M.padd(M.padd(M.pmul(M.GEN_NUMS, u), M.pmul(second, c)), M.pneg(as_point(a["Rp"][i]))))
    return out


def defect_sum(scheme, a, items, keys=None):
    acc = M.IDENTITY
    for i in items:
        for d in defects(scheme, a, i, keys):
            acc = M.padd(acc, d)
    return acc


# ---- signed bases (built once per process) -------------------------------------------------------------------
_BASES = {}


def base(scheme, n=N, seed=4100):
    """n honestly signed items, one key each (oracle_lib.keygen_sign_*), with their secrets ("sk")"""
    key = (scheme, n, seed)
    if key not in _BASES:
        d = getattr(O, "keygen_sign_" + scheme)(n, seed + len(scheme), nthreads=8)
        _BASES[key] = {k: d[k] for k in FIELDS[scheme] + ("sk",)}
    return {k: v.copy() for k, v in _BASES[key].items()}


def _mul(scalars, points):
    return O.scalar_mul(np.stack([le(s) for s in scalars]), np.ascontiguousarray(points))


def keyed_base(scheme, k, n=N, seed=4200):
    """n honest items under k keys (uniform indices): the set's points P0 / P1 (P1: PK' of the double scheme,
    Gen of the var-generator one) with their secrets, items u, R, Rp, idx, m with their nonces"""
    key = ("keyed", scheme, k, n, seed)
    if key not in _BASES:
        rnd = random.Random(seed + 31 * k + len(scheme))
        sk = [rnd.randrange(1, R_ORDER) for _ in range(k)]
        G, Gp = pt_row(M.GEN), pt_row(M.GEN_NUMS)
        P1 = None
        if scheme == "vargen":
            P1 = _mul([rnd.randrange(1, R_ORDER) for _ in range(k)], np.tile(G, (k, 1)))
            P0 = _mul(sk, P1)
        else:
            P0 = _mul(sk, np.tile(G, (k, 1)))
            if scheme == "double":
                P1 = _mul(sk, np.tile(Gp, (k, 1)))
        idx = np.array([rnd.randrange(k) for _ in range(n)], np.uint32)
        r = [rnd.randrange(1, R_ORDER) for _ in range(n)]
        m = np.stack([le(rnd.randrange(M.Q)) for _ in range(n)])
        R = _mul(r, P1[idx] if scheme == "vargen" else np.tile(G, (n, 1)))
        Rp = _mul(r, np.tile(Gp, (n, 1))) if scheme == "double" else None
        c = O.challenge_double(R, Rp, m) if scheme == "double" else O.challenge_single(R, m)
        u = np.stack([le((r[i] - as_int(c[i]) * sk[idx[i]]) % R_ORDER) for i in range(n)])
        _BASES[key] = {"P0": P0, "P1": P1, "sk": sk, "u": u, "R": R, "Rp": Rp, "idx": idx, "m": m, "r": r}
    out = {}
    for name, v in _BASES[key].items():
        out[name] = v.copy() if isinstance(v, np.ndarray) else (list(v) if isinstance(v, list) else v)
    return out


def keyed_oracle(scheme, a, keys):
    P0, P1 = keys
    idx = a["idx"]
    if scheme == "single":
        return O.verify_single(a["u"], a["R"], P0[idx], a["m"], nthreads=8)
    if scheme == "double":
        return O.verify_double(a["u"], a["R"], a["Rp"], P0[idx], P1[idx], a["m"], nthreads=8)
    return O.verify_vargen(a["u"], a["R"], P0[idx], P1[idx], a["m"], nthreads=8)


def oracle(scheme, a):
    return getattr(O, "verify_" + scheme)(*[a[k] for k in FIELDS[scheme]], nthreads=8)


# ---- one item, re-signed with Python integers ----------------------------------------------------------------
def _nonce(scheme, a, i, sk):
    """r_i of an honest item: u + c sk"""
    return (as_int(a["u"][i]) + challenge_of(scheme, a, i) * sk) % R_ORDER


def _sign(scheme, a, i, sk, r, gen=M.GEN, dR=None, dRp=None):
    """item i of `a` signed with (sk, r) over generator `gen`; dR / dRp: points added to R / R' BEFORE the
    challenge is computed (the signature stays consistent with its own hash, the equation is off by them)"""
    R = M.pmul(gen, r)
    if dR is not None:
        R = M.padd(R, dR)
    a["R"][i] = pt_row(R)
    if scheme == "double":
        Rp = M.pmul(M.GEN_NUMS, r)
        if dRp is not None:
            Rp = M.padd(Rp, dRp)
        a["Rp"][i] = pt_row(Rp)
    a["u"][i] = le((r - challenge_of(scheme, a, i) * sk) % R_ORDER)


def _add(a, field, i, P):
    a[field][i] = pt_row(M.padd(as_point(a[field][i]), P))


def _copy(a):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in a.items()}


def _random_point(rnd):
    return M.pmul(M.GEN, rnd.randrange(1, R_ORDER))


def _shift_u(a, i, t):
    a["u"][i] = le((as_int(a["u"][i]) + t) % R_ORDER)


# ---- unkeyed constructions -----------------------------------------------------------------------------------
def forge(scheme, kind, pair, seed=1, src=None, wi=1, wj=1):
    """-> Forgery over base(scheme) (or `src`, a batch with its "sk" column).  wi, wj: the defects are
    wj D at item i and -wi D at item j — with (wi, wj) = (1, 1) they cancel in a plain sum; with the weights
    of the two positions they cancel in the WEIGHTED sum (tests/test_gpu_rlc_known_key.py).  `cross` takes
    pair = (i, i): the first equation is off by -wj D, the second by wi D (weighted: wi = z, wj = z')."""
    assert kind in KINDS[scheme], (scheme, kind)
    rnd = random.Random(1000 * seed + 7 * pair[0] + pair[1])
    honest = src if src is not None else base(scheme)
    sk = {x: as_int(honest["sk"][x]) for x in set(pair)}
    honest = {k: v for k, v in honest.items() if k != "sk"}
    i, j = pair
    if scheme == "vargen" and kind == "u":
        # +-t Gen cancel only over ONE generator: j is re-signed over Gen_i
        gen = as_point(honest["Gen"][i])
        r = _nonce(scheme, honest, j, sk[j])
        honest["Gen"][j] = honest["Gen"][i]
        honest["PK"][j] = pt_row(M.pmul(gen, sk[j]))
        _sign(scheme, honest, j, sk[j], r, gen)
    a = _copy(honest)
    if kind == "u":
        t = rnd.randrange(1, R_ORDER)
        _shift_u(a, i, wj * t)
        _shift_u(a, j, -wi * t)
    elif kind == "R":
        D = _random_point(rnd)
        for x, w in ((i, wj), (j, -wi)):
            gen = as_point(honest["Gen"][x]) if scheme == "vargen" else M.GEN
            _sign(scheme, a, x, sk[x], _nonce(scheme, honest, x, sk[x]), gen, dR=M.pmul(D, w % R_ORDER))
    elif kind in ("PK", "Gen"):
        D = _random_point(rnd)
        for x, w in ((i, wj), (j, -wi)):
            s = challenge_of(scheme, honest, x) if kind == "PK" else as_int(honest["u"][x])
            _add(a, kind, x, M.pmul(D, w * _inv(s) % R_ORDER))
    else:  # cross: the two equations of ONE double item
        assert i == j
        D = _random_point(rnd)
        _sign(scheme, a, i, sk[i], _nonce(scheme, honest, i, sk[i]), dR=M.pmul(D, wj % R_ORDER),
              dRp=M.pmul(D, -wi % R_ORDER))
    return Forgery(scheme, a, honest, sorted(set(pair)))


# ---- keyed constructions -------------------------------------------------------------------------------------
def _keyed_resign(scheme, b, x, key, dR=None):
    """item x of the keyed batch b under key `key`, same nonce"""
    b["idx"][x] = key
    gen = as_point(b["P1"][key]) if scheme == "vargen" else M.GEN
    _sign(scheme, b, x, b["sk"][key], b["r"][x], gen, dR=dR)


def forge_keyed(scheme, kind, k, pair, same_key=True, seed=1, wi=1, wj=1):
    """-> Forgery over keyed_base(scheme, k): .forged / .honest hold u, R, Rp, idx, m; .keys = (P0, P1) of the set
    to register (k + 2 keys for `key`)"""
    assert kind in KEYED_KINDS
    rnd = random.Random(2000 * seed + 7 * pair[0] + pair[1] + k)
    b = keyed_base(scheme, k)
    i, j = pair
    ki = int(b["idx"][i])
    if same_key or kind == "key":
        _keyed_resign(scheme, b, j, ki)
    else:
        assert k > 1 and not (scheme == "vargen" and kind == "u"), "+-t Gen cancel over one generator only"
        if int(b["idx"][j]) == ki:
            _keyed_resign(scheme, b, j, (ki + 1) % k)
    P0, P1 = b["P0"], b["P1"]
    cols = ("u", "R", "Rp", "idx", "m")
    honest = {c: b[c] for c in cols}
    a = _copy(honest)
    if kind == "u":
        t = rnd.randrange(1, R_ORDER)
        _shift_u(a, i, wj * t)
        _shift_u(a, j, -wi * t)
    elif kind == "R":
        D = _random_point(rnd)
        for x, w in ((i, wj), (j, -wi)):
            kx = int(b["idx"][x])
            gen = as_point(P1[kx]) if scheme == "vargen" else M.GEN
            _sign(scheme, a, x, b["sk"][kx], b["r"][x], gen, dR=M.pmul(D, w % R_ORDER))
    else:
        D = _random_point(rnd)
        extra = []
        for x, w in ((i, wj), (j, -wi)):
            c = challenge_of(scheme, honest, x)
            extra.append(pt_row(M.padd(as_point(P0[ki]), M.pmul(D, w * _inv(c) % R_ORDER))))
        P0 = np.concatenate([P0, np.stack(extra)])
        if P1 is not None:
            P1 = np.concatenate([P1, P1[[ki, ki]]])
        a["idx"][i], a["idx"][j] = k, k + 1
    return Forgery(scheme, a, honest, sorted(set(pair)), keys=(P0, P1))
