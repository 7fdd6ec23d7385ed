"""The device field, group-law, Hades and inversion functions on raw limbs, at the bounds the interval
prover (tests/fe29_bounds.py) assigns to their inputs.

schnorr_amd/libdsv_probe.so (tests/gpu_probe/limb_probe.hip, built by __graft_entry__.build()) runs
the functions of fe29.h / jubjub29.h / quad29.h / hades29.h / inv29.h / decode29.h on 9 x u32 limb
records exactly as the device holds them.  Per op the inputs are drawn from four classes:
  (a) random limb vectors inside the op's input contract;
  (b) the prover's ceilings: every limb at its bound as far as the value bound allows (the top limb
      takes what remains), alternating bound / 0 patterns, all limbs zero;
  (c) non-canonical representatives k q of zero for every k the contract admits, and of q - 1 and 1,
      spread over the limbs in more than one way;
  (d) op-specific edges: real curve points with a random z (identity, order 2, order-8 component),
      S-box outputs with limb 0 in {1, 2^29}, inversion inputs that take the exact-compare branch.
Checks: limbs bit-exact against the Python model (tests/fe29_model.py, whose 32/64-bit overflow
conditions are assertions), values against Python integers / pymodel, outputs inside the bounds the
prover states for them, and the four lanes of a quad identical."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import fe29_bounds as FB
import fe29_model as F
import pymodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "schnorr_amd", "csrc"))
import gen_constants as G  # noqa: E402

pytestmark = pytest.mark.gpu

Q, NL, LB, M29 = F.Q, F.NL, F.LB, F.M29
RM = 1 << F.RBITS                                    # Montgomery R = 2^261
RINV = pow(RM, -1, Q)
N_FE, N_PT = 3072, 768                               # items per op: field / point and Hades ops


# ---- the probe library ----------------------------------------------------------------------------
class Probe:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
        self.lib.dsv_probe_ops.restype = ctypes.c_int
        self.lib.dsv_probe_ops.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_char_p)] + [ctypes.POINTER(ctypes.c_int)] * 3
        self.lib.dsv_probe_run.restype = ctypes.c_int
        self.lib.dsv_probe_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        self.ops = {}
        for i in range(self.lib.dsv_probe_ops(-1, None, None, None, None)):
            name, iw, ow, ipw = ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            self.lib.dsv_probe_ops(i, ctypes.byref(name), ctypes.byref(iw), ctypes.byref(ow), ctypes.byref(ipw))
            self.ops[name.value.decode()] = (i, iw.value, ow.value, ipw.value)

    def run(self, name, rows):
        """rows: one list of u32 words per item -> list of output word lists"""
        idx, iw, ow, _ = self.ops[name]
        a = np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))
        assert a.shape == (len(rows), iw), (name, a.shape, iw)
        out = np.zeros((len(rows), ow), dtype=np.uint32)
        st = self.lib.dsv_probe_run(idx, a.ctypes.data, len(rows), out.ctypes.data)
        assert st == 0, "%s: dsv_probe_run returned %d" % (name, st)
        return [[int(x) for x in r] for r in out]


@pytest.fixture(scope="module")
def probe():
    from schnorr_amd import build as B
    lib = B.probe_path()
    assert os.path.exists(lib), "run `__graft_entry__.build()` first: it makes the limb probe libdsv_probe.so"
    return Probe(lib)


def test_probe_exports_the_op_table(probe):
    """every op family the tests below use is there, with whole waves of items"""
    for name in ("mul", "sub4w", "ext_add_sub_aniels_t", "qext_octet_combine", "hades_mds_mask11", "fe_invert_euclid"):
        assert name in probe.ops
    assert probe.ops["qext_double"][3] == 16 and probe.ops["qext_octet_combine"][3] == 8
    assert probe.ops["hades_permute"][3] == 64


# ---- input classes ---------------------------------------------------------------------------------
rnd = random.Random(20261016)


def _fits(limbs, b):
    return all(0 <= x <= y for x, y in zip(limbs, b.l)) and F.val(limbs) <= b.v


def ceiling(b):
    """every limb at its bound; the top limb takes what the value bound leaves"""
    low = list(b.l[:NL - 1])
    return low + [min(b.l[NL - 1], max(0, (b.v - F.val(low + [0])) >> (LB * (NL - 1))))]


def alternating(b, phase):
    low = [b.l[i] if (i + phase) % 2 == 0 else 0 for i in range(NL - 1)]
    top = b.l[NL - 1] if (NL - 1 + phase) % 2 == 0 else 0
    return low + [min(top, max(0, (b.v - F.val(low + [0])) >> (LB * (NL - 1))))]


def random_in(b):
    low = [rnd.randint(0, x) for x in b.l[:NL - 1]]
    room = max(0, (b.v - F.val(low + [0])) >> (LB * (NL - 1)))
    return low + [rnd.randint(0, min(b.l[NL - 1], room))]


def spread(x, b, how):
    """a limb vector of the integer x inside b: canonical limbs, or with 2^29 moved down from limb
    i + 1 into limb i wherever the bounds allow (how = 'low': every limb, 'some': at random)"""
    if x < 0 or x > b.v:
        return None
    l = [(x >> (LB * i)) & M29 for i in range(NL - 1)] + [x >> (LB * (NL - 1))]
    if how != "canon":
        for i in range(NL - 2, -1, -1):
            if how == "some" and rnd.random() < 0.5:
                continue
            while l[i + 1] >= 1 and l[i] + (1 << LB) <= b.l[i]:
                l[i + 1] -= 1
                l[i] += 1 << LB
    return l if _fits(l, b) else None


def zero_reps(b):
    """class (c): k q, q - 1 (+ k q), 1 (+ k q) for every k the bound admits, in several spreads"""
    out = []
    for k in range(b.v // Q + 1):
        for x in (k * Q, k * Q + Q - 1, k * Q + 1):
            for how in ("canon", "low", "some"):
                r = spread(x, b, how)
                if r is not None:
                    out.append(r)
    return out


def edge_set(b):
    """classes (b) and (c) for one field element of bound b"""
    out = [ceiling(b), alternating(b, 0), alternating(b, 1), [0] * NL] + zero_reps(b)
    return [x for x in out if _fits(x, b)]


def draw(bounds, n, extra=()):
    """n items of len(bounds) field elements: every edge of every operand against ceilings and random
    partners, then random items (class a); `extra` items (class d) first"""
    items = [list(x) for x in extra]
    edges = [edge_set(b) for b in bounds]
    for j, es in enumerate(edges):
        for e in es:
            for partner in ("ceil", "rand"):
                items.append([e if k == j else (ceiling(b) if partner == "ceil" else random_in(b))
                              for k, b in enumerate(bounds)])
    for e in zip(*[es[:4] for es in edges]):          # all operands at the same pattern
        items.append(list(e))
    while len(items) < n:
        items.append([random_in(b) for b in bounds])
    for it in items:
        for x, b in zip(it, bounds):
            assert _fits(x, b), (x, b)
    return items


def flat(item):
    return [w for fe in item for w in fe]


def split(words, k):
    return [words[i * NL:(i + 1) * NL] for i in range(k)]


def in_bound(x, b, what):
    assert _fits(x, b), "%s: %s outside %r" % (what, [hex(v) for v in x], b)


# ---- the prover's invariants -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inv():
    g = FB.prove_group_law()
    qd = FB.prove_quad_group_law()
    h = FB.prove_hades()
    nz = FB.prove_normalize_and_limb_conversion()
    acc, niels = g["acc"], g["niels"]
    N = FB.mul(FB.canonical(), FB.canonical())       # fe_to_mont of a decoded coordinate
    return {"acc": acc, "niels": niels, "fixed": FB.canonical(), "N": N, "qacc": qd["acc"], "qout": qd["out"],
            "aniels": {k: FB.join(niels[k], FB.canonical()) for k in ("vpu", "vmu", "t2d")},
            "tt": FB.mul(acc["t1"], acc["t2"]), "hades": h, "inverse": nz["inverse"]}


# ---- fe29.h --------------------------------------------------------------------------------------------
def fe_cases(I):
    """op -> (operand bounds, model(args) -> limbs or flag, value(args ints, out) check or None)"""
    acc, niels, N = I["acc"], I["niels"], I["N"]
    raw = FB.sub_raw(acc["v"], acc["u"], 2)           # an un-carried difference (limbs < 2^31)
    twice = FB.add(N, N)                              # a sum of two products (limbs < 2^30)
    sub8 = FB.sub(acc["u"], N, 8)
    ripple_in = FB.B([(1 << 31) - 1] * (NL - 1) + [(1 << 26)], 16 * Q - 1)
    norm = lambda v: FB.B([M29] * (NL - 1) + [(1 << 30) - 1], v)   # ripple-normalised, value < v
    mont = lambda x: x * RINV % Q
    V = F.val
    return {
        "mul": ([[raw, niels["vmu"]], [FB.add(acc["v"], acc["u"]), niels["vpu"]], [acc["t1"], acc["t2"]], [N, N]],
                lambda a, b: F.mul(a, b), lambda a, b, r: (V(r) - V(a) * V(b) * RINV) % Q == 0),
        "sqr": ([[twice], [N]], lambda a: F.sqr(a), lambda a, r: (V(r) - V(a) ** 2 * RINV) % Q == 0),
        "add": ([[N, N], [FB.dbl(N), N]], F.add, lambda a, b, r: V(r) == V(a) + V(b)),
        "dbl": ([[N], [twice]], F.dbl, lambda a, r: V(r) == 2 * V(a)),
        "carry": ([[raw], [FB.add(FB.dbl(N), N)]], F.carry, lambda a, r: V(r) == V(a)),
        "sub2": ([[N, N], [FB.dbl(N), N]], lambda a, b: F.sub(a, b, 2), lambda a, b, r: V(r) == V(a) + 2 * Q - V(b)),
        "sub2_raw": ([[N, N]], lambda a, b: F.sub_raw(a, b, 2), lambda a, b, r: V(r) == V(a) + 2 * Q - V(b)),
        "sub4": ([[niels["vpu"], niels["vmu"]]], lambda a, b: F.sub(a, b, 4), lambda a, b, r: V(r) == V(a) + 4 * Q - V(b)),
        "sub4w": ([[N, twice], [FB.dbl(N), FB.sub_raw(N, N, 2)]], lambda a, b: F.sub(a, b, "4w"),
                  lambda a, b, r: V(r) == V(a) + 4 * Q - V(b)),
        "sub8": ([[acc["u"], N], [acc["v"], acc["z"]]], lambda a, b: F.sub(a, b, 8), lambda a, b, r: V(r) == V(a) + 8 * Q - V(b)),
        "neg2": ([[N], [I["fixed"]]], F.neg2, lambda a, r: V(r) == 2 * Q - V(a)),
        "ripple": ([[ripple_in], [sub8]], F.ripple, lambda a, r: V(r) == V(a) and all(x <= M29 for x in r[:8])),
        "cond_sub_x8": ([[norm(16 * Q - 1)]], lambda a: F.cond_sub(a, F.QX[8]),
                        lambda a, r: V(r) == (V(a) - 8 * Q if V(a) >= 8 * Q else V(a))),
        "cond_sub_x4": ([[norm(8 * Q - 1)]], lambda a: F.cond_sub(a, F.QX[4]),
                        lambda a, r: V(r) == (V(a) - 4 * Q if V(a) >= 4 * Q else V(a))),
        "cond_sub_x2": ([[norm(4 * Q - 1)]], lambda a: F.cond_sub(a, F.QX[2]),
                        lambda a, r: V(r) == (V(a) - 2 * Q if V(a) >= 2 * Q else V(a))),
        "cond_sub_x1": ([[norm(2 * Q - 1)]], lambda a: F.cond_sub(a, F.QX[1]),
                        lambda a, r: V(r) == (V(a) - Q if V(a) >= Q else V(a))),
        "canon": ([[sub8], [ripple_in]], F.canon, lambda a, r: V(r) == V(a) % Q),
        "from_mont": ([[N], [acc["u"]], [raw]], F.from_mont, lambda a, r: V(r) == mont(V(a))),
        "to_mont": ([[FB.canonical()]], F.to_mont, lambda a, r: (V(r) - V(a) * RM) % Q == 0),
        "equal": ([[acc["u"], FB.mul(N, acc["z"])], [acc["v"], acc["z"]]], lambda a, b: int(F.equal(a, b)),
                  lambda a, b, r: r == int((V(a) - V(b)) % Q == 0)),
        "is_zero_canon": ([[FB.canonical()]], lambda a: int(F.is_zero_canon(a)), lambda a, r: r == int(V(a) == 0)),
    }


def _fe_run(probe, name, bounds, model, value, n=N_FE):
    k = len(bounds)
    extra = []
    if name in ("equal",):                            # equal pairs: the same value, other representatives
        for _ in range(64):
            x = rnd.randrange(Q)
            a, b = spread(x, bounds[0], "some"), spread(x + Q, bounds[1], "low")
            if a is not None and b is not None:
                extra.append([a, b])
    items = draw(bounds, n, extra)
    outs = probe.run(name, [flat(it) for it in items])
    for it, o in zip(items, outs):
        r = o[0] if len(o) == 1 else o
        want = model(*it)
        assert r == want, (name, [[hex(v) for v in x] for x in it], r, want)
        assert value(*it, r), (name, it, r)
    return len(items)


@pytest.mark.parametrize("name", ["mul", "sqr", "add", "dbl", "carry", "sub2", "sub2_raw", "sub4", "sub4w", "sub8",
                                  "neg2", "ripple", "cond_sub_x1", "cond_sub_x2", "cond_sub_x4", "cond_sub_x8",
                                  "canon", "from_mont", "to_mont", "equal", "is_zero_canon"])
def test_fe29_op_limb_exact_at_the_proven_bounds(probe, inv, name):
    """fe29.h: limbs bit-exact against the model, values against Python integers, for every operand
    pair the prover admits (each contract list entry is one such pair)"""
    contracts, model, value = fe_cases(inv)[name]
    total = 0
    for bounds in contracts:
        total += _fe_run(probe, name, bounds, model, value, n=N_FE // len(contracts))
    assert total >= 1000


def test_fe29_word_conversions(probe):
    """fe_from_words_plain / fe_to_words_plain: any 256-bit word vector in, canonical limbs out and back"""
    words = [[rnd.getrandbits(32) for _ in range(8)] for _ in range(N_FE)]
    words += [[0xffffffff] * 8, [0] * 8, [0x80000000] * 8, [1] + [0] * 7, [0] * 7 + [0x80000000]]
    words += [[(x >> (32 * k)) & 0xffffffff for k in range(8)] for x in (Q - 1, Q, Q + 1, 2 * Q, (1 << 255) + 7)]
    limbs = probe.run("from_words_plain", words)
    for w, l in zip(words, limbs):
        assert l == F.from_words_plain(w) and F.val(l) == sum(x << (32 * k) for k, x in enumerate(w))
        assert all(x <= M29 for x in l[:8]) and l[8] < (1 << 24)
    back = probe.run("to_words_plain", limbs)
    assert back == words
    # canonical residues and limb vectors at 2^29 - 1 everywhere
    cl = [F.from_int(rnd.randrange(Q)) for _ in range(256)] + [[M29] * 8 + [(1 << 24) - 1]]
    assert probe.run("to_words_plain", cl) == [F.to_words_plain(x) for x in cl]


# ---- jubjub29.h ----------------------------------------------------------------------------------------
_T8 = None


def _order8():
    global _T8
    if _T8 is None:
        import torsion_model as TM
        _T8 = TM.order8_point()
    return _T8


def curve_points():
    """class (d): identity, order 2, order-8 component, generator multiples"""
    t8 = _order8()
    pts = [M.IDENTITY, (0, Q - 1), t8, M.pmul(t8, 3), M.padd(M.pmul(M.GEN, 12345), t8)]
    return pts + [M.pmul(M.GEN, rnd.randrange(1, M.R_ORDER)) for _ in range(11)]


def rep(x, b):
    """Montgomery form of x as a non-canonical representative inside b where one exists"""
    m = x * RM % Q
    for k in (3, 2, 1, 0):
        if m + k * Q <= b.v:
            r = spread(m + k * Q, b, rnd.choice(("low", "some", "canon")))
            if r is not None:
                return r
    return F.from_int(m)


def ext_of(P, bnd):
    """(u, v, z, t1, t2) = (xz, yz, z, xz, y) of the affine P with a random z: t1 t2 = u v / z"""
    z = rnd.randrange(1, Q)
    return [rep(P[0] * z % Q, bnd["u"]), rep(P[1] * z % Q, bnd["v"]), rep(z, bnd["z"]),
            rep(P[0] * z % Q, bnd["t1"]), rep(P[1], bnd["t2"])]


def niels_of(P, bnd):
    """extended niels (v+u, v-u, z, 2d t) of P with a random z"""
    z = rnd.randrange(1, Q)
    u, v = P[0] * z % Q, P[1] * z % Q
    return [rep((v + u) % Q, bnd["vpu"]), rep((v - u) % Q, bnd["vmu"]), rep(z, bnd["z"]),
            rep(2 * M.D * P[0] * P[1] % Q * z % Q, bnd["t2d"])]


def aniels_of(P, bnd):
    return [rep((P[1] + P[0]) % Q, bnd["vpu"]), rep((P[1] - P[0]) % Q, bnd["vmu"]),
            rep(2 * M.D * P[0] * P[1] % Q, bnd["t2d"])]


def plain(x):
    return F.val(x) * RINV % Q


def affine(u, v, z):
    zi = pow(plain(z), -1, Q)
    return plain(u) * zi % Q, plain(v) * zi % Q


def _ext(ws):
    return dict(zip(("u", "v", "z", "t1", "t2"), ws))


def _niels(ws):
    return dict(zip(("vpu", "vmu", "z", "t2d"), ws))


def _aniels(ws):
    return dict(zip(("vpu", "vmu", "t2d"), ws))


def _ext_words(p):
    return [p["u"], p["v"], p["z"], p["t1"], p["t2"]]


def pt_cases(I):
    """op -> (operand bounds, real-point items, model(items) -> output limbs, point value check)"""
    acc, niels, an, tt = I["acc"], I["niels"], I["aniels"], I["tt"]
    E = [acc[k] for k in ("u", "v", "z", "t1", "t2")]
    NI = [niels[k] for k in ("vpu", "vmu", "z", "t2d")]
    AN = [an[k] for k in ("vpu", "vmu", "t2d")]
    pts = curve_points()
    pairs = [(P, R) for P in pts[:8] for R in (P, M.pneg(P), pts[-1], pts[2], M.IDENTITY)]

    def ext_item(P, R=None, kind=None):
        e = ext_of(P, acc)
        if kind == "niels":
            return e + niels_of(R, niels)
        if kind == "aniels":
            return e + aniels_of(R, an)
        if kind == "aniels_t":
            return e + [rep(P[0] * P[1] % Q * pow(plain(e[2]), 1, Q) % Q, tt)] + aniels_of(R, an)
        return e

    def aff_out(o):
        return affine(o[0], o[1], o[2])

    return {
        "ext_double": (E, [ext_item(P) for P in pts], lambda it: _ext_words(F.ext_double(_ext(it))),
                       lambda it, o, P, R: aff_out(o) == M.pmul(P, 2)),
        "ext_double_affine": ([I["N"], I["N"]], [[rep(P[0], I["N"]), rep(P[1], I["N"])] for P in pts],
                              lambda it: _ext_words(F.ext_double_affine(it[0], it[1])),
                              lambda it, o, P, R: aff_out(o) == M.pmul(P, 2)),
        "ext_double_uvz": (E[:3], [ext_item(P)[:3] for P in pts], lambda it: list(F.ext_double_uvz(*it)),
                           lambda it, o, P, R: aff_out(o) == M.pmul(P, 2)),
        "ext_add_niels": (E + NI, [ext_item(P, R, "niels") for P, R in pairs],
                          lambda it: _ext_words(F.ext_add_niels(_ext(it[:5]), _niels(it[5:]))),
                          lambda it, o, P, R: aff_out(o) == M.padd(P, R)),
        "ext_add_aniels": (E + AN, [ext_item(P, R, "aniels") for P, R in pairs],
                           lambda it: _ext_words(F.ext_add_aniels(_ext(it[:5]), _aniels(it[5:]))),
                           lambda it, o, P, R: aff_out(o) == M.padd(P, R)),
        "ext_add_aniels_t": (E + [tt] + AN, [ext_item(P, R, "aniels_t") for P, R in pairs],
                             lambda it: _ext_words(F.ext_add_aniels_t(_ext(it[:5]), it[5], _aniels(it[6:]))),
                             lambda it, o, P, R: aff_out(o) == M.padd(P, R)),
        "ext_add_sub_aniels_t": (E + [tt] + AN, [ext_item(P, R, "aniels_t") for P, R in pairs],
                                 lambda it: [w for p in F.ext_add_sub_aniels(_ext(it[:5]), _aniels(it[6:]), it[5])
                                             for w in _ext_words(p)],
                                 lambda it, o, P, R: aff_out(o) == M.padd(P, R)
                                 and affine(o[5], o[6], o[7]) == M.padd(P, M.pneg(R))),
        "ext_add_aniels_is_identity": (E + AN, [ext_item(P, R, "aniels") for P, R in pairs]
                                       + [ext_item(M.pneg(R), R, "aniels") for R in pts],
                                       lambda it: [int(F.ext_add_aniels_is_identity(_ext(it[:5]), _aniels(it[5:])))],
                                       lambda it, o, P, R: o[0] == int(M.padd(P, R) == M.IDENTITY)),
        "ext_from_niels": (NI, [niels_of(P, niels) for P in pts],
                           lambda it: _ext_words(F.ext_from_niels(_niels(it))),
                           lambda it, o, P, R: aff_out(o) == P),
        "ext_to_niels": (E, [ext_item(P) for P in pts], lambda it: [F.ext_to_niels(_ext(it))[k] for k in ("vpu", "vmu", "z", "t2d")],
                         lambda it, o, P, R: affine(F.ext_from_niels(_niels(o))["u"], F.ext_from_niels(_niels(o))["v"],
                                                    F.ext_from_niels(_niels(o))["z"]) == P),
        "ext_to_niels_t": (E + [tt], [ext_item(P) + [rep(P[0] * P[1] % Q, tt)] for P in pts],
                           lambda it: [F.ext_to_niels_t(_ext(it[:5]), it[5])[k] for k in ("vpu", "vmu", "z", "t2d")],
                           lambda it, o, P, R: True),
        "ext_eq_affine": (E + [I["N"], I["N"]], [ext_item(P) + [rep(R[0], I["N"]), rep(R[1], I["N"])] for P, R in pairs],
                          lambda it: [int(F.ext_eq_affine(_ext(it[:5]), it[5], it[6]))],
                          lambda it, o, P, R: o[0] == int(P == R)),
    }, pairs, pts


def _pt_out_bounds(name, I):
    acc, niels = I["acc"], I["niels"]
    E = [acc[k] for k in ("u", "v", "z", "t1", "t2")]
    if name in ("ext_to_niels", "ext_to_niels_t"):
        return [niels[k] for k in ("vpu", "vmu", "z", "t2d")]
    if name == "ext_double_uvz":
        return E[:3]
    if name == "ext_add_sub_aniels_t":
        return E + E
    if name in ("ext_add_aniels_is_identity", "ext_eq_affine"):
        return None
    return E


PT_OPS = ["ext_double", "ext_double_affine", "ext_double_uvz", "ext_add_niels", "ext_add_aniels", "ext_add_aniels_t",
          "ext_add_sub_aniels_t", "ext_add_aniels_is_identity", "ext_from_niels", "ext_to_niels", "ext_to_niels_t",
          "ext_eq_affine"]


@pytest.mark.parametrize("name", PT_OPS)
def test_jubjub29_op_limb_exact_and_on_the_curve(probe, inv, name):
    """jubjub29.h: real points (projective, non-canonical limbs) give pymodel's sums and doublings;
    ceiling / random / zero-representative records give the model's limbs; every output record lies
    inside the group law's proven invariant"""
    cases, pairs, pts = pt_cases(inv)
    bounds, real, model, value = cases[name]
    items = draw(bounds, N_PT, [split(flat(r), len(bounds)) for r in real])
    outs = probe.run(name, [flat(it) for it in items])
    ob = _pt_out_bounds(name, inv)
    real_pr = pairs if len(real) == len(pairs) else [(P, None) for P in pts]
    if name == "ext_add_aniels_is_identity":
        real_pr = pairs + [(M.pneg(R), R) for R in pts]
    if name == "ext_eq_affine":
        real_pr = pairs
    for j, (it, o) in enumerate(zip(items, outs)):
        want = model(it)
        got = o if len(o) == 1 else split(o, len(o) // NL)
        assert got == want, (name, j, [[hex(v) for v in x] for x in it])
        if ob is not None:
            for x, b in zip(got, ob):
                in_bound(x, b, name)
        if j < len(real):
            P, R = real_pr[j]
            assert value(it, got, P, R), (name, j, P, R)


# ---- quad29.h / k_quad.hip -------------------------------------------------------------------------------
def _q(ws):
    return dict(zip(("u", "v", "z", "t"), ws))


def _q_words(p):
    return [p["u"], p["v"], p["z"], p["t"]]


def qext_of(P, b):
    z = rnd.randrange(1, Q)
    return [rep(P[0] * z % Q, b["u"]), rep(P[1] * z % Q, b["v"]), rep(z, b["z"]), rep(P[0] * P[1] % Q * z % Q, b["t"])]


QUAD_OPS = ["qext_double_t", "qext_double", "qext_add_niels", "qext_add_aniels", "qext_mul16", "qext_octet_combine"]


@pytest.mark.parametrize("name", QUAD_OPS)
def test_quad29_op_limb_exact_in_all_four_lanes(probe, inv, name):
    """quad29.h and the octet combine of k_quad.hip (from_upper_quad): four (eight) lanes per item, the
    record replicated in each; every lane's copy of the result equals the model's limbs, the affine
    result equals pymodel, and the result lies inside the quad fixpoint's invariant"""
    qa, niels, fixed = inv["qacc"], inv["niels"], inv["fixed"]
    QE = [qa[k] for k in ("u", "v", "z", "t")]
    NI = [niels[k] for k in ("vpu", "vmu", "z", "t2d")]
    AN = [fixed] * 3
    pts = curve_points()
    pairs = [(P, R) for P in pts[:8] for R in (P, M.pneg(P), pts[-1], pts[2], M.IDENTITY)]
    if name in ("qext_double_t", "qext_double", "qext_mul16"):
        bounds, real = QE, [(qext_of(P, qa), P, None) for P in pts]
        model = {"qext_double_t": lambda it: F.qext_double(_q(it), True), "qext_double": lambda it: F.qext_double(_q(it), False),
                 "qext_mul16": lambda it: F.qext_mul16(_q(it))}[name]
        mult = 16 if name == "qext_mul16" else 2
        value = lambda o, P, R: affine(o[0], o[1], o[2]) == M.pmul(P, mult)
    elif name == "qext_add_niels":
        bounds, real = QE + NI, [(qext_of(P, qa) + niels_of(R, niels), P, R) for P, R in pairs]
        model = lambda it: F.qext_add_niels(_q(it[:4]), _niels(it[4:]))
        value = lambda o, P, R: affine(o[0], o[1], o[2]) == M.padd(P, R)
    elif name == "qext_add_aniels":
        bounds, real = QE + AN, [(qext_of(P, qa) + aniels_of(R, {"vpu": fixed, "vmu": fixed, "t2d": fixed}), P, R)
                                 for P, R in pairs]
        model = lambda it: F.qext_add_aniels(_q(it[:4]), _aniels(it[4:]))
        value = lambda o, P, R: affine(o[0], o[1], o[2]) == M.padd(P, R)
    else:
        bounds, real = QE + QE, [(qext_of(P, qa) + qext_of(R, qa), P, R) for P, R in pairs]
        model = lambda it: F.octet_combine(_q(it[:4]), _q(it[4:]))
        value = lambda o, P, R: affine(o[0], o[1], o[2]) == M.padd(P, R)
    items = draw(bounds, N_PT // 2, [r[0] for r in real])
    outs = probe.run(name, [flat(it) for it in items])
    ob = [inv["qout"][k] for k in ("u", "v", "z", "t")] if name == "qext_octet_combine" else QE
    for j, (it, o) in enumerate(zip(items, outs)):
        lanes = [o[k * 4 * NL:(k + 1) * 4 * NL] for k in range(4)]
        assert all(ln == lanes[0] for ln in lanes), (name, j, "the four lanes of a quad differ")
        got = split(lanes[0], 4)
        want = _q_words(model(it))
        assert got == want, (name, j, [[hex(v) for v in x] for x in it])
        for x, b in zip(got, ob):
            in_bound(x, b, name)
        if j < len(real):
            assert value(got, real[j][1], real[j][2]), (name, j)
            if name != "qext_double":
                assert (plain(got[3]) * plain(got[2]) - plain(got[0]) * plain(got[1])) % Q == 0, "t != u v / z"


# ---- Hades (hades29.h / hades_mfma.h) ---------------------------------------------------------------------
_RC_DEV = FB._load_table("DSV_HADES_RC_HOST")
MDS = G.mds()
RC = G.round_constants()


def sbox_model(x):
    return F.mul(F.sqr(F.sqr(x)), x)


def mds_value(vals):
    return [sum(MDS[k][j] * vals[j] for j in range(5)) % Q for k in range(5)]


def sbox_outputs(b, n):
    """S-box outputs as fe_mul returns them: limb 0 in [1, 2^29], limbs 1..7 < 2^29, value < 2^256 + 1;
    class (d): limb 0 in {1, 2^29}, limbs 1..7 in {0, 2^29 - 1}"""
    out = []
    for _ in range(n // 2):
        l0 = rnd.choice((1, 1 << 29))
        l = [l0] + [rnd.choice((0, M29)) for _ in range(7)]
        top = min(b.l[8], (b.v - F.val(l + [0])) >> 232)
        out.append(l + [rnd.choice((0, top))])
    for x in edge_set(b) + [random_in(b) for _ in range(n // 2)]:
        if x[0] == 0:
            x = [1] + x[1:]
        if F.val(x) - 1 < (1 << 256):
            out.append(x)
    return out


def _check_rows(rows, want, h, what):
    for r, w in zip(rows, want):
        in_bound(r, h["row"], what)
        assert F.val(r) % Q == w % Q, what


@pytest.mark.parametrize("name,mask", [("hades_mds", 0), ("hades_mds_row1", 0), ("hades_mds_mask01", 0x01),
                                       ("hades_mds_mask11", 0x11)])
def test_hades_mds_on_the_matrix_cores_at_the_operand_edges(probe, inv, name, mask):
    """hades_mds_mfma: S-box outputs enter with limb 0 in [1, 2^29] and are lowered by one before the
    int8 digit split; constants (one_below_mask) enter one below their value.  Every row equals the
    plain MDS product mod q and comes back inside the prover's row bound."""
    h = inv["hades"]
    ops = sbox_outputs(h["mds_operand"], N_PT)
    consts = [random_in(FB.B([M29] * 8 + [(1 << 24) - 1])) for _ in range(64)] + [[0] * 9, [M29] * 8 + [(1 << 24) - 1]]
    items = []
    for j in range(N_PT):
        it = [ops[(j * 5 + k * 7) % len(ops)] for k in range(5)]
        for k in range(5):
            if (mask >> k) & 1:
                it[k] = consts[(j + k) % len(consts)]
        items.append(it)
    outs = probe.run(name, [flat(it) for it in items])
    for it, o in zip(items, outs):
        vals = [F.val(x) + ((mask >> k) & 1) for k, x in enumerate(it)]
        want = mds_value(vals)
        if name == "hades_mds_row1":
            _check_rows([o], [want[1]], h, name)
        else:
            _check_rows(split(o, 5), want, h, name)


def test_hades_sbox_limb_exact_at_the_proven_input_bound(probe, inv):
    h = inv["hades"]
    items = draw([h["sbox_in"]], N_FE // 2)
    outs = probe.run("hades_sbox", [flat(it) for it in items])
    for it, o in zip(items, outs):
        assert o == sbox_model(it[0])
        assert (F.val(o) * RM ** 4 - F.val(it[0]) ** 5) % Q == 0
        in_bound(o, h["mds_operand"], "hades_sbox")


def _state_items(b, n, words=5):
    return draw([b] * words, n)


def _mont_plain_state(it):
    return [plain(x) for x in it]


@pytest.mark.parametrize("word1", [False, True])
def test_hades_full_round(probe, inv, word1):
    """constants + S-boxes on the VALU, the dense layer on the matrix cores (word1_only: row 1 only)"""
    h = inv["hades"]
    items = _state_items(h["round_in"], N_PT)
    rounds = [rnd.choice((0, 1, 2, 3, 63, 64, 65, 66)) for _ in items]
    name = "hades_full_round_word1" if word1 else "hades_full_round"
    outs = probe.run(name, [flat(it) + [r] for it, r in zip(items, rounds)])
    for it, r, o in zip(items, rounds, outs):
        sb = [sbox_model(F.add(it[k], _RC_DEV[5 * r + k].l)) for k in range(5)]
        want = mds_value([F.val(x) for x in sb])
        if word1:
            _check_rows([o], [want[1]], h, name)
        else:
            _check_rows(split(o, 5), want, h, name)


@pytest.mark.parametrize("pad", [False, True])
def test_hades_first_round_with_constant_words(probe, inv, pad):
    """hades_first_round_const<PAD>: word 0 (and word 4) enter as the constants 0 (1): their S-box
    outputs are folded constants given one below their value"""
    h = inv["hades"]
    items = _state_items(h["round_in"], N_PT)
    name = "hades_first_round_const_pad" if pad else "hades_first_round_const"
    outs = probe.run(name, [flat(it) for it in items])
    for it, o in zip(items, outs):
        s = [[0] * NL] + it[1:4] + [list(F.ONE) if pad else it[4]]
        sb = [sbox_model(F.add(s[k], _RC_DEV[k].l)) for k in range(5)]
        _check_rows(split(o, 5), mds_value([F.val(x) for x in sb]), h, name)


def _plain_rounds(s, first, last):
    for rnd_ in range(first, last):
        full = rnd_ < 4 or rnd_ >= 63
        s = [(x + RC[5 * rnd_ + k]) % Q for k, x in enumerate(s)]
        s = [pow(x, 5, Q) for x in s] if full else s[:4] + [pow(s[4], 5, Q)]
        s = [sum(MDS[k][j] * s[j] for j in range(5)) % Q for k in range(5)]
    return s


def test_hades_partial_rounds_and_permutation(probe, inv):
    """the 59 partial rounds as one scalar recurrence (start-up rows, software pipeline, state rebuild)
    and the whole permutation equal the plain rounds mod q from states at the prover's bounds"""
    h = inv["hades"]
    items = _state_items(h["partial_in"], N_PT // 2)
    outs = probe.run("hades_partial_rounds", [flat(it) for it in items])
    for it, o in zip(items, outs):
        want = _plain_rounds(_mont_plain_state(it), 4, 63)
        rows = split(o, 5)
        for r in rows:
            in_bound(r, h["row"], "hades_partial_rounds")
        assert [plain(r) for r in rows] == want
    items = _state_items(h["permute_in"], N_PT // 2)
    outs = probe.run("hades_permute", [flat(it) for it in items])
    for it, o in zip(items, outs):
        rows = split(o, 5)
        for r in rows:
            in_bound(r, h["row"], "hades_permute")
        assert [plain(r) for r in rows] == M.hades_permute(_mont_plain_state(it))


def test_poseidon_truncate(probe, inv):
    h = inv["hades"]
    items = draw([FB.join(h["hash3"], h["hash5"])], N_FE // 2)
    outs = probe.run("poseidon_truncate", [flat(it) for it in items])
    for it, o in zip(items, outs):
        want = F.to_words_plain(F.from_mont(it[0]))
        want[7] &= 0x03ffffff
        assert o == want
        assert sum(x << (32 * k) for k, x in enumerate(o)) == plain(it[0]) & ((1 << 250) - 1)


# ---- inversions ------------------------------------------------------------------------------------------
def inversion_inputs():
    q = Q
    fib = [1, 2]
    while fib[-1] < q:
        fib.append(fib[-1] + fib[-2])
    zs = [0, 1, 2, 3, 5, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 32) + 1, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2,
          q // 3, q // 3 + 1, (1 << 128) - 1, 1 << 128, (1 << 254) + 12345, fib[-2], fib[-3], q - fib[-4],
          pow(2, -1, q), pow(3, -1, q), pow(7, 200, q)]
    zs += [1 << k for k in range(1, 255, 17)] + [(1 << k) - 1 for k in range(2, 255, 19)]
    zs += [q // d for d in (5, 17, 257, 65537, (1 << 31) - 1, (1 << 40) + 3)]
    # inv_step's exact-compare branch: remainders too close to call from the double images
    zs += [q - (1 << k) for k in range(0, 200, 7)] + [(q + 1) // 2 + k for k in (0, 1, 2)] + [q - 1 - fib[-5]]
    zs += [rnd.randrange(1, q) for _ in range(300)]
    return zs


def test_inversions_against_python_integers(probe, inv):
    """fe_invert_euclid (inv29.h) and fe_invert (decode29.h) on raw Montgomery inputs — non-canonical
    representatives, the edge list of the to_hash_inputs test and the exact-compare branch: the result
    is the inverse mod q (0 for 0) and lies inside the prover's bound"""
    N = inv["N"]
    items = []
    for z in inversion_inputs():
        m = z * RM % Q
        for how in ("canon", "low", "some"):
            for k in (0, 1):
                r = spread(m + k * Q, N, how)
                if r is not None and r not in items:
                    items.append(r)
    items += [x for x in edge_set(N)]
    for name in ("fe_invert_euclid", "fe_invert"):
        its = items if name == "fe_invert_euclid" else items[:600]
        outs = probe.run(name, [list(x) for x in its])
        for x, o in zip(its, outs):
            px = plain(x)
            want = pow(px, -1, Q) if px else 0
            assert plain(o) == want, (name, hex(F.val(x)))
            in_bound(o, inv["inverse"], name)
