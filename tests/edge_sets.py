"""Adversarial base sets with oracle verdicts, for the batch-size dispatch matrix — TEST INFRASTRUCTURE.

One base set per scheme and input form, of a PRIME number of items (no power-of-two aliasing can hide
behind the tiling), shuffled with a fixed seed so that neighbouring items have unrelated verdicts:

* mixed: honest signatures with every harness.tamper class, the structured-relations grid (special keys
  and nonce points, u in {0, 1, r - 1}, m in {0, q - 1}), points with small-order components, malformed
  encodings (u >= r, a coordinate >= q, m >= q) and the form's own edge rows (z = 0, non-canonical z,
  limbs >= the modulus, special compressed encodings): verdicts true and false;
* clean: honest signatures and malformed encodings only — the batch fast accept must accept it.

`base(scheme, form, variant)` -> (arrays in entry-point order, oracle verdicts); built once per process.
`fresh(scheme, form, n, seed)`: a block of freshly signed, tampered items of the same form.
"""
import random

import numpy as np

import harness as H
import mont_cases as MC
import oracle_lib as O
import pymodel as M

Q, R_ORDER = M.Q, M.R_ORDER
FIELDS = {"single": ("u", "R", "PK", "m"), "double": ("u", "R", "Rp", "PK", "PKp", "m"),
          "vargen": ("u", "R", "PK", "Gen", "m")}
POINTS = {s: tuple(f for f in FIELDS[s] if f not in ("u", "m")) for s in FIELDS}
FORMS = ("affine", "ext", "mont", "wire")
TOP = np.full(32, 0xFF, np.uint8)


def _is_prime(n):
    return n > 1 and all(n % p for p in range(2, int(n ** 0.5) + 1))


def _le(x):
    return np.frombuffer(M.le32(x), np.uint8)


def _signed(scheme, n, seed):
    d = getattr(O, "keygen_sign_" + scheme)(n, seed, nthreads=8)
    return {k: d[k].copy() for k in FIELDS[scheme]}


def _cat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _grid(scheme, seed):
    """the structured-relations grid (tests/test_gpu_parity.py test_structured_relations_grid), paired for
    the double / var-generator schemes the way that test pairs it"""
    rnd = np.random.default_rng(seed)
    sqrt_m1 = pow(7, (Q - 1) // 4, Q)
    P = M.pmul(M.GEN, 0x1234567_89ABCDEF)
    specials = [M.IDENTITY, M.GEN, M.pneg(M.GEN), M.GEN_NUMS, M.pneg(M.GEN_NUMS), (0, Q - 1), (sqrt_m1, 0), P,
                M.pneg(P), M.padd(P, P)]
    rows = {k: [] for k in ("u", "R", "PK", "m")}
    for m in (0, Q - 1):
        for pk in specials:
            rr = int(rnd.integers(1, 1 << 62))
            for R in specials[:7] + [M.pmul(M.GEN, rr)]:
                for u in (0, 1, R_ORDER - 1, rr):
                    rows["u"].append(_le(u))
                    rows["R"].append(np.frombuffer(M.point_bytes(R), np.uint8))
                    rows["PK"].append(np.frombuffer(M.point_bytes(pk), np.uint8))
                    rows["m"].append(_le(m))
    g = {k: np.stack(v) for k, v in rows.items()}
    if scheme == "double":
        g["Rp"], g["PKp"] = np.roll(g["R"], 1, axis=0), np.roll(g["PK"], 1, axis=0)
    elif scheme == "vargen":
        g["Gen"] = np.roll(g["PK"], 3, axis=0)
    return {k: g[k] for k in FIELDS[scheme]}


def _torsion(scheme, d, seed):
    """rows of d with an order-8 / order-4 / order-2 component added to one point each"""
    import torsion_model as TM
    t8 = TM.order8_point()
    rnd = random.Random(seed)
    out = {k: v[:24].copy() for k, v in d.items()}
    for i in range(24):
        f = POINTS[scheme][i % len(POINTS[scheme])]
        P = H.to_int_point(out[f][i])
        out[f][i] = np.frombuffer(M.point_bytes(M.padd(P, M.pmul(t8, rnd.choice((1, 2, 4, 5, 7))))), np.uint8)
    return out


def _plant_affine(d, rows):
    """malformed encodings on the given rows: u >= r, v(R) >= q, u(PK) >= q, m >= q (verdict 0 by the
    encoding alone: the reference's types cannot hold them)"""
    for j, i in enumerate(rows):
        [lambda: d["u"].__setitem__(i, TOP), lambda: d["R"][i].__setitem__(slice(32, 64), TOP),
         lambda: d["PK"][i].__setitem__(slice(0, 32), TOP), lambda: d["m"].__setitem__(i, TOP)][j % 4]()


def _special_encodings():
    def enc(v, sign):
        b = bytearray(M.le32(v))
        b[31] |= sign << 7
        return np.frombuffer(bytes(b), np.uint8)
    # (tests/test_gpu_parity.py test_decompress_special_encodings) identity, order 2 / 4, negative zero,
    # non-canonical v, all-ones, a few non-squares
    return [enc(1, 0), enc(1, 1), enc(Q - 1, 0), enc(Q - 1, 1), enc(0, 0), enc(0, 1), enc(Q, 0),
            enc((1 << 255) - 1, 1), enc(2, 0), enc(3, 0), enc(4, 1), enc(5, 0)]


def _par(fn, *arrs):
    """an oracle call over row blocks on a few threads (ctypes releases the GIL; the oracle keeps no state)"""
    from concurrent.futures import ThreadPoolExecutor
    n = arrs[0].shape[0]
    cut = np.linspace(0, n, 9).astype(int)
    with ThreadPoolExecutor(8) as ex:
        parts = list(ex.map(lambda k: fn(*[np.ascontiguousarray(a[cut[k]:cut[k + 1]]) for a in arrs]), range(8)))
    return np.concatenate(parts)


def convert(scheme, form, d, seed, zero_z=(), noncanon_z=(), mont_plant=(), wire_plant=(), wire_special=()):
    """affine items d -> (arrays in the form's entry-point order, oracle verdicts on exactly those bytes).
    ext: (u, uvz..., m) with a random z per point; mont: Montgomery limbs; wire: (sig, pk, m) records.
    The *_plant / zero_z / noncanon_z rows get the form's own malformed encodings."""
    pts = POINTS[scheme]
    rng = np.random.default_rng(seed)
    if form == "affine":
        arrs = [d[k] for k in FIELDS[scheme]]
        return arrs, getattr(O, "verify_" + scheme)(*arrs, nthreads=8)
    if form == "wire":
        comp = {k: O.compress(d[k]) for k in pts}
        specials = _special_encodings()
        for j, i in enumerate(wire_special):
            comp[pts[j % len(pts)]][i] = specials[j % len(specials)]
        for j, i in enumerate(wire_plant):  # undecodable: v = q, v all ones
            comp[pts[j % len(pts)]][i] = specials[6 + (j & 1)]
        nsig = 2 if scheme == "double" else 1
        sig = np.concatenate([d["u"]] + [comp[k] for k in pts[:nsig]], axis=1)
        pk = np.concatenate([comp[k] for k in pts[nsig:]], axis=1)
        arrs = [np.ascontiguousarray(sig), np.ascontiguousarray(pk), d["m"].copy()]
        return arrs, _par(getattr(O, "verify_%s_wire" % scheme), *arrs)
    uvz, ext = {}, {}
    for j, k in enumerate(pts):
        zz = set(i for t, i in enumerate(zero_z) if t % len(pts) == j)
        nz = set(i for t, i in enumerate(noncanon_z) if t % len(pts) == j)
        uvz[k], ext[k] = H.projective(d[k], rng, zero_z=zz, noncanon_z=nz)
    if form == "ext":
        arrs = [d["u"]] + [uvz[k] for k in pts] + [d["m"]]
        want = _par(getattr(O, "verify_%s_ext" % scheme), d["u"], *[ext[k] for k in pts], d["m"])
        want[list(zero_z)] = 0  # z = 0: the reference panics in to_hash_inputs, the engine's verdict is 0
        return arrs, want
    assert form == "mont"
    # limbs of u mod r / m mod q (u >= r and m >= q have no limb form; planted below instead)
    cols = [MC.to_limbs_py(d["u"], R_ORDER)] + [MC.to_limbs_py(uvz[k], Q) for k in pts] + [MC.to_limbs_py(d["m"], Q)]
    for j, i in enumerate(mont_plant):
        kind = j % 4
        if kind == 0:
            cols[1 + (j // 4) % len(pts)][i, 64:96] = 0                 # z = 0
        elif kind == 1:
            cols[1 + (j // 4) % len(pts)][i, 32:64] = 0xFF              # limbs >= q
        elif kind == 2:
            cols[-1][i] = _le(Q)                                         # m limbs = q
        else:
            cols[0][i] = _le(R_ORDER + 5)                                # u limbs >= r
    return cols, _par(getattr(O, "verify_%s_mont" % scheme), *cols)


def _shuffle_to_prime(d, seed):
    """drop d's first rows (honest ones) until the length is prime, shuffle"""
    n = len(d["u"])
    p = n
    while not _is_prime(p):
        p -= 1
    perm = np.random.default_rng(seed).permutation(np.arange(n - p, n))
    return {k: v[perm].copy() for k, v in d.items()}


def _plan_rows(n, count, seed):
    return sorted(np.random.default_rng(seed).choice(n, size=count, replace=False).tolist())


_CACHE = {}
SEED = {"single": 61, "double": 62, "vargen": 63}


def _affine(scheme, variant):
    key = ("affine-items", scheme, variant)
    if key not in _CACHE:
        s = SEED[scheme] + (0 if variant == "mixed" else 10)
        if variant == "mixed":
            honest = _signed(scheme, 1000, s)
            tampered = {k: v[:600].copy() for k, v in honest.items()}
            H.tamper(tampered, kind_single=scheme == "single", period=5)
            tors = _torsion(scheme, {k: v[600:624] for k, v in honest.items()}, s)
            mal = {k: v[624:640].copy() for k, v in honest.items()}
            _plant_affine(mal, range(16))
            d = _cat(honest, tampered, _grid(scheme, s), tors, mal)   # (honest first: trimmed to a prime)
        else:
            d = _signed(scheme, 1620, s)
            _plant_affine(d, _plan_rows(1620, 24, s))
        _CACHE[key] = _shuffle_to_prime(d, s + 1)
    return _CACHE[key]


def base(scheme, form, variant="mixed"):
    """(arrays in entry-point order, oracle verdicts) of the base set; cached"""
    key = (scheme, form, variant)
    if key not in _CACHE:
        d = _affine(scheme, variant)
        n = len(d["u"])
        s = SEED[scheme] * 7 + len(form)
        rows = _plan_rows(n, 64, s)
        if variant == "clean":
            # malformed encodings of the form; affine ones only where the form can carry them (ext / mont / wire
            # points are re-encoded from the affine coordinates)
            e = {k: v.copy() for k, v in d.items()}
            if form != "affine":
                honest = _signed(scheme, n, SEED[scheme] + 10)
                e = honest
                for i in rows[:8]:
                    e["u"][i] = TOP
                for i in rows[8:16]:
                    e["m"][i] = TOP
            kw = {"ext": dict(zero_z=rows[16:24], noncanon_z=rows[24:32]), "mont": dict(mont_plant=rows[:32]),
                  "wire": dict(wire_plant=rows[16:32])}.get(form, {})
            arrs, want = convert(scheme, form, e, s, **kw)
        else:
            kw = {"ext": dict(zero_z=rows[:12], noncanon_z=rows[12:24]), "mont": dict(mont_plant=rows[:24]),
                  "wire": dict(wire_plant=rows[:12], wire_special=rows[12:36])}.get(form, {})
            arrs, want = convert(scheme, form, d, s, **kw)
        arrs = [np.ascontiguousarray(a) for a in arrs]
        _CACHE[key] = (arrs, want)
    return _CACHE[key]


def fresh(scheme, form, n, seed):
    """n freshly signed items, every 5th tampered, in the given form -> (arrays, oracle verdicts)"""
    d = _signed(scheme, n, seed)
    H.tamper(d, kind_single=scheme == "single", period=5)
    arrs, want = convert(scheme, form, d, seed)
    return [np.ascontiguousarray(a) for a in arrs], want
