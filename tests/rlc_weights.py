"""Python-integer model of what the batch fast accept's prep kernels write under a KNOWN weight key —
TEST INFRASTRUCTURE (schnorr_amd/csrc/k_rlc.hip: k_rlc_prep, rlc.h: draw_z / emit_long / emit_short,
k_keyed_rlc.hip: k_keyed_rlc_prep).

Item gi of a group (its place in the group's arrays, whatever sub-group or range it falls into) takes one
ChaCha12 block  blk = chacha_block(key, counter = gi):
  z   = words 0..4 masked to wr c bits      (the first equation's weight; wr = ceil(128 / c) windows)
  z'  = words 8..12, the same mask          (double scheme: the second equation's)
  the keys' scalars  e = z c mod r + (blk[5] % kmul) r,  e' = z' c mod r + (blk[13] % kmul) r,  and the
  var-generator's    z u mod r + (blk[6] % kmul) r   (kmul = floor(2^(wpk c) / r): 17 at 256 bits, 1 at 252)
  f = z u mod r (f' = z' u mod r): the fixed-base scalars (single, double)
Digits are the LSB-first c-bit windows.  An ineligible item has z = 0: all its digits, f and key sums are zero.
"""
import struct

import fe29_model as F
import pymodel as M
import refrng

Q, R_ORDER = M.Q, M.R_ORDER
SCHEMES = ("single", "double", "vargen")
# flags of a sub-group (rlc.h)
OFF_CURVE, TORSION, SUM, OVERFLOW = 1, 2, 4, 8


def geometry(scheme, c, keyed=False):
    """rlc.h: rlc_plan — what does not depend on the item count"""
    wpk = 0 if keyed else -(-252 // c)
    wr = -(-128 // c)
    lpts = 0 if keyed else (1 if scheme == "single" else 2)
    spts = 2 if scheme == "double" else 1
    fixed = {"single": 1, "double": 2, "vargen": 0}[scheme]
    return {"c": c, "wpk": wpk, "wr": wr, "lpts": lpts, "spts": spts, "fixed": fixed,
            "kmul": 17 if wpk * c == 256 else 1, "rows": wpk * lpts + wr * spts, "zbits": wr * c}


def block(key, gi):
    return struct.unpack("<16I", refrng.chacha_block(list(key), gi, rounds=12))


def _z(blk, first, zbits):
    return sum(blk[first + k] << (32 * k) for k in range(5)) & ((1 << zbits) - 1)


def weights(key, gi, c):
    """(z, z') of item gi under `key` with c-bit windows"""
    blk, zbits = block(key, gi), -(-128 // c) * c
    return _z(blk, 0, zbits), _z(blk, 8, zbits)


def digits(x, c, count):
    return [(x >> (c * w)) & ((1 << c) - 1) for w in range(count)]


def item(scheme, key, gi, c, u, chal, good, keyed=False):
    """-> dict: z (one per equation), long {slot: scalar}, short {slot: z}, f [fixed-base scalars],
    rows {row: digit}, ksc [the item's per-key scalars z c (z' c | z u) mod r, keyed]"""
    g = geometry(scheme, c, keyed)
    blk = block(key, gi)
    eqs = 2 if scheme == "double" else 1
    out = {"z": [], "long": {}, "short": {}, "f": [], "rows": {}, "ksc": []}
    for eq in range(eqs):
        z = _z(blk, 8 * eq, g["zbits"]) if good else 0
        out["z"].append(z)
        zc, zu = z * chal % R_ORDER, z * u % R_ORDER
        if not keyed:
            out["long"][eq] = zc + ((blk[8 * eq + 5] % g["kmul"]) * R_ORDER if good else 0)
            if scheme == "vargen":
                out["long"][1] = zu + ((blk[6] % g["kmul"]) * R_ORDER if good else 0)
        out["ksc"].append(zc)
        if scheme == "vargen":
            out["ksc"].append(zu)
        else:
            out["f"].append(zu)
        out["short"][eq] = z
    for slot, e in out["long"].items():
        assert e < 1 << (g["wpk"] * c)
        for w, d in enumerate(digits(e, c, g["wpk"])):
            out["rows"][w * g["lpts"] + slot] = d
    first = g["wpk"] * g["lpts"]
    for slot, z in out["short"].items():
        for w, d in enumerate(digits(z, c, g["wr"])):
            out["rows"][first + w * g["spts"] + slot] = d
    assert len(out["rows"]) == g["rows"]
    return out


def chunk_sums(scalars):
    """the unreduced 32-bit-chunk sums k_keyed_rlc_prep keeps per (sub-group, key, scalar)"""
    return [sum((s >> (32 * j)) & 0xFFFFFFFF for s in scalars) for j in range(8)]


# ---- the stored points: affine niels (v + u, v - u, 2d u v), 9 limbs of 29 bits each, Montgomery form -------
_RINV = pow(F.RMONT, -1, Q)


def fe_value(limbs):
    return F.val([int(x) for x in limbs]) * _RINV % Q


def decode_pt(words):
    """27 words of a stored point -> ((u, v), 2d u v as stored)"""
    a, b, t = fe_value(words[0:9]), fe_value(words[9:18]), fe_value(words[18:27])
    half = pow(2, -1, Q)
    return ((a - b) * half % Q, (a + b) * half % Q), t


def t2d_of(p):
    return 2 * M.D * p[0] * p[1] % Q
