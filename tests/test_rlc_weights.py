"""CPU checks of tests/rlc_weights.py, the Python-integer model of the fast accept's weights: its geometry is
the engine's plan, its digits recompose to the scalars they came from, and the scalars are what the header
of k_rlc.hip states."""
import random

import pytest

import pymodel as M
import rlc_weights as W

KEY = (0x03020100, 0x07060504, 0x0B0A0908, 0x0F0E0D0C, 0x13121110, 0x17161514, 0x1B1A1918, 0x1F1E1D1C)


@pytest.mark.parametrize("scheme", W.SCHEMES)
@pytest.mark.parametrize("c", (4, 6, 8, 12, 14, 16))
def test_geometry_is_the_engines_plan(scheme, c):
    from schnorr_amd import engine as E
    for keyed in (False, True):
        plan = E.keyed_rlc_plan_info(scheme, 777, 5, c, 1) if keyed else E.rlc_plan_info(scheme, 777, c, 1)
        g = W.geometry(scheme, c, keyed)
        for k in ("c", "wpk", "wr", "lpts", "spts", "fixed", "rows"):
            assert g[k] == plan[k], (k, keyed)
        if not keyed:
            assert g["kmul"] == plan["kmul"] == (1 << (g["wpk"] * c)) // M.R_ORDER


@pytest.mark.parametrize("scheme", W.SCHEMES)
@pytest.mark.parametrize("c", (8, 12))
def test_digits_recompose_to_the_scalars(scheme, c):
    rnd = random.Random(c)
    g = W.geometry(scheme, c)
    seen = set()
    for gi in (0, 1, 255, 256, 1542, (1 << 32) + 5):
        u, chal = rnd.randrange(M.R_ORDER), rnd.randrange(1 << 250)
        it = W.item(scheme, KEY, gi, c, u, chal, True)
        z, zp = W.weights(KEY, gi, c)
        assert it["z"] == ([z, zp] if scheme == "double" else [z])
        assert z.bit_length() > 64 and zp.bit_length() > 64 and z != zp and z < 1 << g["zbits"]
        assert z not in seen and zp not in seen
        seen.update((z, zp))
        for slot, e in it["long"].items():
            got = sum(it["rows"][w * g["lpts"] + slot] << (c * w) for w in range(g["wpk"]))
            assert got == e
            weight = it["z"][slot] if scheme == "double" else z
            scalar = u if (scheme == "vargen" and slot == 1) else chal
            assert e % M.R_ORDER == weight * scalar % M.R_ORDER and e // M.R_ORDER < g["kmul"]
        first = g["wpk"] * g["lpts"]
        for slot, zz in it["short"].items():
            assert sum(it["rows"][first + w * g["spts"] + slot] << (c * w) for w in range(g["wr"])) == zz
        assert it["f"] == ([] if scheme == "vargen" else [w * u % M.R_ORDER for w in it["z"]])
        bad = W.item(scheme, KEY, gi, c, u, chal, False)
        assert not any(bad["rows"].values()) and not any(bad["f"]) and not any(bad["ksc"]) and not any(bad["z"])


def test_chunk_sums_are_the_sum():
    rnd = random.Random(3)
    xs = [rnd.randrange(M.R_ORDER) for _ in range(50)]
    assert sum(v << (32 * j) for j, v in enumerate(W.chunk_sums(xs))) == sum(xs)


def test_stored_point_round_trip():
    import fe29_model as F
    p = M.pmul(M.GEN, 12345)
    words = F.to_mont_int((p[1] + p[0]) % M.Q) + F.to_mont_int((p[1] - p[0]) % M.Q) + F.to_mont_int(W.t2d_of(p))
    assert W.decode_pt(words) == (p, W.t2d_of(p))
