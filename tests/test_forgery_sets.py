"""CPU checks of tests/forgery_sets.py: what tests/test_gpu_rlc_forgery.py relies on holds by the ORACLE and
the Python-integer model alone — in every forged batch exactly the forged items are wrong, and the plain
(unweighted) sum of their defects u G + c PK - R is the identity, so only distinct weights reject it."""
import numpy as np
import pytest

import forgery_sets as F
import pymodel as M

SCHEMES = ("single", "double", "vargen")
UNKEYED = [(s, kind, pair) for s in SCHEMES for kind, pair in F.unkeyed_cases(s)]
KEYED = [(s, k, kind, same) for s in SCHEMES for k in F.KEY_COUNTS for kind, same in F.keyed_cases(s, k)]


def _check(f, want_fn, keys=None):
    n = len(f.forged["u"])
    want = np.ones(n, np.uint8)
    want[f.items] = 0
    assert np.array_equal(want_fn(f.forged), want), "the oracle rejects other items than the forged ones"
    assert want_fn(f.honest).all(), "the control batch is not all valid"
    for i in f.items:
        assert any(d != M.IDENTITY for d in F.defects(f.scheme, f.forged, i, keys))
        for col in ("R", "Rp", "PK", "PKp", "Gen"):
            if f.forged.get(col) is not None:
                assert M.on_curve(F.as_point(f.forged[col][i]))
    assert F.defect_sum(f.scheme, f.forged, f.items, keys) == M.IDENTITY, "the defects do not cancel"


@pytest.mark.parametrize("scheme,kind,pair", UNKEYED, ids=["%s-%s-%d-%d" % (s, k, p[0], p[1]) for s, k, p in UNKEYED])
def test_unkeyed_forgeries_cancel_in_a_plain_sum(scheme, kind, pair):
    f = F.forge(scheme, kind, pair)
    assert len(f.forged["u"]) == F.N
    _check(f, lambda a: F.oracle(scheme, a))


@pytest.mark.parametrize("scheme,k,kind,same", KEYED, ids=["%s-k%d-%s-%s" % (s, k, kd, "one" if sm else "two") for s, k, kd, sm in KEYED])
def test_keyed_forgeries_cancel_in_a_plain_sum(scheme, k, kind, same):
    f = F.forge_keyed(scheme, kind, k, (5, 69), same_key=same)
    assert len(f.keys[0]) == (k + 2 if kind == "key" else k)
    if not same:
        assert f.forged["idx"][5] != f.forged["idx"][69]
    _check(f, lambda a: F.keyed_oracle(scheme, a, f.keys), f.keys)


def test_weighted_forgeries_cancel_under_their_weights_only():
    """forge(..., wi, wj): the defects are wj X and -wi X — their plain sum is not the identity, the sum weighted
    with (wi, wj) is"""
    wi, wj = 0x1234567890ABCDEF1122334455667788, 0xFEDCBA09876543218877665544332211
    for scheme, kind, pair in (("single", "R", (5, 69)), ("vargen", "Gen", (5, 69)), ("double", "cross", (5, 5))):
        f = F.forge(scheme, kind, pair, wi=wi, wj=wj)
        assert F.defect_sum(scheme, f.forged, f.items) != M.IDENTITY
        if kind == "cross":
            d = F.defects(scheme, f.forged, 5)
            assert M.padd(M.pmul(d[0], wi), M.pmul(d[1], wj)) == M.IDENTITY
        else:
            di, dj = F.defects(scheme, f.forged, pair[0])[0], F.defects(scheme, f.forged, pair[1])[0]
            assert M.padd(M.pmul(di, wi), M.pmul(dj, wj)) == M.IDENTITY
