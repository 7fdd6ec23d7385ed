"""Worst-case (all-inputs) overflow proof of the lazy-reduction bookkeeping in fe29.h /
jubjub29.h — see tests/fe29_bounds.py.  CPU only."""
import pytest

import fe29_bounds as FB


def test_group_law_bounds_reach_a_fixpoint_without_overflow():
    inv = FB.prove_group_law()
    acc = inv["acc"]
    # what the comments in jubjub29.h promise: multiplication outputs are "N"
    for k in ("u", "v", "z"):
        assert acc[k].l[0] <= FB.M29 + 1           # limb 0 takes the accumulator's missing 1 back
        assert all(x <= FB.M29 for x in acc[k].l[1:8])
        assert acc[k].v < 2 * FB.Q
    assert inv["rounds"] < 10


def test_prover_rejects_a_broken_variant():
    """Sanity of the prover itself: dropping BOTH carry passes of the doubling must be refused."""
    def bad_double(p):
        uu, vv = FB.sqr(p["u"]), FB.sqr(p["v"])
        zz2 = FB.dbl(FB.sqr(p["z"]))
        cu = FB.dbl(FB.mul(p["u"], p["v"]))
        vpu = FB.add(vv, uu)
        vmu = FB.sub_raw(vv, uu, 2)
        ct = FB.sub_raw(zz2, vmu, 4)
        return {"u": FB.mul(cu, ct), "v": FB.mul(vpu, vmu), "z": FB.mul(vmu, ct), "t1": cu, "t2": vpu}

    n = FB.mul(FB.canonical(), FB.canonical())
    with pytest.raises(FB.OverflowError_):
        bad_double({"u": n, "v": n, "z": n, "t1": n, "t2": n})


def test_hades_permutation_cannot_overflow_with_the_shipped_constants():
    """S-boxes on the VALU between rows that come back from the matrix cores (hades29.h)"""
    out = FB.prove_hades()
    assert out["hash3"].v < 3 * FB.Q and out["hash5"].v < 3 * FB.Q


def test_point_decompression_field_code_cannot_overflow():
    FB.prove_decompress()


def test_normalisation_and_limb_conversion_field_code_cannot_overflow():
    """r04: k_scalars_from_mont and k_normalize_uvz with the Euclidean inversion (inv29.h)"""
    out = FB.prove_normalize_and_limb_conversion()
    assert out["quotient"].v < 3 * FB.Q


def test_batch_fast_accept_field_code_cannot_overflow():
    """r05, k_rlc.hip: the curve test, the affine-niels form of decoded points and the four-waves-per-point
    operations (running point with tt = t1 * t2) stay inside the group law's proven invariants"""
    out = FB.prove_fast_accept()
    assert out["rounds"] < 12 and out["acc"]["u"].v < 2 * FB.Q


def test_hades_stage_bounds_are_returned_and_self_consistent():
    """prove_hades() also hands out the per-stage bounds the device limb tests draw ceilings from: the
    S-box proves on the joined S-box input bound, and its output is a valid matrix-core operand"""
    out = FB.prove_hades()
    for k in ("permute_in", "round_in", "sbox_in", "mds_operand", "row", "partial_in"):
        assert isinstance(out[k], FB.B)
    FB.mfma_operand_ok(FB.sbox(out["sbox_in"]), "S-box of the joined input bound")
    assert FB.leq(out["row"], FB.mfma_row())


def test_quad_group_law_bounds_reach_a_fixpoint_without_overflow():
    """quad29.h / k_quad.hip: the four-lanes-per-point chain of k_verify_fixed_half_oct (qext_mul16,
    qext_add_niels of variable-base entries, qext_add_aniels of fixed-base entries, the octet combine
    and the final comparisons) cannot overflow for any input inside the group law's invariants"""
    out = FB.prove_quad_group_law()
    for k in ("u", "v", "z", "t"):
        assert out["acc"][k].l[0] <= FB.M29 + 1
        assert all(x <= FB.M29 for x in out["acc"][k].l[1:8])
        assert out["acc"][k].v < 2 * FB.Q
        assert out["out"][k].v < 2 * FB.Q
    assert out["rounds"] < 12


def test_quad_prover_rejects_a_broken_variant():
    """Sanity of the quad proof: an octet combine whose v - u operand skips its carry pass (fe_sub2_raw
    for fe_sub2) multiplies two un-carried operands and must be refused"""
    def bad_octet_niels(acc, d2):
        n = FB.octet_niels(acc, d2)
        n["vmu"] = FB.sub_raw(acc["v"], acc["u"], 2)
        return n

    with pytest.raises(FB.OverflowError_):
        FB.prove_quad_group_law(octet_niels=bad_octet_niels)
    # and a quad doubling whose ct = 2 z^2 - (v^2 - u^2) skips fe_sub4w's carry pass
    n = FB.mul(FB.canonical(), FB.canonical())
    p = {"u": n, "v": n, "z": n, "t": n}
    uu, vv = FB.mul(p["u"], p["u"]), FB.mul(p["v"], p["v"])
    vmu = FB.sub_raw(vv, uu, 2)
    with pytest.raises(FB.OverflowError_):
        FB.mul(vmu, FB.sub_raw(FB.dbl(FB.mul(p["z"], p["z"])), vmu, "4w"))
