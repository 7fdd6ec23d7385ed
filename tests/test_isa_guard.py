"""ISA regression guard (no GPU): the dominant kernels are compiled to gfx950 assembly and their
register budget, spills, occupancy and the instruction counts of the field multiplier are pinned.

Why: the 189-instruction `fe_mul` rests on `mad_pin` (schnorr_amd/csrc/fe29.h) steering LLVM's
reassociation, and `k_verify_fixed_half` sits exactly on the 256-VGPR / two-waves-per-SIMD budget —
a toolchain bump or an innocent edit can cost 10 % without any test failing.
The limits are the measured values of the shipped build (profiles/r03/isa_hist.json, unchanged since)
plus a small margin; a FASTER build simply passes.  What the kernels compute:
/root/reference/src/keys/public.rs:121-130 (verify), src/signatures.rs:127-134 (challenge hash).

Assembly is cached under build/isa/ by source + header + compiler hash, so only the first run after a
change pays the ~80 s of hipcc.
"""
import concurrent.futures
import os
import shutil
import sys

import pytest

from isa_asm import CSRC, ROOT, _asm, _kernel_info, _stamp

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="hipcc not available")


@pytest.fixture(scope="module")
def isa():
    import isa_hist as H
    stamp = _stamp()
    probe = os.path.join(ROOT, "build", "isa", "probe_%s.hip" % stamp)
    os.makedirs(os.path.dirname(probe), exist_ok=True)
    if not os.path.exists(probe):
        with open(probe, "w") as f:
            f.write(H.PROBE % {"csrc": CSRC})
    units = {"verify": os.path.join(CSRC, "k_verify.hip"), "hash": os.path.join(CSRC, "k_hash.hip"), "probe": probe,
             "rlc": os.path.join(CSRC, "k_rlc.hip")}
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        paths = dict(zip(units, ex.map(lambda p: _asm(p, stamp), units.values())))
    return {"info": {k: _kernel_info(v) for k, v in paths.items()},
            "hist": {k: H.parse(v) for k, v in paths.items()}}


def _find(d, needle):
    hits = [k for k in d if needle in k]
    assert len(hits) == 1, (needle, hits)
    return d[hits[0]]


def test_field_multiplier_instruction_counts(isa):
    """fe_mul: 154 v_mad_u64_u32 + 36 others, fe_sqr: 118 + 44 (probe kernel minus the empty probe)"""
    hist = isa["hist"]["probe"]
    base = _find(hist, "k_probe_empty")["static"]
    valu = lambda name: {k: n - base.get(k, 0) for k, n in _find(hist, name)["static"].items() if k.startswith("v_")}
    mul, sqr = valu("k_probe_fe_mul"), valu("k_probe_fe_sqr")
    # (the probes' own loads / address arithmetic are what the empty probe contains too; its one fe_add
    #  is subtracted with it, so the bound below has 9 v_add of slack on top of the measured 190 / 162)
    assert mul.get("v_mad_u64_u32", 0) <= 154, mul
    assert sqr.get("v_mad_u64_u32", 0) <= 118, sqr
    total = lambda v: sum(n for n in v.values() if n > 0)
    assert total(mul) <= 190, (total(mul), mul)
    assert total(sqr) <= 162, (total(sqr), sqr)


def test_verify_kernel_register_budget(isa):
    """k_verify_fixed_half: exactly the two-waves-per-SIMD budget, the shipped spill level, no growth of
    the instruction stream"""
    for chains, scratch_max, spill_max in ((1, 176, 60), (2, 232, 62)):
        k = _find(isa["info"]["verify"], "k_verify_fixed_halfILi%dE" % chains)
        assert k["vgprs"] <= 256 and k["agprs"] == 0, k
        assert k["occupancy"] == 2, k
        assert k["scratch"] <= scratch_max, k          # shipped: 168 / 224 bytes per lane, outside the window loop
        assert k["vgpr_spill_count"] <= spill_max, k   # shipped: 57 / 59
        h = _find(isa["hist"]["verify"], "k_verify_fixed_halfILi%dE" % chains)
        assert h["static_total"] <= 26800, h["static_total"]   # shipped: 26 506 / 26 572
        mad = h["static"].get("v_mad_u64_u32", 0)
        assert mad <= 16900, mad                               # shipped: 16 731: the algorithm's multiplications


def test_hash_kernel_does_not_spill(isa):
    """k_challenge<true> (double signatures: two trips through one permutation body) keeps its state in
    registers: 0 spilled VGPRs (r03: 190 -> 0); the single hash at most its two"""
    dbl = _find(isa["info"]["hash"], "k_challengeILb1E")
    sgl = _find(isa["info"]["hash"], "k_challengeILb0E")
    assert dbl["vgpr_spill_count"] == 0 and dbl["vgprs"] <= 256 and dbl["occupancy"] == 2, dbl
    assert sgl["vgpr_spill_count"] <= 2 and sgl["vgprs"] <= 256 and sgl["occupancy"] == 2, sgl
    assert dbl["scratch"] <= 64 and sgl["scratch"] <= 64, (dbl, sgl)


def test_batch_fast_accept_kernels_stay_in_registers(isa):
    """k_rlc.hip: no kernel of the bucket pass touches scratch memory — in particular the
    four-waves-per-point tail (k_rlc_scale), whose first version selected operands with a struct-level ?:
    that the compiler turned into a scratch array indexed by the wave number (1.45 ms instead of 0.57) —
    and the bucket accumulation keeps four waves per SIMD."""
    info = {k: v for k, v in isa["info"]["rlc"].items() if "k_rlc_" in k}
    assert len(info) >= 16, sorted(info)          # prep x 3, part1, part2, lenhist, order, accumulate, merge, sum x 4, scale, sample_decide, verdict, chain
    for name, k in info.items():
        assert k["scratch"] == 0 and k["vgpr_spill_count"] == 0, (name, k)
    acc = _find(info, "k_rlc_accumulate")
    assert acc["vgprs"] <= 128 + 8 and acc["occupancy"] >= 3, acc      # shipped: 132 VGPRs
    scale = _find(info, "k_rlc_scale")
    assert scale["vgprs"] <= 192, scale                                  # shipped: 165
