// normalize_items.h — what the kernels that normalise a batch of the reference's in-memory objects share
// (k_normalize_uvz, k_misc.hip; k_normalize_lookup, k_keyed_open_mont.hip): a point's z as a factor of the lane's
// running product, and the conversion of an item's two Montgomery scalars.
#pragma once
#include "common.h"

namespace dsv {

// ------------------------------------------------------------------------------------------
// The z of point i of column `in` ((u, v, z), 3 x 32 B LE per point) as a Montgomery-form factor for Montgomery's
// trick (k_normalize_uvz): ok &= [z is canonical (< q) and != 0]; an offending z is replaced by 1 in the product
// so that it cannot poison the other items of its lane.
// ------------------------------------------------------------------------------------------
DSV_DEV Fe load_z_for_product(const uint8_t* in, size_t i, bool& ok) {
  u32 w[8];
  load_words8(w, in, 3 * i + 2);
  const bool usable = words_lt(w, kQ32) & ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0);
  ok &= usable;
  const Fe z = fe_to_mont(fe_from_words_plain(w));
  return fe_select(usable, z, fe_one());
}
// ------------------------------------------------------------------------------------------
// The reference's in-memory scalars.  `BlsScalar` (dusk-bls12_381 0.13) and `JubJubScalar`
// (dusk-jubjub 0.14; /root/reference/Cargo.toml:25-26) hold `[u64; 4]` MONTGOMERY limbs, R = 2^256:
// the `u` of a Signature (/root/reference/src/signatures.rs:58-61) is u * 2^256 mod r, the message
// handed to verify (/root/reference/src/keys/public.rs:121) is m * 2^256 mod q.  The *_mont entry
// points take those limbs as they lie in memory — the caller runs no `to_bytes()`, i.e. no Montgomery
// reduction, on the host — and the device performs the two reductions: u by one CIOS pass against 1
// (fr.h), m as the fe29 product M * 2^5 * 2^-261.  Limbs that are not below the modulus (the Rust types
// cannot hold them) are poisoned, so the verify kernels give the item verdict 0.  The POINTS of such a
// caller need no conversion: (u R, v R, z R) normalises to the same (u/z, v/z), so they go into
// k_normalize_uvz unchanged.  r04 ran this as a kernel of its own (k_scalars_from_mont: 1024 trivially
// short waves per 2^16 items); r05 calls it from k_normalize_uvz — the host pipeline's preprocessing is
// one launch of few waves.
// ------------------------------------------------------------------------------------------
__device__ constexpr u32 kTwo5[NL] = {32, 0, 0, 0, 0, 0, 0, 0, 0};
DSV_DEV void scalars_from_mont_item(const uint8_t* __restrict__ u_mont, const uint8_t* __restrict__ m_mont, size_t i,
                                    uint8_t* __restrict__ u_out, uint8_t* __restrict__ m_out) {
  u32 w[8], o[8];
  load_words8(w, u_mont, i);
  if (words_lt(w, kR32)) {
    const u32 one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    fr_mont_mul(o, w, one);
    store_words8(u_out, i, o);
  } else {
    store_poison(u_out, i);
  }
  load_words8(w, m_mont, i);
  if (words_lt(w, kQ32)) {
    fe_to_words_plain(o, fe_canon(fe_mul(fe_from_words_plain(w), fe_const(kTwo5))));
    store_words8(m_out, i, o);
  } else {
    store_poison(m_out, i);
  }
}

}  // namespace dsv
