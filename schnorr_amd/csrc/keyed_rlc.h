// keyed_rlc.h — the batch fast accept over a registered key set ("Keyed fast accept"):
// geometry and launchers of k_keyed_rlc.hip, shared with the host unit (dsv_keyed_rlc.hip).
//
// With a table for every registered point the keys leave the bucket pass: sum_i (z_i c_i) PK_idx(i) is
// sum_k s_k PK_k with ONE scalar per (sub-group, key), s_k = sum over the sub-group's items under key k of
// z_i c_i mod r, and s_k PK_k is 32 table additions.  What is left for the buckets is the nonce points with
// their 128-bit weights (rlc_plan(..., keyed = true): no key windows).  A sub-group is accepted iff
//   (1) r * S_p == O for the nonce points' per-bit subset sums (k_rlc_scale, as in the unkeyed pass),
//   (2) every key point an eligible item of the sub-group references passes r * P == O (from its table),
//   (3) single:  (sum z_i u_i) G + sum_k s_k PK_k - sum z_i R_i == O
//       double:  ... + (sum z'_i u_i) G' + sum_k s'_k PK'_k - sum z'_i R'_i
//       vargen:  sum_k a_k Gen_k + sum_k s_k PK_k - sum z_i R_i == O,  a_k = sum z_i u_i over key k
// Eligible: valid byte (hash), u < r, R coordinates < q, idx < k, key_ok[idx].  Others stay out of every sum
// with verdict 0; an eligible R off the curve flags the sub-group (kRlcOffCurve) as in the unkeyed pass.
#pragma once
#include "rlc.h"

namespace dsv {

constexpr int kKeyedLdsKeys = 256;  // sets of at most this many keys sum each workgroup's items in LDS first
constexpr int kKeyParts = 8;        // lanes per key point of a product (four 8-bit windows each)
constexpr int kKeyedTermBlock = 256;
// per-key scalars (and table points they multiply): single s (PK); double s (PK), s' (PK'); vargen s (PK), a (Gen)
inline int keyed_scalars(int scheme) { return scheme == 0 ? 1 : 2; }
// workgroups of k_keyed_rlc_terms per sub-group: kKeyedTermBlock / kKeyParts keys each
inline size_t keyed_term_blocks(size_t k) {
  const size_t per = kKeyedTermBlock / kKeyParts;
  return k ? (k + per - 1) / per : 1;
}

struct KeyedRlcKeys {
  const uint32_t* tables;  // the set's tables (keyed.h), key-major
  const uint8_t* key_ok;
  size_t k;
};
struct KeyedRlcBuffers {
  unsigned long long* ksum;  // groups x k x scalars x 8: the per-key sums as unreduced 32-bit chunks
  uint32_t* touched;         // groups x k: an eligible item of the sub-group references the key
  uint32_t* bad;             // k: a point of the key failed r * P == O
  uint32_t* partial;         // groups x keyed_term_blocks(k) x 36 words: per-workgroup sums of the key terms
  uint32_t* terms;           // groups x 36 words: the key term of each sub-group (extended niels)
};

// per item of the group (blockIdx.y = sub-group): eligibility into ok[], weights from ChaCha12(key, item),
// -R (-R') into the point slots and their digit rows, z u into b.fsc (single / double), the per-key sums into
// kb.ksum / kb.touched.  Zeroes b.counters and the per-key arrays first.  in: u, c, valid, r[0], r[1]
hipError_t launch_keyed_rlc_prep(int scheme, const RlcPlan& p, const RlcBuffers& b, const KeyedRlcBuffers& kb,
                                 const RlcInputs& in, const uint32_t* key_idx, const KeyedRlcKeys& keys,
                                 ChaChaKey key, uint8_t* ok, hipStream_t s);
// the subgroup test of every referenced key point, then s_k PK_k (...) per (sub-group, key) reduced to
// kb.terms[g]; a referenced key that fails the test flags its sub-groups (kRlcTorsion)
hipError_t launch_keyed_rlc_terms(int scheme, const RlcPlan& p, const RlcBuffers& b, const KeyedRlcBuffers& kb,
                                  const KeyedRlcKeys& keys, hipStream_t s);
// the keyed per-signature kernel over the group's items, one launch, blockIdx.y = sub-group: every
// workgroup of a sub-group whose aggregate accepted returns at once (gate: gflags + 4 + 4 g)
void launch_keyed_fallback(int scheme, const RlcPlan& p, const uint8_t* u, const uint8_t* c, const uint8_t* valid,
                           const uint8_t* R_uv, const uint8_t* Rp_uv, const uint32_t* key_idx,
                           const KeyedRlcKeys& keys, const uint32_t* gtab0, const uint32_t* gtab1, uint8_t* ok,
                           const uint32_t* gflags, hipStream_t s);

}  // namespace dsv
