// keyed_mont.h — the keyed typed-object form (dsv_keyset_create_mont_cols, dsv_verify_keyed_mont_*,
// include/dsv.h): the reference's in-memory objects — Montgomery limbs, projective points — verified against a
// registered key set.  No kernel of its own: the normalisation kernel of the unkeyed *_mont forms over the
// signature's nonce points alone, in front of what a keyed call does anyway:
//   k_normalize_uvz<1 | 2>   R [, R'] (u, v, z limbs) -> affine bytes, u / m limbs -> canonical bytes, valid
//   k_challenge              valid enters as the hash's valid_in
//   k_verify_keyed<SCHEME>
// and, in the constructor, over the key points in front of k_build_key_tables.  Host code only (dsv_keyed_mont.hip;
// dsv_host.hip for the job driver).
#pragma once
#include "keyset_host.h"

namespace dsvh {

// columns of a keyed typed batch: u, R [, R'], key_idx, m
inline int keyed_mont_columns(int scheme) { return 3 + keyed_sig_points(scheme); }
// width of column c
inline size_t keyed_mont_width(int scheme, int c) {
  const int np = keyed_sig_points(scheme);
  return c == 0 || c == np + 2 ? 32 : (c <= np ? 96 : 4);
}

// what the normalisation launch writes for n items, in this order (dsv_keyed_mont_workspace_bytes): u, m, R,
// R' (double scheme only), valid, the kernel's prefix scratch; each part rounded up to 256 B
inline size_t keyed_mont_cols_bytes(int scheme, size_t n) {
  const int np = keyed_sig_points(scheme);
  return 2 * align_up(n * 32, 256) + (size_t)np * align_up(n * 64, 256) + align_up(n, 256) +
         align_up(normalize_prefix_bytes(n, np), 256);
}
KeyedCols carve_keyed_mont(Stager& x, int scheme, size_t n);
// u, m: n x 32 B Montgomery limbs; R [, Rp]: n x 96 B limbs of u || v || z (device memory) -> w, one launch on
// `stream`; per_lane / block: the launch shape (0: the kernel's defaults)
void normalize_keyed_mont(int scheme, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* m,
                          size_t n, const KeyedCols& w, hipStream_t stream, int per_lane = 0, int block = 0);

// argument checks of a keyed column batch, before the set is looked at: n, the set pointer, then every
// column's pointer, stride and (key_idx) alignment ("column k: ...").  The scheme is read under the
// registry's shared lock, which the caller holds.
int check_keyed_mont_cols(const dsv_keyset* ks, const dsv_column* cols, size_t n, const uint8_t* ok);
// the host form's body; the caller holds the registry's shared lock from here to the last verdict
int verify_keyed_mont_cols_locked(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok);

// dsv_keyed_open_mont.hip: the open typed form's host body — cols: u, the scheme's points, m, as
// dsv_verify_*_mont_cols takes them; *misses (may be null) = the items that took the unkeyed path.  The caller
// holds the registry's shared lock from here to the last verdict
int verify_keyed_open_mont_cols_locked(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok,
                                       size_t* misses);
constexpr int kOpenMontJob = 1;  // submit_cols_job's `kind` of a keyed job that runs the open form (0: by index)

// dsv_host.hip: a column batch as a job on a driver thread (dsv_job).  ks null: the unkeyed typed-object form
// of scheme `kind`; else a keyed form (kind 0: by key index, kOpenMontJob: the open form), whose driver holds the
// registry's shared lock from before submit returns until its last verdict
int submit_cols_job(const dsv_keyset* ks, int kind, const dsv_column* cols, int ncols, size_t n, uint8_t* ok,
                    dsv_job** out);

}  // namespace dsvh
