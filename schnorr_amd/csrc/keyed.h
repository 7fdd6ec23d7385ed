// keyed.h — registered key sets (dsv_keyset_*, include/dsv.h): the per-key fixed-base tables and what
// the host units know about k_keyed.hip (geometry, launchers).  With a table for every point of a key
// the reference's equation is evaluated as written, with no doubling and no scalar reduction:
//   u*Gen + c*PK == R   as   [ -R + u*Gen + c*PK == O ]
// u*Gen: the engine's 16-bit table of G / G' (16 mixed additions), or the key's own Gen table for the
// var-generator scheme; c*PK: the key's table, 32 mixed additions of signed 8-bit windows.
//
// Per-key table of one point P: 32 windows x 129 entries (|digit| = 0 .. 128; entry 0 is the identity),
// entry [w][d] = affine niels of d * 2^(8w) * P in the 144-B layout of the fixed-base tables (v+u, v-u,
// 2d*uv, -2d*uv: 9 x 29-bit limbs each, Montgomery form, canonical), so ext_add_aniels /
// ext_add_aniels_is_identity (jubjub29.h) consume it unchanged.  594 432 B per point.  Key-major: the
// points of one key (PK | PK' for the double scheme, PK | Gen for the var-generator scheme) are adjacent.
#pragma once
#include "launch.h"

namespace dsv {

constexpr int kKeyBits = 8;
constexpr int kKeyWindows = 32;                          // signed 8-bit windows over a scalar < 2^253
constexpr int kKeyEntries = (1 << (kKeyBits - 1)) + 1;   // |digit| = 0 .. 128
constexpr size_t kKeyPointWords = (size_t)kKeyWindows * kKeyEntries * kEntryWords;
constexpr size_t kKeyPointBytes = kKeyPointWords * 4;
static_assert(kKeyPointBytes == 594432, "per-point table size");
static_assert(kKeyWindows * kKeyBits == 256, "the recoding covers 256 bits");

// points per key: single PK; double PK, PK'; var-generator PK, Gen
inline int keyset_points(int scheme) { return scheme == 0 ? 1 : 2; }
// nonce points per signature: single / var-generator R; double R, R'
inline int keyed_sig_points(int scheme) { return scheme == 1 ? 2 : 1; }
// device bytes of a key set: the tables, then one validity byte per key (rounded up to 256)
inline size_t keyset_table_bytes(int scheme, size_t k) { return (size_t)keyset_points(scheme) * k * kKeyPointBytes; }
inline size_t keyset_total_bytes(int scheme, size_t k) {
  return keyset_table_bytes(scheme, k) + (k + 255) / 256 * 256;
}

constexpr int kKeyBuildBlock = 64;
constexpr int kKeyedBlock = 256;
constexpr unsigned kMaxKeyedGrid = 8192;

// ---- k_keyed.hip -------------------------------------------------------------------------------
// tables of k keys from affine points P0 (PK) and P1 (PK' / Gen; null for the single scheme), 64 B each;
// valid_in (may be null): per-key bytes of an earlier stage (wire decoding), AND-ed into key_ok.
// key_ok[key] = every coordinate canonical, every point on the curve (and valid_in[key]).
void launch_build_key_tables(const uint8_t* P0, const uint8_t* P1, const uint8_t* valid_in, int npoints,
                             size_t k, uint32_t* tables, uint8_t* key_ok, hipStream_t s);
// ok[i] = valid[i] & (u < r) & (idx < k) & key_ok[idx] & [every equation holds]; c / valid from
// launch_challenge.  gtab0 / gtab1: the engine's fixed-base tables of G / G' (unused by scheme 2).
void launch_verify_keyed(int scheme, const uint8_t* u, const uint8_t* c, const uint8_t* valid,
                         const uint8_t* R_uv, const uint8_t* Rp_uv, const uint32_t* key_idx, size_t n,
                         const uint32_t* tables, const uint8_t* key_ok, size_t k, const uint32_t* gtab0,
                         const uint32_t* gtab1, uint8_t* ok, hipStream_t s);
// affine u || v (canonical LE) of one table entry, negated for a negative digit
void launch_key_entry(const uint32_t* entry, int negate, uint8_t* out64, hipStream_t s);

}  // namespace dsv

#ifdef DSV_KEYED_KERNELS
#include "common.h"

namespace dsv {

// entry for signed digit d of `window` in a per-key table: load_aniels (common.h) for 129-entry windows
DSV_DEV ANiels load_key_aniels(const u32* __restrict__ table, int window, int d) {
  const bool neg = d < 0;
  const u32 mag = (u32)(neg ? -d : d);
  const u32* p = table + ((size_t)window * kKeyEntries + mag) * kEntryWords;
  ANiels n;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    n.vpu.l[i] = p[(neg ? NL : 0) + i];
    n.vmu.l[i] = p[(neg ? 0 : NL) + i];
    n.t2d.l[i] = p[(neg ? 3 * NL : 2 * NL) + i];
  }
  return n;
}

// signed recoding into 32 digits in [-128, 127]: y = s + 0x8080..80, digit k = byte k of y - 128.
// Exact for s < 2^254 (no carry out of byte 31); the scalars here are u < r < 2^252 and c < 2^250.
DSV_DEV void recode_key(u32 (&y)[8], const u32 (&s)[8]) {
  u32 carry = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u64 t = (u64)s[i] + 0x80808080u + carry;
    y[i] = (u32)t;
    carry = (u32)(t >> 32);
  }
}
// next digit, LSB first; the shift keeps every register index static
DSV_DEV int next_key_digit(u32 (&y)[8]) {
  const int d = (int)(y[0] & 0xffu) - 128;
#pragma unroll
  for (int i = 0; i < 7; i++) y[i] = __funnelshift_r(y[i], y[i + 1], kKeyBits);
  y[7] >>= kKeyBits;
  return d;
}
// acc += s * P from P's per-key table: 32 mixed additions, no doubling
DSV_DEV Ext key_accumulate(Ext acc, const u32 (&s)[8], const u32* __restrict__ table) {
  u32 y[8];
  recode_key(y, s);
#pragma unroll 1
  for (int w = 0; w < kKeyWindows; w++) acc = ext_add_aniels(acc, load_key_aniels(table, w, next_key_digit(y)));
  return acc;
}
// [ acc + s * P == O ], the last addition only as far as the identity test needs it
DSV_DEV bool key_accumulate_is_identity(Ext acc, const u32 (&s)[8], const u32* __restrict__ table) {
  u32 y[8];
  recode_key(y, s);
#pragma unroll 1
  for (int w = 0; w < kKeyWindows - 1; w++) acc = ext_add_aniels(acc, load_key_aniels(table, w, next_key_digit(y)));
  return ext_add_aniels_is_identity(acc, load_key_aniels(table, kKeyWindows - 1, next_key_digit(y)));
}
// acc + (the part of s * P in windows 4 part .. 4 part + 3): eight lanes, part = 0 .. 7, share one
// product; word `part` of the recoding holds its four digits (selected without a dynamic register index)
DSV_DEV Ext key_accumulate_part(Ext acc, const u32 (&s)[8], const u32* __restrict__ table, int part) {
  u32 y[8];
  recode_key(y, s);
  u32 word = y[0];
#pragma unroll
  for (int q = 1; q < 8; q++) word = part == q ? y[q] : word;
#pragma unroll 1
  for (int w = 0; w < 4; w++) {
    const int d = (int)((word >> (kKeyBits * w)) & 0xffu) - 128;
    acc = ext_add_aniels(acc, load_key_aniels(table, 4 * part + w, d));
  }
  return acc;
}

// the verdict of item i (k_verify_keyed, and the gated fallback of the keyed fast accept, k_keyed_rlc.hip):
// the accumulator starts at -R; u*Gen and c*PK are table additions; the verdict is the identity test inside
// the last one.  NCHAIN = 2 (double): both equations share u, c and the key index and run through the same
// code, (G, PK, R) then (G', PK', R').  No table is read for an index out of range.
template <int SCHEME>
DSV_DEV bool keyed_item_ok(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c,
                           const uint8_t* __restrict__ valid, const uint8_t* __restrict__ R_uv,
                           const uint8_t* __restrict__ Rp_uv, const u32* __restrict__ key_idx, size_t i,
                           const u32* __restrict__ tables, const uint8_t* __restrict__ key_ok, size_t k,
                           const u32* __restrict__ gtab0, const u32* __restrict__ gtab1) {
  constexpr int NP = SCHEME == 0 ? 1 : 2;
  constexpr int NCHAIN = SCHEME == 1 ? 2 : 1;
  const u32 idx = key_idx[i];
  if ((size_t)idx >= k) return false;
  bool good = (valid[i] != 0) & (key_ok[idx] != 0);
  u32 us[8], cs[8];
  load_words8(us, u, i);
  load_words8(cs, c, i);
  const bool u_ok = words_lt(us, kR32);
  good &= u_ok;
  if (!u_ok) us[7] &= 0x0fffffffu;  // keep the recodings in range; the verdict is 0 anyway
  const u32* kt = tables + (size_t)idx * NP * kKeyPointWords;
#pragma unroll 1
  for (int h = 0; h < NCHAIN; h++) {
    const uint8_t* Rsrc = h ? Rp_uv : R_uv;
    Fe ru, rv;
    good &= load_fq_signed(ru, Rsrc, 2 * i, true);  // -R
    good &= load_fq(rv, Rsrc, 2 * i + 1);
    Ext acc = ext_from_affine(ru, rv);
    if (SCHEME == 2)
      acc = key_accumulate(acc, us, kt + kKeyPointWords);  // u * Gen from the key's Gen table
    else
      acc = fixed_base_accumulate(acc, us, h ? gtab1 : gtab0);
    good &= key_accumulate_is_identity(acc, cs, kt + (size_t)h * kKeyPointWords);
  }
  return good;
}

}  // namespace dsv
#endif
