// keyed_lookup.h — the indices of a registered key set over its own keys (dsv_keyset_lookup*,
// dsv_verify_keyed_lookup*, dsv_verify_*_keyed_open*, include/dsv.h): what turns the keys
// of a batch, given by VALUE, into the key_idx column every keyed entry point takes.  A set has one index per key
// form (KeyForm): over the canonical affine bytes callers hold in columns, and over the compressed records
// (`PublicKey*::to_bytes()`) of the same keys.  The record of a valid key is a pure function of its affine bytes
// (v, with bit 255 set to the lowest bit of u), so both are filled from the affine points by byte operations.
//
// One device allocation per index, apart from the tables (keyed.h), made for the set's capacity (the plain
// constructors: k) and never moved:
//   rows   np * 64 B (affine) or np * 32 B (records) per key, key-major (PK | PK' for the double scheme, PK | Gen
//          for the var-generator scheme); rounded up to 256 B
//   slots  `cap` uint32, open addressing: a slot holds a key index or kSlotEmpty; cap = the smallest power
//          of two >= max(64, 2 * capacity), so the table is at most half full; rounded up to 256 B
// Only keys with key_ok == 1 are inserted (their bytes are canonical: every coordinate < q), equal keys share
// one slot that holds the lowest of their indices.  Probing is linear from the key's home slot and wraps.
// The hash (KeyHash over the row's little-endian words) picks the home slot only: a match is always a comparison
// of the whole row.  It is not salted — whoever registers the keys chooses the clusters — and no probe sequence is
// longer than the number of distinct valid keys plus one (the table is never full, and a probe stops at the first
// empty slot).
#pragma once
#include "keyed.h"

namespace dsv {

constexpr uint32_t kSlotEmpty = 0xffffffffu;  // also the index of a miss (DSV_KEY_NONE)
constexpr int kLookupBlock = 256;
constexpr unsigned kMaxLookupGrid = 4096;

inline size_t lookup_round256(size_t x) { return (x + 255) / 256 * 256; }
// slots of a set of k keys (k < 2^32: at most 2^33)
inline size_t keyset_index_cap(size_t k) {
  size_t cap = 64;
  while (cap < 2 * k) cap <<= 1;
  return cap;
}
// the forms a key takes in an index, and the bytes of one key point in each
enum KeyForm { kKeyAffine = 0, kKeyRecord = 1 };
constexpr int kKeyForms = 2;
inline size_t key_point_bytes(KeyForm form) { return form == kKeyAffine ? 64 : 32; }
inline size_t keyset_index_rows_bytes(KeyForm form, int scheme, size_t k) {
  return lookup_round256((size_t)keyset_points(scheme) * key_point_bytes(form) * k);
}
inline size_t keyset_index_total_bytes(KeyForm form, int scheme, size_t k) {
  return k ? keyset_index_rows_bytes(form, scheme, k) + lookup_round256(4 * keyset_index_cap(k)) : 0;
}

// the hash of a row's little-endian words (16 * np affine, 8 * np record); home slot = hash & (cap - 1)
struct KeyHash {
  uint32_t h = 0;
  __host__ __device__ void word(uint32_t w) { h = (h ^ w) * 0x9E3779B1u; }
  __host__ __device__ uint32_t finish() const {
    uint32_t x = h;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
  }
};

// ---- k_keyed_lookup.hip ------------------------------------------------------------------------
// *p = v on `s`, by a one-lane kernel: the single words the capturable by-value calls reset per call (misses, the
// miss list's length).  Not a memset node: in a captured graph, the first replay after a key set was created or
// appended to in between had its 4-byte memset node write another byte value than the captured 0; a kernel node
// keeps its arguments.
void launch_store_word(uint32_t* p, uint32_t v, hipStream_t s);
// Every slot of an index to kSlotEmpty on `s` (mask + 1 slots, a power of two): once, when the set is created.
hipError_t launch_clear_key_index(uint32_t* slots, size_t mask, hipStream_t s);
// m further keys, indices first .. first + m - 1, into the `form` index of a set that holds `first` keys already
// (a fresh set: first = 0): from the affine points P0 / P1 (null for one-point keys) their tables were built from
// and the table build's key_ok for them (earlier on `s`; both start at the first NEW key), writes the keys' rows
// (the affine bytes, or the records formed from them) into `rows` at first + j and inserts the valid keys into
// `slots` (the whole index's, cleared when the set was created).  One lane per new key.  Writes only rows >= first
// and slots that were empty or hold an equal key; may run beside lookups enqueued with k <= first.  The launch's
// error surfaces through hipGetLastError() like every launcher's.
void launch_index_append(KeyForm form, const uint8_t* P0, const uint8_t* P1, const uint8_t* key_ok, int npoints,
                         size_t first, size_t m, uint8_t* rows, uint32_t* slots, size_t mask, hipStream_t s);
// key_idx[i] = the index in the slot of item i's key, else kSlotEmpty.  kKeyAffine: the key's bytes are
// key_a[i] | key_b[i], 64 B each (key_b null for one-point keys); kKeyRecord: its record, 32 * npoints bytes at
// key_a + i * 32 * npoints (key_b null); 16-byte aligned either way.  k: the set's key count as the call sees it —
// an occupant >= k (appended since) is read as an empty slot; misses (may be null): zeroed on `s`
// (launch_store_word), then the number of items that got kSlotEmpty.  One lane per item, grid-stride.
hipError_t launch_index_lookup(KeyForm form, const uint8_t* key_a, const uint8_t* key_b, int npoints, size_t n,
                               const uint8_t* rows, const uint32_t* slots, size_t mask, size_t k, uint32_t* key_idx,
                               uint32_t* misses, hipStream_t s);

// ---- k_keyed_replace.hip: keys replaced in place (dsv_keyset_replace*) -----------------------
// m keys built in a scratch of the call's own — tables (m * npoints tables, key-major), key_ok (m bytes), and the
// affine points they were built from (P0 / P1 as for launch_index_append) — scattered into the set: key j's tables,
// key_ok byte, affine index row and record index row (formed from the point as the append forms it) go to index
// indices[j] (device memory, m pairwise distinct indices below the set's k).  16-byte loads and stores, grid-stride.
void launch_replace_commit(int npoints, const uint32_t* indices, size_t m, const uint32_t* src_tables,
                           const uint8_t* src_key_ok, const uint8_t* P0, const uint8_t* P1, uint32_t* tables,
                           uint8_t* key_ok, uint8_t* affine_rows, uint8_t* record_rows, hipStream_t s);
// the affine index rows of k keys (key-major) as the planar columns P0 [, P1] launch_index_append reads
void launch_rows_to_planar(int npoints, const uint8_t* affine_rows, size_t k, uint8_t* P0, uint8_t* P1,
                           hipStream_t s);
// The canonical layout of the `form` index over keys 0 .. k - 1 — what inserting them one after the other in index
// order gives: each valid key that equals no valid key of lower index in the first empty slot from its home slot
// on.  reps: a slot array of the same size that holds exactly those keys' indices, in any layout (what
// launch_index_append at first = 0 leaves in a cleared array); slots: the index's own, cleared earlier on `s`.  One
// lane per slot of reps; the keys' bytes come from the affine rows (the record form: its rows' bytes formed from
// them).
void launch_index_reinsert(KeyForm form, int npoints, const uint8_t* affine_rows, const uint32_t* reps,
                           uint32_t* slots, size_t mask, hipStream_t s);

}  // namespace dsv

#ifdef DSV_INDEX_KERNELS
// what the kernel units of the indices share (k_keyed_lookup.hip, k_keyed_replace.hip, k_keyed_open_mont.hip,
// k_keyed_census.hip)
namespace dsv {
namespace {

// a row in registers: W x 16 B
template <int W>
struct Words {
  uint4 q[W];
};
template <int W>
__device__ __forceinline__ Words<W> load_row(const uint8_t* __restrict__ rows, size_t i) {
  Words<W> w;
  const uint4* p = reinterpret_cast<const uint4*>(rows + i * (size_t)(16 * W));
#pragma unroll
  for (int j = 0; j < W; j++) w.q[j] = p[j];
  return w;
}
__device__ __forceinline__ bool same16(const uint4& x, const uint4& y) {
  return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) == 0u;
}
template <int W>
__device__ __forceinline__ bool same_words(const Words<W>& a, const Words<W>& b) {
  bool eq = true;
#pragma unroll
  for (int j = 0; j < W; j++) eq &= same16(a.q[j], b.q[j]);
  return eq;
}
template <int W>
__device__ __forceinline__ uint32_t home_hash(const Words<W>& w) {
  KeyHash h;
#pragma unroll
  for (int j = 0; j < W; j++) {
    h.word(w.q[j].x);
    h.word(w.q[j].y);
    h.word(w.q[j].z);
    h.word(w.q[j].w);
  }
  return h.finish();
}

// ------------------------------------------------------------------------------------------
// The lookup's walk (k_index_lookup, k_keyed_lookup.hip; k_normalize_lookup, k_keyed_open_mont.hip): from the home
// slot of the row w, compare against the index's copy of each occupant's row; the walk ends at the first empty
// slot.  k (> 0): the set's key count when the call was enqueued.  An occupant >= k was appended since: it is read
// as an empty slot and ends the walk.  That is exact: every key below k whose walk passes this slot was placed
// while the slot was still empty, so it sits in front of it.  Returns the occupant's index, or kSlotEmpty.  A set
// without an index (k = 0, no rows, no slots) is the caller's to keep away.
// ------------------------------------------------------------------------------------------
template <int W>
__device__ __forceinline__ uint32_t walk_index(const Words<W>& w, const uint8_t* __restrict__ rows,
                                               const uint32_t* __restrict__ slots, size_t mask, size_t k) {
  uint32_t found = kSlotEmpty;
  size_t slot = home_hash<W>(w) & mask;
#pragma unroll 1
  for (size_t probe = 0;; probe++) {
    const uint32_t occ = slots[slot];
    if (occ >= k) break;  // empty (kSlotEmpty >= k), or a key newer than this call
    if (same_words<W>(w, load_row<W>(rows, occ))) {
      found = occ;
      break;
    }
    if (probe == mask) break;  // unreachable: the table is at most half full, an empty slot ends the walk first
    slot = (slot + 1) & mask;
  }
  return found;
}
// The walk for a caller that may hold a set without an index (k = 0: no rows, no slots): nothing is read and every
// key misses.  What the census runs per item (k_keyed_census.hip).
template <int W>
__device__ __forceinline__ uint32_t find_key(const Words<W>& w, const uint8_t* __restrict__ rows,
                                             const uint32_t* __restrict__ slots, size_t mask, size_t k) {
  return k ? walk_index<W>(w, rows, slots, mask, k) : kSlotEmpty;
}

// ---- the key forms: W = 16-byte words per row; source(P0, P1, j) = the row of the affine source key j (u || v,
// 64 B per point), item(key_a, key_b, i) = the row of a batch's item i, occupant(...) = the row of the occupant
// `old` of a slot as the append kernel compares it: a key of an earlier call (old < first) from the index's own
// rows, a lane of this launch from the source points ----------------------------------------------------------

// kKeyAffine: 64 B per point, the source key's bytes as they are; an item's columns are read the same way
template <int NP>
struct AffineKey {
  static constexpr int W = 4 * NP;
  static __device__ __forceinline__ Words<W> source(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                    size_t i) {
    Words<W> w;
    const uint4* pa = reinterpret_cast<const uint4*>(a + i * 64);
#pragma unroll
    for (int j = 0; j < 4; j++) w.q[j] = pa[j];
    if (NP == 2) {
      const uint4* pb = reinterpret_cast<const uint4*>(b + i * 64);
#pragma unroll
      for (int j = 0; j < 4; j++) w.q[4 * (NP - 1) + j] = pb[j];
    }
    return w;
  }
  static __device__ __forceinline__ Words<W> item(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                  size_t i) {
    return source(a, b, i);
  }
  // one pointer select, one load (a pair of loads under `old < first` costs NP = 2 nine VGPRs and a wave of
  // occupancy)
  static __device__ __forceinline__ Words<W> occupant(const uint8_t* __restrict__ P0, const uint8_t* __restrict__ P1,
                                                      const uint8_t* rows, uint32_t old, size_t first) {
    const bool older = old < first;
    const uint8_t* pa = older ? rows + (size_t)old * (size_t)(64 * NP) : P0 + (size_t)(old - first) * 64;
    const uint8_t* pb = older ? pa + 64 : P1 + (size_t)(old - first) * 64;
    return source(pa, pb, 0);
  }
};

// kKeyRecord: 32 B per point, the compressed record of the source point — v, bit 255 = the lowest bit of u —
// formed by byte operations; an item's record is one row at key_a (key_b unused)
template <int NP>
struct RecordKey {
  static constexpr int W = 2 * NP;
  static __device__ __forceinline__ Words<W> source(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                    size_t i) {
    Words<W> w;
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const uint4* pt = reinterpret_cast<const uint4*>((p ? b : a) + i * 64);
      const uint32_t sign = pt[0].x << 31;
      w.q[2 * p] = pt[2];
      w.q[2 * p + 1] = pt[3];
      w.q[2 * p + 1].w = (w.q[2 * p + 1].w & 0x7fffffffu) | sign;
    }
    return w;
  }
  static __device__ __forceinline__ Words<W> item(const uint8_t* __restrict__ a, const uint8_t* __restrict__,
                                                  size_t i) {
    return load_row<W>(a, i);
  }
  static __device__ __forceinline__ Words<W> occupant(const uint8_t* __restrict__ P0, const uint8_t* __restrict__ P1,
                                                      const uint8_t* rows, uint32_t old, size_t first) {
    return old < first ? load_row<W>(rows, old) : source(P0, P1, old - first);
  }
};

}  // namespace
}  // namespace dsv
#endif
