// keyed_open_wire.h — the key cache for serialized records (dsv_keyset_lookup_wire*, dsv_verify_*_keyed_open_wire*,
// include/dsv.h): a second index in every key set, over the COMPRESSED records of its own valid
// keys — `PublicKey*::to_bytes()`, the form the cache's inputs arrive in — and the decompression of the keys of the
// items that missed.  The record of a valid registered key is a pure function of its affine bytes (v, with bit 255
// set to the lowest bit of u), so a hit is found by byte operations alone; only a miss pays for a square root.
//
// One device allocation per set, apart from the tables (keyed.h) and the affine index (keyed_lookup.h), made for
// the set's capacity and never moved:
//   records  np * 32 B per key, key-major (pk | pk' for the double scheme, pk | gen for the var-generator scheme);
//            rounded up to 256 B
//   slots    keyset_index_cap(capacity) uint32, open addressing exactly as in keyed_lookup.h: a slot holds a key
//            index or kSlotEmpty, linear probing from the home slot, at most half full; rounded up to 256 B
// Only keys with key_ok == 1 are inserted, equal keys share one slot that holds the lowest of their indices.  The
// home slot is KeyHash over the record's 8 * np little-endian words; a match is a comparison of all 32 * np bytes.
#pragma once
#include "keyed_lookup.h"

namespace dsv {

inline size_t keyset_wire_records_bytes(int scheme, size_t k) {
  return lookup_round256((size_t)keyset_points(scheme) * 32 * k);
}
inline size_t keyset_wire_index_total_bytes(int scheme, size_t k) {
  return k ? keyset_wire_records_bytes(scheme, k) + lookup_round256(4 * keyset_index_cap(k)) : 0;
}

// ---- k_keyed_open_wire.hip ---------------------------------------------------------------------
// launch_append_key_index for the wire index (fresh set: first = 0): the m new keys' records are formed from the
// affine points P0 / P1 (null for one-point keys; both start at the first NEW key) by byte operations, written to
// `records` at row first + j, and the keys with key_ok == 1 inserted into `slots` (the whole wire index's, cleared
// when the set was created).  One lane per new key.  Writes only rows >= first and slots that were empty or hold
// an equal key; may run beside lookups enqueued with k <= first.
void launch_append_wire_index(const uint8_t* P0, const uint8_t* P1, const uint8_t* key_ok, int npoints, size_t first,
                              size_t m, uint8_t* records, uint32_t* slots, size_t mask, hipStream_t s);
// launch_key_lookup over records: key_idx[i] = the index in the slot of item i's key record (32 * npoints bytes at
// pk + i * 32 * npoints, 16-byte aligned), else kSlotEmpty; k, misses as for launch_key_lookup.
hipError_t launch_key_lookup_wire(const uint8_t* pk, int npoints, size_t n, const uint8_t* records,
                                  const uint32_t* slots, size_t mask, size_t k, uint32_t* key_idx, uint32_t* misses,
                                  hipStream_t s);
// The key points of the listed items: for j < min(*count, n) and i = list[j] < n, point p of key record i
// (pk + i * 32 * npoints + 32 * p) is decompressed — k_decompress's bytes for every input — into row i of P0
// (p = 0) / P1 (p = 1), and valid[i] &= every point of the record decodes.  No other row of P0 / P1 / valid is
// touched.  Sized for n items: lanes past the list's end return at once.
void launch_decompress_listed(int npoints, const uint8_t* pk, size_t n, const uint32_t* list, const uint32_t* count,
                              uint8_t* P0, uint8_t* P1, uint8_t* valid, const uint32_t* ts_cancel,
                              const uint8_t* ts_hash, hipStream_t s);

}  // namespace dsv
