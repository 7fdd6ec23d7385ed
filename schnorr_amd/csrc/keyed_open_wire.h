// keyed_open_wire.h — the key cache for serialized records (dsv_verify_*_keyed_open_wire*, include/dsv.h;
// DESIGN.md §10.7): the decompression of the keys of the items that missed the set's record index
// (keyed_lookup.h: kKeyRecord).  A hit is found by byte operations alone; only a miss pays for a square root.
#pragma once
#include "keyed_lookup.h"

namespace dsv {

// ---- k_keyed_open_wire.hip ---------------------------------------------------------------------
// The key points of the listed items: for j < min(*count, n) and i = list[j] < n, point p of key record i
// (pk + i * 32 * npoints + 32 * p) is decompressed — k_decompress's bytes for every input — into row i of P0
// (p = 0) / P1 (p = 1), and valid[i] &= every point of the record decodes.  No other row of P0 / P1 / valid is
// touched.  Sized for n items: lanes past the list's end return at once.
void launch_decompress_listed(int npoints, const uint8_t* pk, size_t n, const uint32_t* list, const uint32_t* count,
                              uint8_t* P0, uint8_t* P1, uint8_t* valid, const uint32_t* ts_cancel,
                              const uint8_t* ts_hash, hipStream_t s);

}  // namespace dsv
