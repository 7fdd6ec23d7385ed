// keyed_census.h — the census of a batch's keys against a registered key set (include/dsv.h: dsv_keyset_census*;
// DESIGN.md §10.10): per registered key the number of items that hit it, and the distinct keys that missed, each
// with its number of items and the lowest item that carries it.  What a key cache needs to choose whom to admit
// (dsv_keyset_append*) and whom to evict (dsv_keyset_replace*), computed on the device next to the verify call.
// The lookup is keyed_lookup.h's walk over the set's own index, unchanged; the census adds two things to it:
//
//   hits        hits[found] += 1 per hit.  Not one global atomic per item: for k <= lds_keys a workgroup counts in an
//               LDS histogram of k words (zeroed at its start, flushed at its end with one global atomic per
//               non-zero bin); above, the lanes of a wave that found the same index are combined first (leader
//               loop: readlane, ballot, popcount) and the wave issues one global atomic per distinct index.
//   miss table  the call's own open-addressing table in the workspace: cap = keyset_index_cap(n) uint32 slots (never
//               more than half full: at most n distinct keys) and as many uint32 counts.  Home slot = home_hash of
//               the item's row & (cap - 1), the hash of the set's own index.  A slot holds the ITEM INDEX of a
//               representative of its key, or kSlotEmpty; an occupant's key is read from the call's own input
//               columns at that item's row, which nobody writes during the call.  Walk: atomicCAS(empty -> i); an
//               occupant with an equal key: atomicMin(slot, i), atomicAdd(count[slot], c), stop; else the next slot,
//               wrapping.  k_index_append's invariants hold word for word: a slot never returns to empty, and its
//               occupant only changes to an equal key with a lower item index — so all items of one key stop at one
//               slot, its count is exact and its representative ends as the key's lowest item index in the call.
//               No lane ever waits for another: a slot has no lock state and no walk spins.
//               In front of the walk the lanes of a wave that carry the same key are combined — matched on the
//               32-bit hash first, then compared word for word against the group's lowest lane, never on the hash
//               alone — and only that lane walks, with the group's popcount and (its own) lowest item index.
//
// One call is a straight chain of launches on one stream: totals cleared (launch_store_word), table cleared,
// census, report.
#pragma once
#include "keyed_lookup.h"

namespace dsv {

// Keys up to which a workgroup counts its hits in LDS: 4096 words = 16 KiB per workgroup of 256 lanes, so the
// eight workgroups that fill a CU's 32 wave slots hold 128 KiB of its 160 KiB of LDS — the largest power of two
// that costs no occupancy.  DSV_CENSUS_LDS_KEYS overrides it, up to kCensusLdsKeysMax (64 KiB,
// what a launch may ask for without opting in to more).
constexpr int kCensusLdsKeys = 4096;
constexpr int kCensusLdsKeysMax = 16384;

inline size_t census_table_bytes(size_t n) { return 2 * lookup_round256(4 * keyset_index_cap(n)); }

// The census of n items on `s` (n > 0).  form / key_a / key_b / npoints / rows / slots / mask / k: as for
// launch_index_lookup; k = 0 (no rows, no slots): every item misses and nothing is walked.  usable (may be null):
// one byte per item, 0 = the item has no key bytes (the typed form: a limb group >= q or z = 0) — it gets
// kSlotEmpty, counts in totals[1] and totals[2] and enters neither the table nor the report.  key_idx (may be null):
// what launch_index_lookup writes.  hits (may be null): u32[>= k], ADDED to.  miss_rep / miss_count: u32[n], entries
// [0, totals[0]) written in no particular order.  totals: u32[4] = distinct missed keys, missed items, unusable
// items, 0.  table: census_table_bytes(n) device bytes, 256-byte aligned.  lds_keys: the threshold as the process
// runs it.  Launch errors surface through hipGetLastError().
void launch_census(KeyForm form, const uint8_t* key_a, const uint8_t* key_b, const uint8_t* usable, int npoints,
                   size_t n, const uint8_t* rows, const uint32_t* slots, size_t mask, size_t k, int lds_keys,
                   uint32_t* key_idx, uint32_t* hits, uint32_t* miss_rep, uint32_t* miss_count, uint32_t* totals,
                   void* table, hipStream_t s);

}  // namespace dsv
