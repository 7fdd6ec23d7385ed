// keyed_open_mont.h — the key cache for typed objects (dsv_verify_keyed_open_mont_*, include/dsv.h; DESIGN.md
// §10.9): the open-set form of verify over exactly the arguments of the reference's `verify_batch` — Montgomery
// limbs, projective points.  One front kernel normalises the nonce points AND the key points of a batch, converts
// the two scalars and looks the normalised key up in the set's affine index (keyed_lookup.h: kKeyAffine), all in
// the one preprocessing launch the typed forms have; behind it the chain of the open-set form runs unchanged
// (keyed_open.h): challenge hash, keyed kernel, miss list, the unkeyed equation over the list.
#pragma once
#include "keyed_lookup.h"

namespace dsv {

// ---- k_keyed_open_mont.hip ---------------------------------------------------------------------
// a: in[0 .. nps) the nonce points R [, R'], in[nps .. nps + npk) the key points PK [, PK' | Gen] (u || v || z
// limbs, 96 B per item, 16-byte aligned); out[0 .. nps) the nonce points' affine columns, out[nps ..) the miss
// branch's own key columns (64 B per item), of which only the rows of misses are written; u_mont / m_mont ->
// u_out / m_out as launch_normalize_uvz converts them (all four set).  valid, prefix, want_per_lane, block: those
// of launch_normalize_uvz over nps + npk points — same lanes, same prefix layout, same grid.
// key_idx[i] = the index of item i's normalised key in the affine index (rows / slots / mask; k: the set's key
// count as the call sees it — an occupant >= k is an empty slot; k = 0: nothing is read, everything misses), else
// kSlotEmpty; an item whose key limbs are not usable (a coordinate >= q, z = 0) gets kSlotEmpty and valid[i] = 0.
// misses (may be null): the number of items that got kSlotEmpty is ADDED to it, one atomic per wave — the caller
// resets it (launch_store_word) where a call starts.
void launch_normalize_lookup(const NormalizeArgs& a, int nps, int npk, size_t n, uint8_t* valid, uint32_t* prefix,
                             const uint8_t* rows, const uint32_t* slots, size_t mask, size_t k, uint32_t* key_idx,
                             uint32_t* misses, hipStream_t s, int want_per_lane = 0, int block = 0);

// The two-launch front's gate (DSV_OPEN_MONT_FUSED=0), behind launch_index_lookup over the normalised key columns:
// an item whose key limbs (key_a [, key_b]: 96 B of u || v || z per item, as above) are not usable and whose
// key_idx[i] is not kSlotEmpty — the bytes normalised from unusable limbs happened to be a registered key's — gets
// kSlotEmpty, and *count (may be null; the lookup's own count) grows by one: the front kernel never looks such a
// key up.  One lane per item.
void launch_unusable_keys_miss(const uint8_t* key_a, const uint8_t* key_b, int npk, size_t n, uint32_t* key_idx,
                               uint32_t* count, hipStream_t s);

}  // namespace dsv
