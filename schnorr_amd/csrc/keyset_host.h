// keyset_host.h — what the host units know about a registered key set (keyed.h: the tables): the handle,
// the registry's lock and checks (dsv_keyset.hip), what a keyed call reads of its items.
#pragma once
#include <shared_mutex>

#include "dsv_host.h"
#include "keyed_wire.h"

struct dsv_keyset {
  int scheme = 0;
  size_t k = 0;
  int device = -1;
  size_t bytes = 0;
  uint32_t* tables = nullptr;  // one allocation: the tables, then key_ok
  uint8_t* key_ok = nullptr;
  bool alive = false;
};

namespace dsvh {

// A keyed call's items are make_items(scheme, u, {R[, R']}, m): the signature's points in their canonical slots,
// the key slots (PK, PK', Gen) null — the keys come from the set.
inline bool keyed_any_null(const Items& in) { return !in.u || !in.R() || (in.scheme == 1 && !in.Rp()) || !in.m; }

inline size_t keyed_ws_bytes(size_t n) { return align_up(n * 32, 256) + align_up(n, 256); }
// live key sets: verify calls read under the shared lock, create / destroy / shutdown write under the exclusive one
std::shared_mutex& keyset_mutex();
// (shared lock held) n is in range; ks is live, of `scheme`, on an initialised device: ctx = its context
int check_set(const dsv_keyset* ks, int scheme, size_t n, Context*& ctx);
// (shared lock held, check_set passed, n > 0) the rest of a keyed _dev call's checks, in this order: null
// pointers, the window bits (0 for the per-signature form), workspace_bytes >= need(n, ks->k, window_bits), `ok`
// on the set's device (ctx: the set's context)
// inputs_null: one of the call's input pointers other than idx is null (affine items: keyed_any_null; the wire
// form: the records or m)
int check_keyed_dev(const dsv_keyset* ks, const Context* ctx, bool inputs_null, const void* idx, size_t n,
                    const void* ok, const void* workspace, size_t workspace_bytes, int window_bits,
                    size_t (*need)(size_t n, size_t k, int window_bits));
inline int check_keyed_dev(const dsv_keyset* ks, const Context* ctx, const Items& in, const void* idx, size_t n,
                           const void* ok, const void* workspace, size_t workspace_bytes, int window_bits,
                           size_t (*need)(size_t n, size_t k, int window_bits)) {
  return check_keyed_dev(ks, ctx, keyed_any_null(in), idx, n, ok, workspace, workspace_bytes, window_bits, need);
}
// the calling thread's current device, which must be initialised: where a constructor builds its set
int current_context(Context*& out);
// tables of k keys from device points P0 / P1 (affine, 64 B each; P1 null for the single scheme) and an earlier
// stage's per-key verdicts valid_in (may be null), built on `s`; blocks, registers the set, *out = its handle
int create_from_device(Context& ctx, int scheme, const uint8_t* P0, const uint8_t* P1, const uint8_t* valid_in,
                       size_t k, hipStream_t s, dsv_keyset** out);
// challenge hash, then the keyed kernel; every pointer device memory of ctx's device
// valid_in (may be null): per-item bytes of an earlier stage (the wire form's decoder), AND-ed in by the hash
void enqueue_keyed(const Context& ctx, const dsv_keyset* ks, const Items& in, const uint32_t* idx, size_t n,
                   uint8_t* ok, void* workspace, hipStream_t s, const uint8_t* valid_in = nullptr);

// ---- the keyed wire form (dsv_keyed_wire.hip, keyed_wire.h) -----------------------------------------------
// the decoder's outputs for n records, in this order (dsv_keyed_wire_workspace_bytes): u, R, R' (double scheme
// only), valid; each part rounded up to 256 B
inline size_t keyed_wire_cols_bytes(int scheme, size_t n) {
  return align_up(n * 32, 256) + (size_t)keyed_wire_points(scheme) * align_up(n * 64, 256) + align_up(n, 256);
}
struct KeyedWireCols {
  uint8_t *u, *R, *Rp, *valid;
  Items items(int scheme, const void* m) const { return make_items(scheme, u, {R, Rp}, m); }
};
KeyedWireCols carve_keyed_wire(Stager& x, int scheme, size_t n);
// n signature records (device memory, 16-byte aligned) -> out.u, out.R() [, out.Rp()] and valid, one launch on
// `stream`; a step of its own so that it can stand in front of the keyed fast accept as well
void decode_keyed_wire(const Context& ctx, int scheme, const uint8_t* sig, size_t n, const Items& out, uint8_t* valid,
                       hipStream_t stream);

}  // namespace dsvh
