// keyset_host.h — what the host units know about a registered key set (keyed.h: the tables): the handle,
// the registry's lock and checks (dsv_keyset.hip), what a keyed call reads of its items.
#pragma once
#include <shared_mutex>

#include "dsv_host.h"
#include "keyed.h"

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
int check_keyed_dev(const dsv_keyset* ks, const Context* ctx, const Items& in, const void* idx, size_t n,
                    const void* ok, const void* workspace, size_t workspace_bytes, int window_bits,
                    size_t (*need)(size_t n, size_t k, int window_bits));
// challenge hash, then the keyed kernel; every pointer device memory of ctx's device
void enqueue_keyed(const Context& ctx, const dsv_keyset* ks, const Items& in, const uint32_t* idx, size_t n,
                   uint8_t* ok, void* workspace, hipStream_t s);

}  // namespace dsvh
