// keyset_host.h — what the host units know about a registered key set (keyed.h: the tables): the handle,
// the registry's lock and checks (dsv_keyset.hip), a keyed call's per-item inputs.
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

// one keyed call's per-item inputs: u, the signature's points R (and R' for the double scheme), m
struct KeyedIn {
  int scheme;
  const uint8_t *u, *R, *Rp, *m;
  bool any_null() const { return !u || !R || (scheme == 1 && !Rp) || !m; }
  Items items() const {  // (what launch_hash reads: R, R', m)
    Items in{scheme, u};
    in.pt[layout(scheme).R] = R;
    if (scheme == 1) in.pt[layout(scheme).Rp] = Rp;
    in.m = m;
    return in;
  }
};
inline KeyedIn keyed_in(int scheme, const void* u, const void* R, const void* Rp, const void* m) {
  return KeyedIn{scheme, (const uint8_t*)u, (const uint8_t*)R, (const uint8_t*)Rp, (const uint8_t*)m};
}

inline size_t keyed_ws_bytes(size_t n) { return align_up(n * 32, 256) + align_up(n, 256); }
// live key sets: verify calls read under the shared lock, create / destroy / shutdown write under the exclusive one
std::shared_mutex& keyset_mutex();
// (shared lock held) ks is live, of `scheme`, on an initialised device: ctx = its context
int check_set(const dsv_keyset* ks, int scheme, Context*& ctx);
// challenge hash, then the keyed kernel; every pointer device memory of ctx's device
void enqueue_keyed(const Context& ctx, const dsv_keyset* ks, const KeyedIn& in, const uint32_t* idx, size_t n,
                   uint8_t* ok, void* workspace, hipStream_t s);

}  // namespace dsvh
