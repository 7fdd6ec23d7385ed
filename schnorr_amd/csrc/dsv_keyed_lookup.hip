// dsv_keyed_lookup.hip — registered key sets by key VALUE (include/dsv.h: dsv_keyset_lookup*,
// dsv_verify_keyed_lookup*; keyed_lookup.h): the key columns of a batch, canonical affine bytes, are looked up
// in the set's index and the batch is verified by the indices found — the closed-set form of verify: a key
// that is not in the set is a rejection.  Device form: lookup (k_key_lookup), challenge hash, keyed kernel —
// three launches on the caller's stream.  Host forms: the same per chunk through the context's staging.
#include "keyset_host.h"

namespace dsvh {

// a call without a handle before dsv_init: there is no handle to give yet, so it is told that nothing is up
// (a handle, live or dead, goes through check_set like every keyed call)
int library_up(const dsv_keyset* ks) {
  if (!ks && g_primary.load(std::memory_order_acquire) < 0)
    return fail(DSV_ERR_NOT_INITIALIZED, "dsv_init() has not been called");
  return DSV_OK;
}

bool keys_null(int scheme, const void* key_a, const void* key_b) {
  return !key_a || (keyset_points(scheme) == 2 && !key_b);
}
// the lookup kernel reads a key in 16-byte loads
int check_key_alignment(int scheme, const void* key_a, const void* key_b) {
  if (((uintptr_t)key_a & 15) || (keyset_points(scheme) == 2 && ((uintptr_t)key_b & 15)))
    return fail(DSV_ERR_INVALID_ARGUMENT, "key columns must be 16-byte aligned");
  return DSV_OK;
}
// a 4-byte-aligned word on the set's device (ctx: the set's context)
int check_misses(const dsv_keyset* ks, const Context* ctx, const void* misses) {
  if (!misses) return DSV_OK;
  if ((uintptr_t)misses & 3) return fail(DSV_ERR_INVALID_ARGUMENT, "misses must be 4-byte aligned");
  Context* mctx = nullptr;
  if (int r = device_context(misses, mctx)) return r;
  if (mctx != ctx)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key set of device %d used on device %d", ks->device, mctx->device);
  return DSV_OK;
}

// the lookup of n items on s; every pointer device memory of the set's device.  An empty set has no index:
// everything misses.
int enqueue_lookup(const dsv_keyset* ks, const void* key_a, const void* key_b, size_t n, uint32_t* idx,
                   uint32_t* misses, hipStream_t s) {
  if (ks->k == 0) {
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(idx), (int)kSlotEmpty, n, s));
    if (misses) launch_store_word(misses, (uint32_t)n, s);
    HIP_TRY(hipGetLastError());
    return DSV_OK;
  }
  HIP_TRY(launch_key_lookup(static_cast<const uint8_t*>(key_a), static_cast<const uint8_t*>(key_b),
                            keyset_points(ks->scheme), n, ks->index, ks->slots, ks->slot_mask, ks->k, idx, misses,
                            s));
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

namespace {

uint32_t home_hash_host(int np, const uint8_t* key_a, const uint8_t* key_b) {
  KeyHash h;
  for (int p = 0; p < np; p++) {
    const uint8_t* b = p ? key_b : key_a;
    for (int i = 0; i < 16; i++)
      h.word((uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
             (uint32_t)b[4 * i + 3] << 24);
  }
  return h.finish();
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyset_index_bytes(int scheme, size_t k) {
  return scheme_ok(scheme) ? keyset_index_total_bytes(scheme, k) : 0;
}
size_t dsv_keyed_lookup_workspace_bytes(size_t n) { return align_up(4 * n, 256) + keyed_ws_bytes(n); }

uint64_t dsv_debug_keyset_home_slot(int scheme, size_t k, const uint8_t* key_a, const uint8_t* key_b) {
  if (!scheme_ok(scheme) || k == 0 || keys_null(scheme, key_a, key_b)) return ~(uint64_t)0;
  return (uint64_t)home_hash_host(keyset_points(scheme), key_a, key_b) & ((uint64_t)keyset_index_cap(k) - 1);
}

int dsv_keyset_lookup_dev(const dsv_keyset* ks, const void* key_a, const void* key_b, size_t n, void* key_idx_out,
                          void* misses, void* stream) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (n == 0) return DSV_OK;
  if (keys_null(ks->scheme, key_a, key_b) || !key_idx_out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  if (int r = check_key_alignment(ks->scheme, key_a, key_b)) return r;
  if ((uintptr_t)key_idx_out & 3) return fail(DSV_ERR_INVALID_ARGUMENT, "key_idx_out must be 4-byte aligned");
  Context* octx = nullptr;
  if (int r = device_context(key_idx_out, octx)) return r;
  if (octx != cp)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key set of device %d used on device %d", ks->device, octx->device);
  if (int r = check_misses(ks, cp, misses)) return r;
  DSV_ON_DEVICE(*cp);
  return enqueue_lookup(ks, key_a, key_b, n, static_cast<uint32_t*>(key_idx_out), static_cast<uint32_t*>(misses),
                        (hipStream_t)stream);
}

int dsv_keyset_lookup(const dsv_keyset* ks, const uint8_t* key_a, const uint8_t* key_b, size_t n,
                      uint32_t* key_idx_out, size_t* misses) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (n == 0) {
    if (misses) *misses = 0;
    return DSV_OK;
  }
  if (keys_null(ks->scheme, key_a, key_b) || !key_idx_out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const int np = keyset_points(ks->scheme);
  const size_t chunk = n < kLookupHostChunk ? n : kLookupHostChunk;
  if (int r = ensure_stage(ctx, chunk * (64 * (size_t)np + 4) + 5 * 256)) return r;
  size_t total = 0;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t cnt = n - off < chunk ? n - off : chunk;
    Stager st(ctx.stage);
    uint8_t* da = st.take(cnt * 64);
    uint8_t* db = np == 2 ? st.take(cnt * 64) : nullptr;
    uint32_t* di = reinterpret_cast<uint32_t*>(st.take(cnt * 4));
    uint32_t* dmiss = reinterpret_cast<uint32_t*>(st.take(4));
    H2D(da, key_a + off * 64, cnt * 64);
    if (db) H2D(db, key_b + off * 64, cnt * 64);
    if (int r = enqueue_lookup(ks, da, db, cnt, di, dmiss, 0)) return r;
    uint32_t missed = 0;
    D2H(key_idx_out + off, di, cnt * 4);
    D2H(&missed, dmiss, 4);
    HIP_TRY(hipStreamSynchronize(0));
    total += missed;
  }
  if (misses) *misses = total;
  return DSV_OK;
}

int dsv_verify_keyed_lookup_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* Rp_uv,
                                const void* key_a, const void* key_b, const void* m, size_t n, void* ok,
                                void* workspace, size_t workspace_bytes, void* stream, void* misses) {
  if (int r = library_up(ks)) return r;
  // the index column is the first thing carved from the workspace: the index pointer run_keyed_dev checks and
  // hands to the keyed kernel is the workspace itself
  return run_keyed_dev(
      ks, -1,
      [=](int scheme) {
        return !u || !R_uv || (keyed_sig_points(scheme) == 2 && !Rp_uv) || !m || keys_null(scheme, key_a, key_b);
      },
      [=](int) { return align_up(4 * n, 256); }, workspace, n, ok, workspace, workspace_bytes, stream,
      [=](const Context& ctx, int scheme, Stager& x, hipStream_t s, Items& in, const uint8_t*&) {
        if (int r = check_key_alignment(scheme, key_a, key_b)) return r;
        if (int r = check_misses(ks, &ctx, misses)) return r;
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * n));
        if (int r = enqueue_lookup(ks, key_a, key_b, n, idx, static_cast<uint32_t*>(misses), s)) return r;
        in = make_items(scheme, u, {R_uv, keyed_sig_points(scheme) == 2 ? Rp_uv : nullptr}, m);
        return (int)DSV_OK;
      });
}

int dsv_verify_keyed_lookup(const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                            const uint8_t* key_a, const uint8_t* key_b, const uint8_t* m, size_t n, uint8_t* ok,
                            size_t* misses) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (n == 0) {
    if (misses) *misses = 0;
    return DSV_OK;
  }
  const int scheme = ks->scheme, ns = keyed_sig_points(scheme), np = keyset_points(scheme);
  if (!u || !R_uv || (ns == 2 && !Rp_uv) || !m || keys_null(scheme, key_a, key_b) || !ok)
    return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const size_t chunk = n < kLookupHostChunk ? n : kLookupHostChunk;
  const size_t per_item = 32 + 32 + 4 + 1 + 64 * (size_t)(ns + np);
  if (int r = ensure_stage(ctx, chunk * per_item + keyed_ws_bytes(chunk) + 12 * 256)) return r;
  size_t total = 0;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t cnt = n - off < chunk ? n - off : chunk;
    Stager st(ctx.stage);
    uint8_t* du = st.take(cnt * 32);
    uint8_t* dm = st.take(cnt * 32);
    uint32_t* di = reinterpret_cast<uint32_t*>(st.take(cnt * 4));
    uint8_t* dok = st.take(cnt);
    uint8_t* dR = st.take(cnt * 64);
    uint8_t* dRp = ns == 2 ? st.take(cnt * 64) : nullptr;
    uint8_t* da = st.take(cnt * 64);
    uint8_t* db = np == 2 ? st.take(cnt * 64) : nullptr;
    uint32_t* dmiss = reinterpret_cast<uint32_t*>(st.take(4));
    void* ws = st.take(keyed_ws_bytes(cnt));
    H2D(du, u + off * 32, cnt * 32);
    H2D(dm, m + off * 32, cnt * 32);
    H2D(dR, R_uv + off * 64, cnt * 64);
    if (dRp) H2D(dRp, Rp_uv + off * 64, cnt * 64);
    H2D(da, key_a + off * 64, cnt * 64);
    if (db) H2D(db, key_b + off * 64, cnt * 64);
    if (int r = enqueue_lookup(ks, da, db, cnt, di, dmiss, 0)) return r;
    enqueue_keyed(ctx, ks, make_items(scheme, du, {dR, dRp}, dm), di, cnt, dok, ws, 0);
    HIP_TRY(hipGetLastError());
    uint32_t missed = 0;
    D2H(ok + off, dok, cnt);
    D2H(&missed, dmiss, 4);
    HIP_TRY(hipStreamSynchronize(0));
    total += missed;
  }
  if (misses) *misses = total;
  return DSV_OK;
}

int dsv_debug_keyset_index_stats(const dsv_keyset* ks, uint64_t out[4]) {
  if (int r = library_up(ks)) return r;
  if (!ks || !out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, 0, cp)) return r;
  out[0] = out[1] = out[2] = out[3] = 0;
  const size_t k = ks->k;  // (an append may be filling rows and slots from k on: they are not this call's)
  if (k == 0) return DSV_OK;
  DSV_ON_DEVICE(*cp);
  const int np = keyset_points(ks->scheme);
  const size_t cap = ks->slot_mask + 1, key_bytes = 64 * (size_t)np;
  std::vector<uint8_t> keys(k * key_bytes);
  std::vector<uint32_t> slots(cap);
  HIP_TRY(hipMemcpy(keys.data(), ks->index, keys.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(slots.data(), ks->slots, cap * 4, hipMemcpyDeviceToHost));
  out[0] = cap;
  for (size_t slot = 0; slot < cap; slot++) {
    const uint32_t occ = slots[slot];
    if (occ == kSlotEmpty) continue;
    if (occ >= ks->capacity) return fail(DSV_ERR_HIP, "slot %zu holds %u of %zu keys", slot, occ, ks->capacity);
    if (occ >= k) continue;  // a key newer than this call: an empty slot, as the lookup reads it
    out[1]++;
    const uint8_t* kb = keys.data() + occ * key_bytes;
    const size_t home = home_hash_host(np, kb, kb + 64) & ks->slot_mask;
    const uint64_t probes = ((slot - home) & ks->slot_mask) + 1;  // slots read to find it
    if (slot != home) out[2]++;
    if (probes > out[3]) out[3] = probes;
  }
  return DSV_OK;
}

}  // extern "C"
