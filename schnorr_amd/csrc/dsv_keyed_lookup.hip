// dsv_keyed_lookup.hip — registered key sets by key VALUE (include/dsv.h: dsv_keyset_lookup*,
// dsv_keyset_lookup_wire*, dsv_verify_keyed_lookup*; keyed_lookup.h): the keys of a batch — canonical affine
// bytes in columns, or compressed records — are looked up in the set's index of that form, and the batch is
// verified by the indices found — the closed-set form of verify: a key that is not in the set is a rejection.
// Device form: lookup (k_index_lookup), challenge hash, keyed kernel — three launches on the caller's stream.
// Host forms: the same per chunk through the context's staging (run_by_value_host).
#include "keyset_host.h"

namespace dsvh {

// a call without a handle before dsv_init: there is no handle to give yet, so it is told that nothing is up
// (a handle, live or dead, goes through check_set like every keyed call)
int library_up(const dsv_keyset* ks) {
  if (!ks && g_primary.load(std::memory_order_acquire) < 0)
    return fail(DSV_ERR_NOT_INITIALIZED, "dsv_init() has not been called");
  return DSV_OK;
}

// columns a batch's keys come in: one per key point (affine), or one of whole records
static int key_columns(KeyForm form, int scheme) { return form == kKeyAffine ? keyset_points(scheme) : 1; }

bool keys_null(KeyForm form, int scheme, const void* key_a, const void* key_b) {
  return !key_a || (key_columns(form, scheme) == 2 && !key_b);
}
int check_key_alignment(KeyForm form, int scheme, const void* key_a, const void* key_b) {
  if (((uintptr_t)key_a & 15) || (key_columns(form, scheme) == 2 && ((uintptr_t)key_b & 15)))
    return fail(DSV_ERR_INVALID_ARGUMENT, "%s must be 16-byte aligned",
                form == kKeyAffine ? "key columns" : "key records");
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

int enqueue_lookup(const dsv_keyset* ks, KeyForm form, const void* key_a, const void* key_b, size_t n, uint32_t* idx,
                   uint32_t* misses, hipStream_t s) {
  if (ks->k == 0) {
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(idx), (int)kSlotEmpty, n, s));
    if (misses) launch_store_word(misses, (uint32_t)n, s);
    HIP_TRY(hipGetLastError());
    return DSV_OK;
  }
  HIP_TRY(launch_index_lookup(form, static_cast<const uint8_t*>(key_a), static_cast<const uint8_t*>(key_b),
                              keyset_points(ks->scheme), n, ks->index[form].rows, ks->index[form].slots,
                              ks->slot_mask, ks->k, idx, misses, s));
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

int stage_keys(KeyForm form, int scheme, Stager& st, const uint8_t* key_a, const uint8_t* key_b, size_t off,
               size_t cnt, uint8_t*& da, uint8_t*& db) {
  const size_t item = keys_item_bytes(form, scheme) / (size_t)key_columns(form, scheme);
  da = st.take(cnt * item);
  db = key_columns(form, scheme) == 2 ? st.take(cnt * item) : nullptr;
  H2D(da, key_a + off * item, cnt * item);
  if (db) H2D(db, key_b + off * item, cnt * item);
  return DSV_OK;
}

int stage_affine_chunk(int scheme, Stager& st, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                       const uint8_t* m, const uint8_t* key_a, const uint8_t* key_b, size_t off, size_t cnt,
                       AffineChunk& c) {
  const int ns = keyed_sig_points(scheme);
  uint8_t* du = st.take(cnt * 32);
  uint8_t* dm = st.take(cnt * 32);
  c.idx = reinterpret_cast<uint32_t*>(st.take(cnt * 4));
  c.ok = st.take(cnt);
  uint8_t* dR = st.take(cnt * 64);
  uint8_t* dRp = ns == 2 ? st.take(cnt * 64) : nullptr;
  H2D(du, u + off * 32, cnt * 32);
  H2D(dm, m + off * 32, cnt * 32);
  H2D(dR, R_uv + off * 64, cnt * 64);
  if (dRp) H2D(dRp, Rp_uv + off * 64, cnt * 64);
  c.in = make_items(scheme, du, {dR, dRp}, dm);
  return stage_keys(kKeyAffine, scheme, st, key_a, key_b, off, cnt, c.key_a, c.key_b);
}

namespace {

// the hash of a key's little-endian words: `words` at a, then as many at b (null: none)
uint32_t key_hash_host(const uint8_t* a, const uint8_t* b, int words) {
  KeyHash h;
  for (const uint8_t* p : {a, b})
    for (int i = 0; p && i < words; i++)
      h.word((uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 |
             (uint32_t)p[4 * i + 3] << 24);
  return h.finish();
}

int lookup_dev(KeyForm form, const dsv_keyset* ks, const void* key_a, const void* key_b, size_t n, void* key_idx_out,
               void* misses, void* stream) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (n == 0) return DSV_OK;
  if (keys_null(form, ks->scheme, key_a, key_b) || !key_idx_out)
    return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  if (int r = check_key_alignment(form, ks->scheme, key_a, key_b)) return r;
  if ((uintptr_t)key_idx_out & 3) return fail(DSV_ERR_INVALID_ARGUMENT, "key_idx_out must be 4-byte aligned");
  Context* octx = nullptr;
  if (int r = device_context(key_idx_out, octx)) return r;
  if (octx != cp)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key set of device %d used on device %d", ks->device, octx->device);
  if (int r = check_misses(ks, cp, misses)) return r;
  DSV_ON_DEVICE(*cp);
  return enqueue_lookup(ks, form, key_a, key_b, n, static_cast<uint32_t*>(key_idx_out),
                        static_cast<uint32_t*>(misses), (hipStream_t)stream);
}

int lookup_host(KeyForm form, const dsv_keyset* ks, const uint8_t* key_a, const uint8_t* key_b, size_t n,
                uint32_t* key_idx_out, size_t* misses) {
  return run_by_value_host(
      ks, -1, any_scheme, [=](int scheme) { return keys_null(form, scheme, key_a, key_b); },
      [=](int scheme, size_t cnt) { return cnt * (keys_item_bytes(form, scheme) + 4) + 5 * 256; }, n, key_idx_out, 4,
      misses, [=](Context&, int scheme, Stager& st, size_t off, size_t cnt, uint32_t* dmiss, const void*& dout) {
        uint8_t *da, *db;
        if (int r = stage_keys(form, scheme, st, key_a, key_b, off, cnt, da, db)) return r;
        uint32_t* di = reinterpret_cast<uint32_t*>(st.take(cnt * 4));
        dout = di;
        return enqueue_lookup(ks, form, da, db, cnt, di, dmiss, 0);
      });
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyset_index_bytes(int scheme, size_t k) {
  return scheme_ok(scheme) ? keyset_index_total_bytes(kKeyAffine, scheme, k) : 0;
}
size_t dsv_keyset_wire_index_bytes(int scheme, size_t k) {
  return scheme_ok(scheme) ? keyset_index_total_bytes(kKeyRecord, scheme, k) : 0;
}
size_t dsv_keyed_lookup_workspace_bytes(size_t n) { return align_up(4 * n, 256) + keyed_ws_bytes(n); }

uint64_t dsv_debug_keyset_home_slot(int scheme, size_t k, const uint8_t* key_a, const uint8_t* key_b) {
  if (!scheme_ok(scheme) || k == 0 || keys_null(kKeyAffine, scheme, key_a, key_b)) return ~(uint64_t)0;
  return (uint64_t)key_hash_host(key_a, keyset_points(scheme) == 2 ? key_b : nullptr, 16) &
         ((uint64_t)keyset_index_cap(k) - 1);
}
int dsv_debug_keyset_wire_home_slot(int scheme, size_t capacity, const uint8_t* record, uint64_t* slot) {
  if (!scheme_ok(scheme)) return fail(DSV_ERR_INVALID_ARGUMENT, "unknown scheme %d", scheme);
  if (capacity == 0) return fail(DSV_ERR_INVALID_ARGUMENT, "a set of no capacity has no index");
  if (!record || !slot) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  *slot = (uint64_t)key_hash_host(record, nullptr, 8 * keyset_points(scheme)) &
          ((uint64_t)keyset_index_cap(capacity) - 1);
  return DSV_OK;
}

int dsv_keyset_lookup_dev(const dsv_keyset* ks, const void* key_a, const void* key_b, size_t n, void* key_idx_out,
                          void* misses, void* stream) {
  return lookup_dev(kKeyAffine, ks, key_a, key_b, n, key_idx_out, misses, stream);
}
int dsv_keyset_lookup_wire_dev(const dsv_keyset* ks, const void* pk_records, size_t n, void* key_idx_out,
                               void* misses, void* stream) {
  return lookup_dev(kKeyRecord, ks, pk_records, nullptr, n, key_idx_out, misses, stream);
}
int dsv_keyset_lookup(const dsv_keyset* ks, const uint8_t* key_a, const uint8_t* key_b, size_t n,
                      uint32_t* key_idx_out, size_t* misses) {
  return lookup_host(kKeyAffine, ks, key_a, key_b, n, key_idx_out, misses);
}
int dsv_keyset_lookup_wire(const dsv_keyset* ks, const uint8_t* pk_records, size_t n, uint32_t* key_idx_out,
                           size_t* misses) {
  return lookup_host(kKeyRecord, ks, pk_records, nullptr, n, key_idx_out, misses);
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
        return !u || !R_uv || (keyed_sig_points(scheme) == 2 && !Rp_uv) || !m ||
               keys_null(kKeyAffine, scheme, key_a, key_b);
      },
      [=](int) { return align_up(4 * n, 256); }, workspace, n, ok, workspace, workspace_bytes, stream,
      [=](const Context& ctx, int scheme, Stager& x, hipStream_t s, Items& in, const uint8_t*&) {
        if (int r = check_key_alignment(kKeyAffine, scheme, key_a, key_b)) return r;
        if (int r = check_misses(ks, &ctx, misses)) return r;
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * n));
        if (int r = enqueue_lookup(ks, kKeyAffine, key_a, key_b, n, idx, static_cast<uint32_t*>(misses), s)) return r;
        in = make_items(scheme, u, {R_uv, keyed_sig_points(scheme) == 2 ? Rp_uv : nullptr}, m);
        return (int)DSV_OK;
      });
}

int dsv_verify_keyed_lookup(const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                            const uint8_t* key_a, const uint8_t* key_b, const uint8_t* m, size_t n, uint8_t* ok,
                            size_t* misses) {
  return run_by_value_host(
      ks, -1, any_scheme,
      [=](int scheme) { return affine_inputs_null(scheme, u, R_uv, Rp_uv, m, key_a, key_b); },
      [=](int scheme, size_t cnt) { return affine_chunk_bytes(scheme, cnt) + keyed_ws_bytes(cnt); }, n, ok, 1, misses,
      [=](Context& ctx, int scheme, Stager& st, size_t off, size_t cnt, uint32_t* dmiss, const void*& dout) {
        AffineChunk c;
        if (int r = stage_affine_chunk(scheme, st, u, R_uv, Rp_uv, m, key_a, key_b, off, cnt, c)) return r;
        void* ws = st.take(keyed_ws_bytes(cnt));
        dout = c.ok;
        if (int r = enqueue_lookup(ks, kKeyAffine, c.key_a, c.key_b, cnt, c.idx, dmiss, 0)) return r;
        enqueue_keyed(ctx, ks, c.in, c.idx, cnt, c.ok, ws, 0);
        HIP_TRY(hipGetLastError());
        return (int)DSV_OK;
      });
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
  HIP_TRY(hipMemcpy(keys.data(), ks->index[kKeyAffine].rows, keys.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(slots.data(), ks->index[kKeyAffine].slots, cap * 4, hipMemcpyDeviceToHost));
  out[0] = cap;
  for (size_t slot = 0; slot < cap; slot++) {
    const uint32_t occ = slots[slot];
    if (occ == kSlotEmpty) continue;
    if (occ >= ks->capacity) return fail(DSV_ERR_HIP, "slot %zu holds %u of %zu keys", slot, occ, ks->capacity);
    if (occ >= k) continue;  // a key newer than this call: an empty slot, as the lookup reads it
    out[1]++;
    const uint8_t* kb = keys.data() + occ * key_bytes;
    const size_t home = key_hash_host(kb, np == 2 ? kb + 64 : nullptr, 16) & ks->slot_mask;
    const uint64_t probes = ((slot - home) & ks->slot_mask) + 1;  // slots read to find it
    if (slot != home) out[2]++;
    if (probes > out[3]) out[3] = probes;
  }
  return DSV_OK;
}

}  // extern "C"
