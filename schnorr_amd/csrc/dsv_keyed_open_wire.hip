// dsv_keyed_open_wire.hip — the key cache for serialized records (include/dsv.h: dsv_keyset_lookup_wire*,
// dsv_verify_*_keyed_open_wire*; keyed_open_wire.h): the open-set form of verify for a caller that
// holds `Signature*::to_bytes()` and `PublicKey*::to_bytes()` records.  The verdicts are those of the unkeyed wire
// call on the same records for every input; an item whose key record is that of a valid registered key is decided
// by the key's tables and its key is never decompressed, every other item by the unkeyed equation on its own
// decompressed key.  Device form, one stream, enqueue-only: decode of the signatures, lookup of the key records in
// the set's wire index, challenge hash and keyed kernel over all n (a miss gets 0 there), the list of the misses,
// the decompression of the listed items' keys, the unkeyed equation over the list.  Host form: the same per chunk
// through the context's staging.
#include "keyset_host.h"

namespace dsvh {

// An empty set has no index: everything misses.
int enqueue_lookup_wire(const dsv_keyset* ks, const void* pk, size_t n, uint32_t* idx, uint32_t* misses,
                        hipStream_t s) {
  if (ks->k == 0) {
    HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(idx), (int)kSlotEmpty, n, s));
    if (misses) launch_store_word(misses, (uint32_t)n, s);
    HIP_TRY(hipGetLastError());
    return DSV_OK;
  }
  HIP_TRY(launch_key_lookup_wire(static_cast<const uint8_t*>(pk), keyset_points(ks->scheme), n, ks->wire_index,
                                 ks->wire_slots, ks->slot_mask, ks->k, idx, misses, s));
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

namespace {

int check_record_alignment(const void* p, const char* what) {
  if ((uintptr_t)p & 15) return fail(DSV_ERR_INVALID_ARGUMENT, "%s must be 16-byte aligned", what);
  return DSV_OK;
}

// the miss branch's part of the workspace, as the open-set form by affine bytes lays it out (dsv_keyed_open.hip):
// list | count | per-lane window tables — and behind it the key columns only the listed rows of which are written
size_t open_miss_bytes(size_t n) { return align_up(4 * n, 256) + 256 + var_table_bytes(n, kTablesPerLane); }
size_t key_cols_bytes(int scheme, size_t n) { return (size_t)keyset_points(scheme) * align_up(n * 64, 256); }
struct MissBranch {
  uint32_t *list, *count, *tables;
  uint8_t *P0, *P1;
};
MissBranch carve_miss_branch(Stager& x, int scheme, size_t n) {
  MissBranch b;
  b.list = reinterpret_cast<uint32_t*>(x.take(4 * n));
  b.count = reinterpret_cast<uint32_t*>(x.take(4));
  b.tables = reinterpret_cast<uint32_t*>(x.take(var_table_bytes(n, kTablesPerLane)));
  b.P0 = x.take(n * 64);
  b.P1 = keyset_points(scheme) == 2 ? x.take(n * 64) : nullptr;
  return b;
}
// behind the keyed kernel on s: the misses of idx are listed, their key records (pk) decompressed into the listed
// rows of b.P0 / b.P1 with the decode flags AND-ed into w.valid, and decided by the unkeyed equation from the c /
// valid the challenge hash left in w; in: the keyed call's items
int enqueue_miss_branch(const Context& ctx, const Items& in, const uint8_t* pk, const uint32_t* idx, size_t n,
                        uint8_t* ok, const MissBranch& b, const Workspace& w, hipStream_t s) {
  HIP_TRY(launch_miss_list(idx, n, b.list, b.count, s));
  launch_decompress_listed(keyset_points(in.scheme), pk, n, b.list, b.count, b.P0, b.P1, w.valid, ctx.ts_cancel,
                           ctx.ts_hash, s);
  HIP_TRY(hipGetLastError());
  if (in.scheme == 2) {
    launch_verify_var_listed(in.u, w.c, b.P0, b.P1, in.R(), w.valid, n, ok, b.tables, b.list, b.count, s);
    HIP_TRY(hipGetLastError());
    return DSV_OK;
  }
  const ChainOperands op0{b.P0, in.R(), ctx.table[0]};
  const ChainOperands op1{b.P1, in.Rp(), ctx.table[1]};
  launch_verify_listed(in.scheme == 1 ? 2 : 1, in.u, w.c, op0, op1, w.valid, n, ok, b.tables, b.list, b.count, s);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

size_t open_wire_cols_bytes(int scheme, size_t n) {
  return align_up(4 * n, 256) + open_miss_bytes(n) + key_cols_bytes(scheme, n) + keyed_wire_cols_bytes(scheme, n);
}

int open_wire_dev(int scheme, const dsv_keyset* ks, const void* sig, const void* pk, const void* m, size_t n,
                  void* ok, void* workspace, size_t workspace_bytes, void* stream, void* misses) {
  if (int r = library_up(ks)) return r;
  // the workspace in order: idx | list | count | window tables | P0 [| P1] | u | R [| R'] | decode flags | c |
  // valid; run_keyed_dev checks and hands on the index pointer, which is the workspace itself
  MissBranch b{};
  Items items;
  return run_keyed_dev(
      ks, scheme, [=](int) { return !sig || !pk || !m; }, [=](int) { return open_wire_cols_bytes(scheme, n); },
      workspace, n, ok, workspace, workspace_bytes, stream,
      [&](const Context& ctx, int, Stager& x, hipStream_t s, Items& in, const uint8_t*& valid_in) {
        if (int r = check_record_alignment(sig, "signature records")) return r;
        if (int r = check_record_alignment(pk, "key records")) return r;
        if (int r = check_misses(ks, &ctx, misses)) return r;
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * n));
        b = carve_miss_branch(x, scheme, n);
        const KeyedCols w = carve_keyed_wire(x, scheme, n);
        items = in = w.items(scheme, m);
        valid_in = w.valid;
        decode_keyed_wire(ctx, scheme, static_cast<const uint8_t*>(sig), n, in, w.valid, s);
        HIP_TRY(hipGetLastError());
        return enqueue_lookup_wire(ks, pk, n, idx, static_cast<uint32_t*>(misses), s);
      },
      [&](const Context& ctx, hipStream_t s, const Workspace& w) {
        return enqueue_miss_branch(ctx, items, static_cast<const uint8_t*>(pk),
                                   static_cast<const uint32_t*>(workspace), n, static_cast<uint8_t*>(ok), b, w, s);
      });
}

int open_wire_host(int scheme, const dsv_keyset* ks, const uint8_t* sig, const uint8_t* pk, const uint8_t* m,
                   size_t n, uint8_t* ok, size_t* misses) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, scheme, n, cp)) return r;
  if (n == 0) {
    if (misses) *misses = 0;
    return DSV_OK;
  }
  if (!sig || !pk || !m || !ok) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const size_t sig_bytes = layout(scheme).sig_bytes, pk_bytes = layout(scheme).pk_bytes;
  const size_t chunk = n < kLookupHostChunk ? n : kLookupHostChunk;
  if (int r = ensure_stage(ctx, chunk * (sig_bytes + pk_bytes + 32 + 1) + 256 + open_wire_cols_bytes(scheme, chunk) +
                                    keyed_ws_bytes(chunk) + 6 * 256))
    return r;
  size_t total = 0;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t cnt = n - off < chunk ? n - off : chunk;
    Stager st(ctx.stage);
    uint8_t* dsig = st.take(cnt * sig_bytes);
    uint8_t* dpk = st.take(cnt * pk_bytes);
    uint8_t* dm = st.take(cnt * 32);
    uint8_t* dok = st.take(cnt);
    uint32_t* dmiss = reinterpret_cast<uint32_t*>(st.take(4));
    uint32_t* di = reinterpret_cast<uint32_t*>(st.take(cnt * 4));
    const MissBranch b = carve_miss_branch(st, scheme, cnt);
    const KeyedCols w = carve_keyed_wire(st, scheme, cnt);
    void* ws = st.take(keyed_ws_bytes(cnt));
    H2D(dsig, sig + off * sig_bytes, cnt * sig_bytes);
    H2D(dpk, pk + off * pk_bytes, cnt * pk_bytes);
    H2D(dm, m + off * 32, cnt * 32);
    const Items in = w.items(scheme, dm);
    decode_keyed_wire(ctx, scheme, dsig, cnt, in, w.valid, 0);
    HIP_TRY(hipGetLastError());
    if (int r = enqueue_lookup_wire(ks, dpk, cnt, di, dmiss, 0)) return r;
    enqueue_keyed(ctx, ks, in, di, cnt, dok, ws, 0, w.valid);
    HIP_TRY(hipGetLastError());
    if (int r = enqueue_miss_branch(ctx, in, dpk, di, cnt, dok, b, carve(ws, cnt), 0)) return r;
    uint32_t missed = 0;
    D2H(ok + off, dok, cnt);
    D2H(&missed, dmiss, 4);
    HIP_TRY(hipStreamSynchronize(0));
    total += missed;
  }
  if (misses) *misses = total;
  return DSV_OK;
}

uint32_t record_hash_host(int np, const uint8_t* b) {
  KeyHash h;
  for (int i = 0; i < 8 * np; i++)
    h.word((uint32_t)b[4 * i] | (uint32_t)b[4 * i + 1] << 8 | (uint32_t)b[4 * i + 2] << 16 |
           (uint32_t)b[4 * i + 3] << 24);
  return h.finish();
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyset_wire_index_bytes(int scheme, size_t k) {
  return scheme_ok(scheme) ? keyset_wire_index_total_bytes(scheme, k) : 0;
}
size_t dsv_keyed_open_wire_workspace_bytes(int scheme, size_t n) {
  return scheme_ok(scheme) ? open_wire_cols_bytes(scheme, n) + keyed_ws_bytes(n) : 0;
}

int dsv_debug_keyset_wire_home_slot(int scheme, size_t capacity, const uint8_t* record, uint64_t* slot) {
  if (!scheme_ok(scheme)) return fail(DSV_ERR_INVALID_ARGUMENT, "unknown scheme %d", scheme);
  if (capacity == 0) return fail(DSV_ERR_INVALID_ARGUMENT, "a set of no capacity has no index");
  if (!record || !slot) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  *slot = (uint64_t)record_hash_host(keyset_points(scheme), record) & ((uint64_t)keyset_index_cap(capacity) - 1);
  return DSV_OK;
}

int dsv_keyset_lookup_wire_dev(const dsv_keyset* ks, const void* pk_records, size_t n, void* key_idx_out,
                               void* misses, void* stream) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (n == 0) return DSV_OK;
  if (!pk_records || !key_idx_out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  if (int r = check_record_alignment(pk_records, "key records")) return r;
  if ((uintptr_t)key_idx_out & 3) return fail(DSV_ERR_INVALID_ARGUMENT, "key_idx_out must be 4-byte aligned");
  Context* octx = nullptr;
  if (int r = device_context(key_idx_out, octx)) return r;
  if (octx != cp)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key set of device %d used on device %d", ks->device, octx->device);
  if (int r = check_misses(ks, cp, misses)) return r;
  DSV_ON_DEVICE(*cp);
  return enqueue_lookup_wire(ks, pk_records, n, static_cast<uint32_t*>(key_idx_out), static_cast<uint32_t*>(misses),
                             (hipStream_t)stream);
}

int dsv_keyset_lookup_wire(const dsv_keyset* ks, const uint8_t* pk_records, size_t n, uint32_t* key_idx_out,
                           size_t* misses) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (n == 0) {
    if (misses) *misses = 0;
    return DSV_OK;
  }
  if (!pk_records || !key_idx_out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const size_t rec = layout(ks->scheme).pk_bytes;
  const size_t chunk = n < kLookupHostChunk ? n : kLookupHostChunk;
  if (int r = ensure_stage(ctx, chunk * (rec + 4) + 4 * 256)) return r;
  size_t total = 0;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t cnt = n - off < chunk ? n - off : chunk;
    Stager st(ctx.stage);
    uint8_t* dpk = st.take(cnt * rec);
    uint32_t* di = reinterpret_cast<uint32_t*>(st.take(cnt * 4));
    uint32_t* dmiss = reinterpret_cast<uint32_t*>(st.take(4));
    H2D(dpk, pk_records + off * rec, cnt * rec);
    if (int r = enqueue_lookup_wire(ks, dpk, cnt, di, dmiss, 0)) return r;
    uint32_t missed = 0;
    D2H(key_idx_out + off, di, cnt * 4);
    D2H(&missed, dmiss, 4);
    HIP_TRY(hipStreamSynchronize(0));
    total += missed;
  }
  if (misses) *misses = total;
  return DSV_OK;
}

int dsv_verify_single_keyed_open_wire_dev(const dsv_keyset* ks, const void* sig64, const void* pk32, const void* m,
                                          size_t n, void* ok, void* workspace, size_t workspace_bytes, void* stream,
                                          void* misses) {
  return open_wire_dev(0, ks, sig64, pk32, m, n, ok, workspace, workspace_bytes, stream, misses);
}
int dsv_verify_double_keyed_open_wire_dev(const dsv_keyset* ks, const void* sig96, const void* pk64, const void* m,
                                          size_t n, void* ok, void* workspace, size_t workspace_bytes, void* stream,
                                          void* misses) {
  return open_wire_dev(1, ks, sig96, pk64, m, n, ok, workspace, workspace_bytes, stream, misses);
}
int dsv_verify_vargen_keyed_open_wire_dev(const dsv_keyset* ks, const void* sig64, const void* pk64, const void* m,
                                          size_t n, void* ok, void* workspace, size_t workspace_bytes, void* stream,
                                          void* misses) {
  return open_wire_dev(2, ks, sig64, pk64, m, n, ok, workspace, workspace_bytes, stream, misses);
}

int dsv_verify_single_keyed_open_wire(const dsv_keyset* ks, const uint8_t* sig64, const uint8_t* pk32,
                                      const uint8_t* m, size_t n, uint8_t* ok, size_t* misses) {
  return open_wire_host(0, ks, sig64, pk32, m, n, ok, misses);
}
int dsv_verify_double_keyed_open_wire(const dsv_keyset* ks, const uint8_t* sig96, const uint8_t* pk64,
                                      const uint8_t* m, size_t n, uint8_t* ok, size_t* misses) {
  return open_wire_host(1, ks, sig96, pk64, m, n, ok, misses);
}
int dsv_verify_vargen_keyed_open_wire(const dsv_keyset* ks, const uint8_t* sig64, const uint8_t* pk64,
                                      const uint8_t* m, size_t n, uint8_t* ok, size_t* misses) {
  return open_wire_host(2, ks, sig64, pk64, m, n, ok, misses);
}

}  // extern "C"
