// dsv_keyed_open_wire.hip — the key cache for serialized records (include/dsv.h: dsv_verify_*_keyed_open_wire*;
// keyed_open_wire.h): the open-set form of verify for a caller that holds
// `Signature*::to_bytes()` and `PublicKey*::to_bytes()` records.  The verdicts are those of the unkeyed wire call on
// the same records for every input; an item whose key record is that of a valid registered key is decided by the
// key's tables and its key is never decompressed, every other item by the unkeyed equation on its own decompressed
// key.  Device form, one stream, enqueue-only: decode of the signatures, lookup of the key records in the set's
// record index, challenge hash and keyed kernel over all n (a miss gets 0 there), then the miss branch of
// dsv_keyed_open.hip, which owns the key columns here: the list of the misses, the decompression of the listed
// items' keys, the unkeyed equation over the list.  Host form: the same per chunk through the context's staging.
#include "keyset_host.h"

namespace dsvh {
namespace {

int check_sig_alignment(const void* sig) {
  if ((uintptr_t)sig & 15) return fail(DSV_ERR_INVALID_ARGUMENT, "signature records must be 16-byte aligned");
  return DSV_OK;
}

// idx | list | count | window tables | P0 [| P1] | u | R [| R'] | decode flags
size_t open_wire_cols_bytes(int scheme, size_t n) {
  return align_up(4 * n, 256) + open_miss_bytes(kKeyRecord, scheme, n) + keyed_wire_cols_bytes(scheme, n);
}

int open_wire_dev(int scheme, const dsv_keyset* ks, const void* sig, const void* pk, const void* m, size_t n,
                  void* ok, void* workspace, size_t workspace_bytes, void* stream, void* misses) {
  if (int r = library_up(ks)) return r;
  // the workspace in order: open_wire_cols_bytes | c | valid; run_keyed_dev checks and hands on the index pointer,
  // which is the workspace itself
  MissBranch b{};
  Items items;
  return run_keyed_dev(
      ks, scheme, [=](int) { return !sig || !pk || !m; }, [=](int) { return open_wire_cols_bytes(scheme, n); },
      workspace, n, ok, workspace, workspace_bytes, stream,
      [&](const Context& ctx, int, Stager& x, hipStream_t s, Items& in, const uint8_t*& valid_in) {
        if (int r = check_sig_alignment(sig)) return r;
        if (int r = check_key_alignment(kKeyRecord, scheme, pk, nullptr)) return r;
        if (int r = check_misses(ks, &ctx, misses)) return r;
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * n));
        b = carve_miss_branch(x, kKeyRecord, scheme, n, pk, nullptr);
        const KeyedCols w = carve_keyed_wire(x, scheme, n);
        items = in = w.items(scheme, m);
        valid_in = w.valid;
        decode_keyed_wire(ctx, scheme, static_cast<const uint8_t*>(sig), n, in, w.valid, s);
        HIP_TRY(hipGetLastError());
        return enqueue_lookup(ks, kKeyRecord, pk, nullptr, n, idx, static_cast<uint32_t*>(misses), s);
      },
      [&](const Context& ctx, hipStream_t s, const Workspace& w) {
        return enqueue_miss_branch(ctx, items, static_cast<const uint32_t*>(workspace), n, static_cast<uint8_t*>(ok),
                                   b, w, s);
      });
}

int open_wire_host(int scheme, const dsv_keyset* ks, const uint8_t* sig, const uint8_t* pk, const uint8_t* m,
                   size_t n, uint8_t* ok, size_t* misses) {
  return run_by_value_host(
      ks, scheme, any_scheme, [=](int) { return !sig || !pk || !m; },
      [=](int, size_t cnt) {
        return cnt * (layout(scheme).sig_bytes + layout(scheme).pk_bytes + 32 + 1) + 256 +
               open_wire_cols_bytes(scheme, cnt) + keyed_ws_bytes(cnt) + 6 * 256;
      },
      n, ok, 1, misses,
      [=](Context& ctx, int, Stager& st, size_t off, size_t cnt, uint32_t* dmiss, const void*& dout) {
        const size_t sig_bytes = layout(scheme).sig_bytes;
        uint8_t* dsig = st.take(cnt * sig_bytes);
        uint8_t* dm = st.take(cnt * 32);
        uint8_t* dok = st.take(cnt);
        uint8_t *dpk, *none;
        H2D(dsig, sig + off * sig_bytes, cnt * sig_bytes);
        H2D(dm, m + off * 32, cnt * 32);
        if (int r = stage_keys(kKeyRecord, scheme, st, pk, nullptr, off, cnt, dpk, none)) return r;
        uint32_t* di = reinterpret_cast<uint32_t*>(st.take(cnt * 4));
        const MissBranch b = carve_miss_branch(st, kKeyRecord, scheme, cnt, dpk, nullptr);
        const KeyedCols w = carve_keyed_wire(st, scheme, cnt);
        void* ws = st.take(keyed_ws_bytes(cnt));
        dout = dok;
        const Items in = w.items(scheme, dm);
        decode_keyed_wire(ctx, scheme, dsig, cnt, in, w.valid, 0);
        HIP_TRY(hipGetLastError());
        if (int r = enqueue_lookup(ks, kKeyRecord, dpk, nullptr, cnt, di, dmiss, 0)) return r;
        enqueue_keyed(ctx, ks, in, di, cnt, dok, ws, 0, w.valid);
        HIP_TRY(hipGetLastError());
        return enqueue_miss_branch(ctx, in, di, cnt, dok, b, carve(ws, cnt), 0);
      });
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyed_open_wire_workspace_bytes(int scheme, size_t n) {
  return scheme_ok(scheme) ? open_wire_cols_bytes(scheme, n) + keyed_ws_bytes(n) : 0;
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
