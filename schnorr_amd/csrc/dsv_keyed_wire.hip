// dsv_keyed_wire.hip — the keyed wire form (include/dsv.h: dsv_verify_*_keyed_wire*): serialized signatures
// verified against a registered key set.  Device form: decode (k_keyed_wire_decode), challenge hash, keyed
// kernel — three launches on the caller's stream.  Host form: the same per sub-batch of the shared host
// pipeline (dsv_pipeline.h), under the key-set registry's shared lock for the whole call.
#include "dsv_pipeline.h"
#include "keyset_host.h"

namespace dsvh {

KeyedCols carve_keyed_wire(Stager& x, int scheme, size_t n) {
  KeyedCols w = {};
  w.u = x.take(n * 32);
  w.R = x.take(n * 64);
  w.Rp = keyed_sig_points(scheme) == 2 ? x.take(n * 64) : nullptr;
  w.valid = x.take(n);
  return w;
}

void decode_keyed_wire(const Context& ctx, int scheme, const uint8_t* sig, size_t n, const Items& out, uint8_t* valid,
                       hipStream_t stream) {
  launch_keyed_wire_decode(scheme, sig, n, const_cast<uint8_t*>(out.u), const_cast<uint8_t*>(out.R()),
                           const_cast<uint8_t*>(out.Rp()), valid, ctx.ts_cancel, ctx.ts_hash, stream);
}

namespace {

size_t keyed_wire_ws_bytes(int scheme, size_t n) { return keyed_wire_cols_bytes(scheme, n) + keyed_ws_bytes(n); }

// decode -> hash -> keyed kernel for cnt records; every pointer device memory of ctx's device
void enqueue_keyed_wire(const Context& ctx, const dsv_keyset* ks, const uint8_t* sig, const uint32_t* idx,
                        const void* m, size_t cnt, uint8_t* ok, const KeyedCols& w, void* keyed_ws,
                        hipStream_t s) {
  const Items in = w.items(ks->scheme, m);
  decode_keyed_wire(ctx, ks->scheme, sig, cnt, in, w.valid, s);
  enqueue_keyed(ctx, ks, in, idx, cnt, ok, keyed_ws, s, w.valid);
}

int verify_keyed_wire_dev(const dsv_keyset* ks, int scheme, const void* sig, const void* idx, const void* m,
                          size_t n, void* ok, void* workspace, size_t workspace_bytes, void* stream) {
  return run_keyed_dev(
      ks, scheme, [=](int) { return !sig || !m; }, [=](int) { return keyed_wire_cols_bytes(scheme, n); }, idx, n, ok,
      workspace, workspace_bytes, stream,
      [=](const Context& ctx, int, Stager& x, hipStream_t s, Items& in, const uint8_t*& valid_in) {
        if ((uintptr_t)sig & 15) return fail(DSV_ERR_INVALID_ARGUMENT, "records must be 16-byte aligned");
        const KeyedCols w = carve_keyed_wire(x, scheme, n);
        in = w.items(scheme, m);
        valid_in = w.valid;
        decode_keyed_wire(ctx, scheme, (const uint8_t*)sig, n, in, w.valid, s);
        return (int)DSV_OK;
      });
}

// host arrays: the shared pipeline on the key set's device; per sub-batch the decoded columns come from the
// lane's scratch, the keyed workspace (c, valid) from the lane's verify workspace, which is never smaller
constexpr size_t kKeyedWireItemBytes = 32 + 2 * 64 + 1;
int verify_keyed_wire_host(const dsv_keyset* ks, int scheme, const uint8_t* sig, const uint32_t* idx,
                           const uint8_t* m, size_t n, uint8_t* ok) {
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, scheme, n, cp)) return r;
  if (n == 0) return DSV_OK;
  if (!sig || !idx || !m || !ok) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  const HostIn ins[3] = {{sig, layout(scheme).sig_bytes}, {reinterpret_cast<const uint8_t*>(idx), 4}, {m, 32}};
  return run_pipelined(*cp, ins, 3, ok, n, 0, kKeyedWireItemBytes, NoPrep{},
                       [=](const Staged& g, size_t off, size_t cnt, void* dok, void* ws, Stager& x, hipStream_t st) {
    enqueue_keyed_wire(*cp, ks, g.p[0] + off * g.bytes[0],
                       reinterpret_cast<const uint32_t*>(g.p[1] + off * g.bytes[1]), g.p[2] + off * g.bytes[2], cnt,
                       static_cast<uint8_t*>(dok), carve_keyed_wire(x, scheme, cnt), ws, st);
    HIP_TRY(hipGetLastError());
    return (int)DSV_OK;
  });
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyed_wire_workspace_bytes(int scheme, size_t n) {
  return scheme_ok(scheme) ? keyed_wire_ws_bytes(scheme, n) : 0;
}

int dsv_verify_single_keyed_wire_dev(const dsv_keyset* ks, const void* sig64, const void* key_idx, const void* m,
                                     size_t n, void* ok, void* workspace, size_t workspace_bytes, void* stream) {
  return verify_keyed_wire_dev(ks, 0, sig64, key_idx, m, n, ok, workspace, workspace_bytes, stream);
}
int dsv_verify_double_keyed_wire_dev(const dsv_keyset* ks, const void* sig96, const void* key_idx, const void* m,
                                     size_t n, void* ok, void* workspace, size_t workspace_bytes, void* stream) {
  return verify_keyed_wire_dev(ks, 1, sig96, key_idx, m, n, ok, workspace, workspace_bytes, stream);
}
int dsv_verify_vargen_keyed_wire_dev(const dsv_keyset* ks, const void* sig64, const void* key_idx, const void* m,
                                     size_t n, void* ok, void* workspace, size_t workspace_bytes, void* stream) {
  return verify_keyed_wire_dev(ks, 2, sig64, key_idx, m, n, ok, workspace, workspace_bytes, stream);
}

int dsv_verify_single_keyed_wire(const dsv_keyset* ks, const uint8_t* sig64, const uint32_t* key_idx,
                                 const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_keyed_wire_host(ks, 0, sig64, key_idx, m, n, ok);
}
int dsv_verify_double_keyed_wire(const dsv_keyset* ks, const uint8_t* sig96, const uint32_t* key_idx,
                                 const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_keyed_wire_host(ks, 1, sig96, key_idx, m, n, ok);
}
int dsv_verify_vargen_keyed_wire(const dsv_keyset* ks, const uint8_t* sig64, const uint32_t* key_idx,
                                 const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_keyed_wire_host(ks, 2, sig64, key_idx, m, n, ok);
}

}  // extern "C"
