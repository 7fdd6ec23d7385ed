// dsv_wire.hip — serialized records (`Signature::from_bytes`, `PublicKey::from_bytes`:
// /root/reference/src/signatures.rs:117-122, :261-269, :398-403; src/keys/public.rs:94-100, :294-298,
// :361-371): point decompression on the device (k_decompress), then the per-signature kernels.
#include "dsv_pipeline.h"

using namespace dsvh;

extern "C" {

// ---- wire formats ---------------------------------------------------------------------------
int dsv_decompress_points_dev(const void* in, size_t in_stride, size_t n, void* out_uv, void* ok,
                              int accumulate, void* stream) {
  DSV_DEV_PROLOGUE(n, out_uv);
  return decompress_on(ctx, in, in_stride, n, out_uv, ok, accumulate, (hipStream_t)stream);
}
// JubJubAffine::to_bytes: canonical v with bit 255 = lowest bit of canonical u.  Pure byte
// shuffling on affine input, so it runs on the host.
int dsv_compress_points(const uint8_t* in_uv, size_t n, uint8_t* out32) {
  if (int r = check_n(n)) return r;
  if (n == 0) return DSV_OK;
  if (!in_uv || !out32) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  for (size_t i = 0; i < n; i++) {
    memcpy(out32 + 32 * i, in_uv + 64 * i + 32, 32);
    out32[32 * i + 31] |= (uint8_t)((in_uv[64 * i] & 1) << 7);
  }
  return DSV_OK;
}

int dsv_decompress_points(const uint8_t* in32, size_t n, uint8_t* out_uv, uint8_t* ok) {
  if (n && (!in32 || !out_uv || !ok)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_HOST_PROLOGUE(n);
  DSV_HOST_LOCK();
  if (int r = ensure_stage(ctx, align_up(n * 32, 256) + align_up(n * 64, 256) + align_up(n, 256))) return r;
  Stager st(ctx.stage);
  uint8_t *din = st.take(n * 32), *dout = st.take(n * 64), *dok = st.take(n);
  H2D(din, in32, n * 32);
  if (int r = decompress_on(ctx, din, 32, n, dout, dok, 0, 0)) return r;
  D2H(out_uv, dout, n * 64);
  D2H(ok, dok, n);
  HIP_TRY(hipStreamSynchronize(0));
  return DSV_OK;
}

extern "C++" {
namespace dsvh {
WireWs carve_wire(Stager& x, size_t n) {
  WireWs w;
  w.u = x.take(n * 32);
  w.R = x.take(n * 64);
  w.Rp = x.take(n * 64);
  w.P0 = x.take(n * 64);
  w.P1 = x.take(n * 64);
  w.valid = x.take(n);
  return w;
}
// sig: n records of sig_bytes = 32 (u) + 32 per nonce point; pk: n records of pk_bytes = 32 per key point
int decode_wire(Context& ctx, int scheme, const uint8_t* sig, const uint8_t* pk, size_t n, const Items& out,
                uint8_t* valid, hipStream_t st) {
  const SchemeLayout& L = layout(scheme);
  const int ns = (int)(L.sig_bytes / 32) - 1;
  launch_gather32(sig, L.sig_bytes, n, const_cast<uint8_t*>(out.u), st);
  for (int k = 0; k < L.points; k++) {
    const uint8_t* in = k < ns ? sig + 32 * (1 + k) : pk + 32 * (k - ns);
    if (int r = decompress_on(ctx, in, k < ns ? L.sig_bytes : L.pk_bytes, n, const_cast<uint8_t*>(out.pt[k]), valid,
                              k > 0, st))
      return r;
  }
  return DSV_OK;
}
}  // namespace dsvh
namespace {
// shared body of the *_wire entry points
constexpr size_t kWireItemBytes = 32 + 4 * 64 + 1;
int verify_wire_on(Context& ctx, int scheme, const uint8_t* dsig, const uint8_t* dpk, const void* dm,
                   size_t cnt, void* dok, const WireWs& x, void* vws, hipStream_t st) {
  const Items in = x.items(scheme, dm);
  if (int r = decode_wire(ctx, scheme, dsig, dpk, cnt, in, x.valid, st)) return r;
  if (int rc = verify_on(ctx, in, cnt, dok, vws, st, x.valid)) return rc;
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}
// device-pointer form: serialized records already resident in HBM
int verify_wire_dev(int scheme, const void* sig, const void* pk, const void* m, size_t n, void* ok,
                    void* workspace, void* stream) {
  if (n && (!sig || !pk || !m || !ok || !workspace)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  if (((uintptr_t)sig | (uintptr_t)pk) & 15) return fail(DSV_ERR_INVALID_ARGUMENT, "records must be 16-byte aligned");
  DSV_DEV_PROLOGUE(n, ok);
  Stager x(static_cast<uint8_t*>(workspace));
  const WireWs w = carve_wire(x, n);
  void* vws = x.take(dsv_workspace_bytes(n));
  return verify_wire_on(ctx, scheme, (const uint8_t*)sig, (const uint8_t*)pk, m, n, ok, w, vws,
                        (hipStream_t)stream);
}
}  // namespace

namespace dsvh {
int verify_wire(Context& ctx, int scheme, const uint8_t* sig, const uint8_t* pk, const uint8_t* m,
                size_t n, uint8_t* ok) {
  const size_t sig_bytes = layout(scheme).sig_bytes, pk_bytes = layout(scheme).pk_bytes;
  const HostIn ins[3] = {{sig, sig_bytes}, {pk, pk_bytes}, {m, 32}};
  Context* cp = &ctx;
  return run_pipelined(ctx, ins, 3, ok, n, 0, kWireItemBytes, NoPrep{},
                       [=](const Staged& g, size_t off, size_t cnt, void* dok, void* ws, Stager& x, hipStream_t st) {
    return verify_wire_on(*cp, scheme, g.p[0] + off * g.bytes[0], g.p[1] + off * g.bytes[1],
                          g.p[2] + off * g.bytes[2], cnt, dok, carve_wire(x, cnt), ws, st);
  });
}
}  // namespace dsvh
namespace {
int verify_wire_host(int scheme, const uint8_t* sig, const uint8_t* pk, const uint8_t* m, size_t n, uint8_t* ok) {
  if (n && (!sig || !pk || !m || !ok)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_HOST_PROLOGUE(n);
  return verify_wire(ctx, scheme, sig, pk, m, n, ok);
}
}  // namespace
}  // extern "C++"

size_t dsv_wire_workspace_bytes(size_t n) {
  return align_up(n * 32, 256) + 4 * align_up(n * 64, 256) + align_up(n, 256) +
         align_up(dsv_workspace_bytes(n), 256) + 256;
}
int dsv_verify_single_wire_dev(const void* sig64, const void* pk32, const void* m, size_t n, void* ok,
                               void* workspace, void* stream) {
  return verify_wire_dev(0, sig64, pk32, m, n, ok, workspace, stream);
}
int dsv_verify_double_wire_dev(const void* sig96, const void* pk64, const void* m, size_t n, void* ok,
                               void* workspace, void* stream) {
  return verify_wire_dev(1, sig96, pk64, m, n, ok, workspace, stream);
}
int dsv_verify_vargen_wire_dev(const void* sig64, const void* pk64, const void* m, size_t n, void* ok,
                               void* workspace, void* stream) {
  return verify_wire_dev(2, sig64, pk64, m, n, ok, workspace, stream);
}

int dsv_verify_single_wire(const uint8_t* sig64, const uint8_t* pk32, const uint8_t* m, size_t n,
                           uint8_t* ok) {
  return verify_wire_host(0, sig64, pk32, m, n, ok);
}
int dsv_verify_double_wire(const uint8_t* sig96, const uint8_t* pk64, const uint8_t* m, size_t n,
                           uint8_t* ok) {
  return verify_wire_host(1, sig96, pk64, m, n, ok);
}
int dsv_verify_vargen_wire(const uint8_t* sig64, const uint8_t* pk64, const uint8_t* m, size_t n,
                           uint8_t* ok) {
  return verify_wire_host(2, sig64, pk64, m, n, ok);
}

}  // extern "C"
