// rlc_probe.hip — TEST-ONLY: one group's batch-fast-accept aggregate under a CHOSEN weight key
// (tests/test_gpu_rlc_known_key.py).  The engine draws the ChaCha key of the weights z_i per call and never
// shows it; with the key chosen here the prep kernels' outputs can be compared word for word with a
// Python-integer model (tests/rlc_weights.py), and the aggregate can be shown to accept exactly when the stated
// weighted sum is the identity.
//
// No kernel of its own and no copy of the engine's: it links against libdsv.so and drives the engine's own
// launchers (rlc.h, keyed_rlc.h) in the order dsv_rlc.hip / dsv_keyed_rlc.hip do —
//   begin -> [hash] -> prep + bucket pass (one range, or two with a merge) -> [keys' terms] -> tail
// — on the null stream, waits, and copies back the sub-groups' flag words, ok[] and, on request, what the prep
// wrote.  Built by schnorr_amd/build.py: build_rlc_probe() into schnorr_amd/libdsv_rlcprobe.so; not part of libdsv.so.
#include "dsv_host.h"
#include "keyed_rlc.h"
#include "keyset_host.h"

using namespace dsvh;

extern "C" {
struct dsv_rlcprobe_args {
  int32_t scheme, window_bits, groups, reserved;
  uint64_t n;
  uint64_t boundary;  // unkeyed, groups == 1: != 0 runs the bucket pass in the ranges [0, boundary) and [boundary, n)
  uint32_t key[8];
  // device memory: the items (points the scheme does not have, and the keyed form's key columns: null)
  const void *u, *R, *Rp, *PK, *PKp, *Gen, *m;
  const void *c, *valid;  // both or neither; null: the challenge hash runs (m needed)
  const dsv_keyset* keyset;  // keyed entry only
  const void* key_idx;
  // host memory; any of the last five may be null
  uint32_t* flags;    // groups x 4 words
  uint8_t* ok;        // n
  uint16_t* digits;   // groups x digits_stride
  uint32_t* fsc;      // groups x fsc_stride
  uint32_t* pts;      // groups x pts_stride
  uint64_t* ksum;     // groups x k x scalars x 8 (keyed)
  uint32_t* touched;  // groups x k (keyed)
};
}

namespace {
constexpr size_t kProbeMaxItems = (size_t)1 << 20;

struct ProbeCarve {
  uint8_t *c, *valid, *ok;
  RlcBuffers b;
  KeyedRlcBuffers kb;
  size_t bytes;
};
// c, valid, ok and one flag block of its own, then the engine's own carves of the bucket and per-key buffers
ProbeCarve carve_probe(uint8_t* base, const RlcPlan& p, size_t n, int scheme, bool keyed, size_t k) {
  ProbeCarve r = {};
  Stager st(base);
  r.c = st.take(n * 32);
  r.valid = st.take(n);
  r.ok = st.take(n);
  r.b.flags = reinterpret_cast<u32*>(st.take(kRlcGroupFlagWords * sizeof(u32)));
  carve_rlc_buffers(st, p, r.b);
  if (keyed) carve_keyed_rlc_buffers(st, p, scheme, k, r.kb);
  r.bytes = st.off;
  return r;
}
struct DeviceBlock {
  void* p = nullptr;
  ~DeviceBlock() {
    if (p) (void)hipFree(p);
  }
};
int check_args(const dsv_rlcprobe_args* a, bool keyed) {
  if (!a || a->scheme < 0 || a->scheme > 2 || a->n == 0 || a->n > kProbeMaxItems || !rlc_bits_ok(a->window_bits) ||
      a->groups < 1 || a->groups > kRlcMaxSub)
    return fail(DSV_ERR_INVALID_ARGUMENT, "rlc probe: bad geometry");
  if (a->boundary && (keyed || a->groups != 1 || a->boundary >= a->n))
    return fail(DSV_ERR_INVALID_ARGUMENT, "rlc probe: two ranges need the unkeyed form, one sub-group, 0 < boundary < n");
  if (keyed && (!a->keyset || !a->keyset->alive || a->keyset->scheme != a->scheme || !a->key_idx))
    return fail(DSV_ERR_INVALID_ARGUMENT, "rlc probe: no key set of this scheme");
  return DSV_OK;
}
RlcPlan probe_plan(const dsv_rlcprobe_args* a, bool keyed) {
  return rlc_group_plan(a->scheme, a->n, a->window_bits, a->groups, keyed);
}
int geometry(const dsv_rlcprobe_args* a, bool keyed, uint64_t* out) {
  if (int r = check_args(a, keyed)) return r;
  if (!out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  const RlcPlan p = probe_plan(a, keyed);
  const size_t k = keyed ? a->keyset->k : 0;
  const ProbeCarve cv = carve_probe(reinterpret_cast<uint8_t*>((uintptr_t)4096), p, a->n, a->scheme, keyed, k);
  const uint64_t v[8] = {p.groups, p.sub, cv.b.pts_stride, cv.b.fsc_stride, cv.b.digits_stride, p.rows, p.row_stride,
                         keyed ? (uint64_t)k * keyed_scalars(a->scheme) * 8 : 0};
  for (int i = 0; i < 8; i++) out[i] = v[i];
  return DSV_OK;
}
int run(const dsv_rlcprobe_args* a, bool keyed) {
  if (int r = check_args(a, keyed)) return r;
  const int scheme = a->scheme;
  const size_t n = a->n;
  const uint8_t* pts[5] = {(const uint8_t*)a->R, (const uint8_t*)a->Rp, (const uint8_t*)a->PK, (const uint8_t*)a->PKp,
                           (const uint8_t*)a->Gen};
  const bool need[5] = {true, scheme == 1, !keyed, !keyed && scheme == 1, !keyed && scheme == 2};
  bool missing = !a->u || !a->flags || !a->ok || (!a->c != !a->valid) || (!a->c && !a->m);
  for (int k = 0; k < 5; k++) missing = missing || (need[k] && !pts[k]);
  if (missing) return fail(DSV_ERR_INVALID_ARGUMENT, "rlc probe: null pointer");
  Context* ctxp = nullptr;
  if (int r = device_context(a->u, ctxp)) return r;
  Context& ctx = *ctxp;
  DSV_ON_DEVICE(ctx);
  const RlcPlan plan = probe_plan(a, keyed);
  const size_t nk = keyed ? a->keyset->k : 0;
  const size_t bytes = carve_probe(reinterpret_cast<uint8_t*>((uintptr_t)4096), plan, n, scheme, keyed, nk).bytes;
  DeviceBlock mem;
  HIP_TRY(hipMalloc(&mem.p, bytes + 256));
  // (the engine's workspaces come uninitialised: whatever a kernel reads it must have written)
  HIP_TRY(hipMemset(mem.p, 0xCD, bytes + 256));
  const ProbeCarve cv = carve_probe(static_cast<uint8_t*>(mem.p), plan, n, scheme, keyed, nk);
  const hipStream_t s = nullptr;
  ChaChaKey key;
  for (int k = 0; k < 8; k++) key.w[k] = a->key[k];
  HIP_TRY(launch_rlc_begin(cv.b, s));
  const uint8_t* c = (const uint8_t*)a->c;
  const uint8_t* valid = (const uint8_t*)a->valid;
  if (!c) {
    Items items;
    if (keyed) items = scheme == 1 ? make_items(1, a->u, {a->R, a->Rp}, a->m) : make_items(scheme, a->u, {a->R}, a->m);
    else if (scheme == 0) items = make_items(0, a->u, {a->R, a->PK}, a->m);
    else if (scheme == 1) items = make_items(1, a->u, {a->R, a->Rp, a->PK, a->PKp}, a->m);
    else items = make_items(2, a->u, {a->R, a->PK, a->Gen}, a->m);
    launch_hash(items, n, cv.c, cv.valid, s);
    HIP_TRY(hipGetLastError());
    c = cv.c, valid = cv.valid;
  }
  RlcInputs in = {};
  in.u = (const uint8_t*)a->u, in.c = c, in.valid = valid;
  in.pk[0] = pts[2], in.pk[1] = pts[3], in.r[0] = pts[0], in.r[1] = pts[1], in.gen = pts[4];
  if (keyed) {
    const KeyedRlcKeys keys{a->keyset->tables, a->keyset->key_ok, a->keyset->k};
    HIP_TRY(launch_keyed_rlc_prep(scheme, plan, cv.b, cv.kb, in, (const uint32_t*)a->key_idx, keys, key, cv.ok, s));
    HIP_TRY(launch_rlc_sort(plan, cv.b, false, s));
    HIP_TRY(launch_keyed_rlc_terms(scheme, plan, cv.b, cv.kb, keys, s));
    HIP_TRY(launch_rlc_finish(plan, cv.b, ctx.table[0], ctx.table[1], false, s, cv.kb.terms));
  } else if (a->boundary) {
    HIP_TRY(launch_rlc_buckets(scheme, rlc_range(plan, 0, a->boundary), cv.b, in, key, cv.ok, false, s));
    HIP_TRY(launch_rlc_buckets(scheme, rlc_range(plan, a->boundary, n - a->boundary), cv.b, in, key, cv.ok, true, s));
    HIP_TRY(launch_rlc_finish(plan, cv.b, ctx.table[0], ctx.table[1], true, s));
  } else {
    HIP_TRY(launch_rlc_buckets(scheme, plan, cv.b, in, key, cv.ok, false, s));
    HIP_TRY(launch_rlc_finish(plan, cv.b, ctx.table[0], ctx.table[1], false, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  const size_t G = plan.groups;
  HIP_TRY(hipMemcpy(a->flags, cv.b.flags + 4, G * 4 * sizeof(u32), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(a->ok, cv.ok, n, hipMemcpyDeviceToHost));
  if (a->digits) HIP_TRY(hipMemcpy(a->digits, cv.b.digits, G * cv.b.digits_stride * 2, hipMemcpyDeviceToHost));
  if (a->fsc) HIP_TRY(hipMemcpy(a->fsc, cv.b.fsc, G * cv.b.fsc_stride * 4, hipMemcpyDeviceToHost));
  if (a->pts) HIP_TRY(hipMemcpy(a->pts, cv.b.pts, G * cv.b.pts_stride * 4, hipMemcpyDeviceToHost));
  if (keyed && a->ksum)
    HIP_TRY(hipMemcpy(a->ksum, cv.kb.ksum, G * nk * (size_t)keyed_scalars(scheme) * 8 * 8, hipMemcpyDeviceToHost));
  if (keyed && a->touched) HIP_TRY(hipMemcpy(a->touched, cv.kb.touched, G * nk * sizeof(u32), hipMemcpyDeviceToHost));
  return DSV_OK;
}
}  // namespace

extern "C" {
// out[8]: sub-groups, items per sub-group, then the per-sub-group strides (in elements) of pts, fsc and digits,
// digit rows, digits per row, 64-bit chunk words per sub-group of ksum (keyed)
int dsv_rlcprobe_geometry(const dsv_rlcprobe_args* a, uint64_t* out) { return geometry(a, false, out); }
int dsv_rlcprobe_geometry_keyed(const dsv_rlcprobe_args* a, uint64_t* out) { return geometry(a, true, out); }
int dsv_rlcprobe_run(const dsv_rlcprobe_args* a) { return run(a, false); }
int dsv_rlcprobe_run_keyed(const dsv_rlcprobe_args* a) { return run(a, true); }
// two draws of the engine's per-call weight key (dsv_rlc.hip: rlc_random_key)
int dsv_rlcprobe_random_keys(uint32_t* out16) {
  if (!out16) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  for (int d = 0; d < 2; d++) {
    ChaChaKey key;
    if (int r = rlc_random_key(key)) return r;
    for (int k = 0; k < 8; k++) out16[8 * d + k] = key.w[k];
  }
  return DSV_OK;
}
}
