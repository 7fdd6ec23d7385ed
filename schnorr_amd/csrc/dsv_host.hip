// dsv_host.hip — the host-pointer entry points of include/dsv.h: every verify scheme over affine bytes,
// projective points (`to_hash_inputs` on the device), the reference's in-memory Montgomery limbs and
// columns of typed objects (what the Rust `verify_batch(&[Signature], &[PublicKey], &[BlsScalar])`
// binds), their *_multi forms over all initialised devices, and the submit / wait form.  All of them
// run the chunked pipeline of dsv_pipeline.h.
#include "dsv_pipeline.h"
#include "keyed_mont.h"

namespace dsvh {
std::atomic<int> g_host_threads{0};
}
using namespace dsvh;

extern "C" {

extern "C++" {
namespace {
// whole-chunk `to_hash_inputs` of the scheme's points (d: u, points..., m); fills the staged view of the
// affine path.  mont: the scalars d[0] / d[1 + np] are Montgomery limbs — the same launch converts them
// into two arrays of the scratch
int prep_normalize(const Context& ctx, int scheme, bool mont, const void* const* d, size_t cnt, Stager& x,
                   hipStream_t st, Staged& g) {
  const int np = layout(scheme).points;
  uint8_t *cu = nullptr, *cm = nullptr;
  if (mont) cu = x.take(cnt * 32), cm = x.take(cnt * 32);
  const uint8_t* in[4] = {};
  uint8_t* out[4] = {};
  for (int k = 0; k < np; k++) {
    in[k] = (const uint8_t*)d[1 + k];
    out[k] = x.take(cnt * 64);
    g.p[1 + k] = out[k];
    g.bytes[1 + k] = 64;
  }
  uint8_t* valid = x.take(cnt);
  u32* prefix = reinterpret_cast<u32*>(x.take(normalize_prefix_bytes(cnt, np)));
  normalize_on(scheme, in, out, cnt, valid, prefix, st, mont ? (const uint8_t*)d[0] : nullptr,
               (const uint8_t*)d[1 + np], cu, cm, ctx.norm_per_lane, ctx.norm_block);
  HIP_TRY(hipGetLastError());
  g.p[0] = mont ? cu : (const uint8_t*)d[0];
  g.p[1 + np] = mont ? cm : (const uint8_t*)d[1 + np];
  g.bytes[0] = g.bytes[1 + np] = 32;
  g.valid = valid;
  return DSV_OK;
}
// one shard [off, off + cnt) of a column batch on one device through the chunked pipeline: affine items
// as they are, projective points / Montgomery limbs normalised chunk by chunk first (the chunk's
// scratch holds the affine points; the pipeline's own verify workspace is used per sub-batch)
int verify_host_shard(Context& ctx, int scheme, int form, const dsv_column* cols, size_t off, size_t cnt, uint8_t* ok) {
  HostIn ins[kMaxHostIn];
  const size_t nin = column_inputs(scheme, form, cols, off, ins);
  Context* cp = &ctx;
  auto part = [=](const Staged& g, size_t o, size_t c, void* dok, void* ws, Stager&, hipStream_t st) {
    // (g.valid: the chunk-level preprocessing's verdict on the items)
    if (int rc = verify_on(*cp, g.items(scheme, o), c, dok, ws, st, g.valid ? g.valid + o : nullptr)) return rc;
    HIP_TRY(hipGetLastError());
    return (int)DSV_OK;
  };
  const unsigned flags = scheme != 0 ? kPipeHeavy : 0u;
  if (form == kAffine) return run_pipelined(ctx, ins, nin, ok + off, cnt, 0, 0, NoPrep{}, part, flags);
  const bool mont = form == kMont;
  return run_pipelined(ctx, ins, nin, ok + off, cnt, mont ? kMontItemBytes : kExtItemBytes, 0,
                       [=](const void* const* d, size_t c, Stager& x, hipStream_t st, Staged& g) {
                         return prep_normalize(*cp, scheme, mont, d, c, x, st, g);  // ONE launch
                       },
                       part, flags);
}
// the same items as columns of dense arrays
size_t item_columns(const Items& in, size_t pt_bytes, dsv_column* cols) {
  const int np = layout(in.scheme).points;
  cols[0] = dsv_column{in.u, 32};
  for (int k = 0; k < np; k++) cols[1 + k] = dsv_column{in.pt[k], pt_bytes};
  cols[1 + np] = dsv_column{in.m, 32};
  return (size_t)np + 2;
}
// affine / projective arrays in host memory.  The plain forms check their pointers before n, the *_multi
// forms after it
int verify_host(int form, const Items& in, size_t n, uint8_t* ok, bool multi) {
  if (multi) {
    if (int r = check_n(n)) return r;
    if (n == 0) return DSV_OK;
  }
  if (n && (in.any_null() || !ok)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  dsv_column cols[kMaxHostIn];
  item_columns(in, form_pt_bytes(form), cols);
  return verify_host_cols(in.scheme, form, cols, n, ok, multi);
}
// Montgomery limbs as dense arrays: the column forms' checks ("column k: ...")
int verify_mont(const Items& in, size_t n, uint8_t* ok, bool multi) {
  dsv_column cols[kMaxHostIn];
  item_columns(in, 96, cols);
  return verify_host_cols(in.scheme, kMont, cols, n, ok, multi);
}
}  // namespace
namespace dsvh {
size_t column_inputs(int scheme, int form, const dsv_column* cols, size_t off, HostIn* ins) {
  const size_t nc = (size_t)layout(scheme).points + 2;
  for (size_t k = 0; k < nc; k++) {
    const size_t width = (k == 0 || k == nc - 1) ? 32 : form_pt_bytes(form);
    ins[k] = HostIn{static_cast<const uint8_t*>(cols[k].base) + off * cols[k].stride, width, cols[k].stride};
  }
  return nc;
}
int check_cols(int scheme, const dsv_column* cols, size_t n, const uint8_t* ok, int form) {
  if (int r = check_n(n)) return r;
  if (n == 0) return DSV_OK;
  if (!cols || !ok) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  const int nc = layout(scheme).points + 2;
  for (int k = 0; k < nc; k++) {
    const size_t width = (k == 0 || k == nc - 1) ? 32 : form_pt_bytes(form);
    if (!cols[k].base) return fail(DSV_ERR_INVALID_ARGUMENT, "column %d: null pointer", k);
    if (cols[k].stride < width) return fail(DSV_ERR_INVALID_ARGUMENT, "column %d: stride %zu < %zu", k, cols[k].stride, width);
  }
  return DSV_OK;
}
int verify_host_cols(int scheme, int form, const dsv_column* cols, size_t n, uint8_t* ok, bool multi) {
  if (int r = check_cols(scheme, cols, n, ok, form)) return r;
  if (n == 0) return DSV_OK;
  if (multi)
    return run_multi(n, [=](Context& ctx, size_t off, size_t cnt) {
      return verify_host_shard(ctx, scheme, form, cols, off, cnt, ok);
    });
  Context* ctxp = nullptr;
  if (int r = host_context(ctxp)) return r;
  return verify_host_shard(*ctxp, scheme, form, cols, 0, n, ok);
}
}  // namespace dsvh
}  // extern "C++"

int dsv_verify_single(const uint8_t* u, const uint8_t* R_uv, const uint8_t* PK_uv,
                      const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kAffine, make_items(0, u, {R_uv, PK_uv}, m), n, ok, false);
}
int dsv_verify_double(const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                      const uint8_t* PK_uv, const uint8_t* PKp_uv, const uint8_t* m, size_t n,
                      uint8_t* ok) {
  return verify_host(kAffine, make_items(1, u, {R_uv, Rp_uv, PK_uv, PKp_uv}, m), n, ok, false);
}
int dsv_verify_vargen(const uint8_t* u, const uint8_t* R_uv, const uint8_t* PK_uv,
                      const uint8_t* Gen_uv, const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kAffine, make_items(2, u, {R_uv, PK_uv, Gen_uv}, m), n, ok, false);
}

// ---- the same over ALL initialised devices (what a Rust verify_batch on an 8-GPU node calls) ----
int dsv_verify_single_multi(const uint8_t* u, const uint8_t* R_uv, const uint8_t* PK_uv,
                            const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kAffine, make_items(0, u, {R_uv, PK_uv}, m), n, ok, true);
}
int dsv_verify_double_multi(const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                            const uint8_t* PK_uv, const uint8_t* PKp_uv, const uint8_t* m, size_t n,
                            uint8_t* ok) {
  return verify_host(kAffine, make_items(1, u, {R_uv, Rp_uv, PK_uv, PKp_uv}, m), n, ok, true);
}
int dsv_verify_vargen_multi(const uint8_t* u, const uint8_t* R_uv, const uint8_t* PK_uv,
                            const uint8_t* Gen_uv, const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kAffine, make_items(2, u, {R_uv, PK_uv, Gen_uv}, m), n, ok, true);
}

// ---- projective inputs: the reference's in-memory types ------------------------------------
// `PublicKey::from(&sk)` = GENERATOR_EXTENDED * sk and R = GENERATOR_EXTENDED * r are JubJubExtended
// values with z != 1 (/root/reference/src/keys/public.rs:61-67, src/keys/secret.rs:159), and the
// reference's verify starts with `to_hash_inputs` (src/signatures.rs:131, :280-281): one field
// inversion per point.  The *_ext entry points take (u, v, z) and do that step on the device —
// Montgomery's trick over all points of an item and over the items of a lane (k_normalize_uvz) —
// so a caller (the Rust verify_batch) does no field arithmetic on the host at all.  (The *_ext_dev
// forms: dsv_device.hip.)

// JubJubExtended::to_hash_inputs for n points: (u, v, z) -> (u/z, v/z); ok[i] = 0 for z = 0 or a
// non-canonical coordinate (the reference would panic / cannot hold such a value)
int dsv_to_hash_inputs(const uint8_t* in_uvz, size_t n, uint8_t* out_uv, uint8_t* ok) {
  if (n && (!in_uvz || !out_uv || !ok)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_HOST_PROLOGUE(n);
  DSV_HOST_LOCK();
  const size_t pre = normalize_prefix_bytes(n, 1);
  if (int r = ensure_stage(ctx, align_up(n * 96, 256) + align_up(n * 64, 256) + align_up(n, 256) +
                                    align_up(pre, 256)))
    return r;
  Stager st(ctx.stage);
  uint8_t *din = st.take(n * 96), *dout = st.take(n * 64), *dok = st.take(n);
  u32* dpre = reinterpret_cast<u32*>(st.take(pre));
  H2D(din, in_uvz, n * 96);
  NormalizeArgs a = {};
  a.in[0] = din;
  a.out[0] = dout;
  launch_normalize_uvz(a, 1, n, dok, dpre, 0);
  HIP_TRY(hipGetLastError());
  D2H(out_uv, dout, n * 64);
  D2H(ok, dok, n);
  HIP_TRY(hipStreamSynchronize(0));
  return DSV_OK;
}

int dsv_verify_single_ext(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz,
                          const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kExt, make_items(0, u, {R_uvz, PK_uvz}, m), n, ok, false);
}
int dsv_verify_double_ext(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* Rp_uvz,
                          const uint8_t* PK_uvz, const uint8_t* PKp_uvz, const uint8_t* m, size_t n,
                          uint8_t* ok) {
  return verify_host(kExt, make_items(1, u, {R_uvz, Rp_uvz, PK_uvz, PKp_uvz}, m), n, ok, false);
}
int dsv_verify_vargen_ext(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz,
                          const uint8_t* Gen_uvz, const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kExt, make_items(2, u, {R_uvz, PK_uvz, Gen_uvz}, m), n, ok, false);
}
int dsv_verify_single_ext_multi(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz,
                                const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kExt, make_items(0, u, {R_uvz, PK_uvz}, m), n, ok, true);
}
int dsv_verify_double_ext_multi(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* Rp_uvz,
                                const uint8_t* PK_uvz, const uint8_t* PKp_uvz, const uint8_t* m,
                                size_t n, uint8_t* ok) {
  return verify_host(kExt, make_items(1, u, {R_uvz, Rp_uvz, PK_uvz, PKp_uvz}, m), n, ok, true);
}
int dsv_verify_vargen_ext_multi(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz,
                                const uint8_t* Gen_uvz, const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_host(kExt, make_items(2, u, {R_uvz, PK_uvz, Gen_uvz}, m), n, ok, true);
}

// ---- the reference's in-memory representation: Montgomery limbs --------------------------------
// The Rust types hold every field element as `[u64; 4]` Montgomery limbs with R = 2^256
// (`BlsScalar(pub [u64; 4])`, dusk-bls12_381 0.13; `JubJubScalar`, the coordinates of
// `JubJubExtended`, dusk-jubjub 0.14 — /root/reference/Cargo.toml:25-26; the fields:
// src/signatures.rs:58-61, src/keys/public.rs:59).  `to_bytes()` is one Montgomery reduction per
// element — eight per single signature, fourteen per double one — on ONE host thread: ~30x below the
// engine.  The *_mont entry points take the limbs as they lie in memory:
//   points  (u R, v R, z R) : straight into k_normalize_uvz — a quotient does not see the common factor
//   u, m                    : two reductions per signature inside the same kernel (scalars_from_mont_item)
// so a binding copies bytes and nothing else; the *_mont_cols forms even take the typed objects
// where they lie (one strided column per field) and gather them into the pinned staging with the
// pipeline's copy threads — no intermediate structure of arrays on the host.

// copy threads of the host entry points (per process): n >= 1 sets, 0 restores the default
// ($DSV_HOST_THREADS, else 4); returns the value now in force
int dsv_set_host_threads(int n) {
  g_host_threads.store(n > 0 ? clamp_host_threads(n) : 0, std::memory_order_relaxed);
  return host_copy_threads();
}

// ---- asynchronous form: submit returns at once, the batch runs on a library-owned driver thread ----
// What a caller with a stream of batches uses to keep the GPU busy across calls: while batch k's last
// chunks are on the GPU, batch k + 1's driver already gathers, transfers and enqueues its first ones
// (each call in flight owns a Pipe; the compute lanes are shared, so the GPU sees one FIFO of
// sub-batches).  A third submit simply waits for a pipe inside its driver thread.
struct dsv_job {
  std::thread th;
  std::mutex m;
  std::condition_variable cv;
  bool started = false;
  std::atomic<bool> finished{false};
  int rc = DSV_OK;
  std::string err;
  int kind = 0;
  const dsv_keyset* ks = nullptr;  // a keyed typed-object form (keyed_mont.h: `kind` says which); null: unkeyed
  int ncols = 0;
  dsv_column cols[6] = {};
  size_t n = 0;
  uint8_t* ok = nullptr;
};
extern "C++" {
namespace dsvh {
// (arguments checked by the caller)
int submit_cols_job(const dsv_keyset* ks, int kind, const dsv_column* cols, int ncols, size_t n, uint8_t* ok,
                    dsv_job** out) {
  if (g_primary.load(std::memory_order_acquire) < 0)
    return fail(DSV_ERR_NOT_INITIALIZED, "dsv_init() has not been called");
  dsv_job* j = new (std::nothrow) dsv_job;
  if (!j) return fail(DSV_ERR_HIP, "out of host memory");
  j->kind = kind;
  j->ks = ks;
  j->ncols = ncols;
  j->n = n;
  j->ok = ok;
  for (int k = 0; k < ncols; k++) j->cols[k] = cols[k];
  auto job_count = [](int d) {
    std::lock_guard<std::mutex> lk(g_jobs_mu);
    g_jobs += d;
    if (g_jobs == 0) g_jobs_cv.notify_all();
  };
  job_count(+1);
  try {
    j->th = std::thread([j, job_count] {
      // a keyed job holds the key-set registry's shared lock from before submit returns to its last verdict:
      // dsv_keyset_destroy and dsv_shutdown* (exclusive) wait for the job instead of freeing the set under it.
      // Nothing the driver does takes that lock again, and dsv_shutdown_device waits for the jobs before it
      // asks for the registry, holding no lock a driver needs.
      std::shared_lock<std::shared_mutex> registry(keyset_mutex(), std::defer_lock);
      if (j->ks) registry.lock();
      {
        std::lock_guard<std::mutex> lk(j->m);
        j->started = true;
      }
      j->cv.notify_all();
      {  // the driver gathers the first shard itself: next to the device that takes it
        const int d = t_device >= 0 ? t_device : g_primary.load(std::memory_order_acquire);
        if (d >= 0 && d < kMaxDevices) (void)pin_this_thread(g_ctx[d].numa_cpus);
      }
      if (!j->ks)
        j->rc = verify_host_cols(j->kind, kMont, j->cols, j->n, j->ok, true);
      else if (j->kind == kOpenMontJob)
        j->rc = verify_keyed_open_mont_cols_locked(j->ks, j->cols, j->n, j->ok, nullptr);
      else
        j->rc = verify_keyed_mont_cols_locked(j->ks, j->cols, j->n, j->ok);
      if (j->rc) j->err = g_err;  // the text lives in this thread's thread-local
      if (j->ks) registry.unlock();
      j->finished.store(true, std::memory_order_release);
      job_count(-1);
    });
  } catch (...) {
    job_count(-1);
    delete j;
    return fail(DSV_ERR_HIP, "could not start the driver thread of the batch");
  }
  {
    // jobs take their place in the device's queue in submission order: return once the driver runs
    // (it queues for its pipe within microseconds; the next submit has a thread to start first)
    std::unique_lock<std::mutex> lk(j->m);
    j->cv.wait(lk, [j] { return j->started; });
  }
  *out = j;
  return DSV_OK;
}
}  // namespace dsvh
namespace {
int submit_mont_cols(int kind, const dsv_column* cols, size_t n, uint8_t* ok, dsv_job** out) {
  if (!out) return fail(DSV_ERR_INVALID_ARGUMENT, "null job pointer");
  *out = nullptr;
  if (int r = check_cols(kind, cols, n, ok, kMont)) return r;
  return submit_cols_job(nullptr, kind, cols, n ? layout(kind).points + 2 : 0, n, ok, out);
}
}  // namespace
}  // extern "C++"
int dsv_verify_single_mont_cols_submit(const dsv_column* cols, size_t n, uint8_t* ok, dsv_job** job) { return submit_mont_cols(0, cols, n, ok, job); }
int dsv_verify_double_mont_cols_submit(const dsv_column* cols, size_t n, uint8_t* ok, dsv_job** job) { return submit_mont_cols(1, cols, n, ok, job); }
int dsv_verify_vargen_mont_cols_submit(const dsv_column* cols, size_t n, uint8_t* ok, dsv_job** job) { return submit_mont_cols(2, cols, n, ok, job); }
int dsv_job_done(const dsv_job* job) {
  if (!job) return fail(DSV_ERR_INVALID_ARGUMENT, "null job");
  return job->finished.load(std::memory_order_acquire) ? 1 : 0;
}
int dsv_job_wait(dsv_job* job) {
  if (!job) return fail(DSV_ERR_INVALID_ARGUMENT, "null job");
  if (job->th.joinable()) job->th.join();
  const int rc = job->rc;
  if (rc) g_err = job->err;
  delete job;
  return rc;
}
int dsv_max_in_flight(void) { return kPipes; }

int dsv_verify_single_mont_cols(const dsv_column* cols, size_t n, uint8_t* ok) { return verify_host_cols(0, kMont, cols, n, ok, true); }
int dsv_verify_double_mont_cols(const dsv_column* cols, size_t n, uint8_t* ok) { return verify_host_cols(1, kMont, cols, n, ok, true); }
int dsv_verify_vargen_mont_cols(const dsv_column* cols, size_t n, uint8_t* ok) { return verify_host_cols(2, kMont, cols, n, ok, true); }

int dsv_verify_single_mont(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz, const uint8_t* m,
                           size_t n, uint8_t* ok) {
  return verify_mont(make_items(0, u, {R_uvz, PK_uvz}, m), n, ok, false);
}
int dsv_verify_double_mont(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* Rp_uvz,
                           const uint8_t* PK_uvz, const uint8_t* PKp_uvz, const uint8_t* m, size_t n,
                           uint8_t* ok) {
  return verify_mont(make_items(1, u, {R_uvz, Rp_uvz, PK_uvz, PKp_uvz}, m), n, ok, false);
}
int dsv_verify_vargen_mont(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz,
                           const uint8_t* Gen_uvz, const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_mont(make_items(2, u, {R_uvz, PK_uvz, Gen_uvz}, m), n, ok, false);
}
int dsv_verify_single_mont_multi(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz,
                                 const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_mont(make_items(0, u, {R_uvz, PK_uvz}, m), n, ok, true);
}
int dsv_verify_double_mont_multi(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* Rp_uvz,
                                 const uint8_t* PK_uvz, const uint8_t* PKp_uvz, const uint8_t* m, size_t n,
                                 uint8_t* ok) {
  return verify_mont(make_items(1, u, {R_uvz, Rp_uvz, PK_uvz, PKp_uvz}, m), n, ok, true);
}
int dsv_verify_vargen_mont_multi(const uint8_t* u, const uint8_t* R_uvz, const uint8_t* PK_uvz,
                                 const uint8_t* Gen_uvz, const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_mont(make_items(2, u, {R_uvz, PK_uvz, Gen_uvz}, m), n, ok, true);
}

int dsv_challenge_single(const uint8_t* R_uv, const uint8_t* m, size_t n, uint8_t* c) {
  if (n && (!R_uv || !m || !c)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_HOST_PROLOGUE(n);
  DSV_HOST_LOCK();
  if (int r = ensure_stage(ctx, align_up(n * 64, 256) + 2 * align_up(n * 32, 256))) return r;
  Stager st(ctx.stage);
  uint8_t *dR = st.take(n * 64), *dm = st.take(n * 32), *dc = st.take(n * 32);
  H2D(dR, R_uv, n * 64);
  H2D(dm, m, n * 32);
  launch_challenge(false, (const uint8_t*)dR, (const uint8_t*)nullptr, (const uint8_t*)dm, n, dc, (uint8_t*)nullptr, 0);
  HIP_TRY(hipGetLastError());
  D2H(c, dc, n * 32);
  HIP_TRY(hipStreamSynchronize(0));
  return DSV_OK;
}
int dsv_challenge_double(const uint8_t* R_uv, const uint8_t* Rp_uv, const uint8_t* m, size_t n,
                         uint8_t* c) {
  if (n && (!R_uv || !Rp_uv || !m || !c)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_HOST_PROLOGUE(n);
  DSV_HOST_LOCK();
  if (int r = ensure_stage(ctx, 2 * align_up(n * 64, 256) + 2 * align_up(n * 32, 256))) return r;
  Stager st(ctx.stage);
  uint8_t *dR = st.take(n * 64), *dRp = st.take(n * 64), *dm = st.take(n * 32),
          *dc = st.take(n * 32);
  H2D(dR, R_uv, n * 64);
  H2D(dRp, Rp_uv, n * 64);
  H2D(dm, m, n * 32);
  launch_challenge(true, (const uint8_t*)dR, (const uint8_t*)dRp, (const uint8_t*)dm, n, dc, (uint8_t*)nullptr, 0);
  HIP_TRY(hipGetLastError());
  D2H(c, dc, n * 32);
  HIP_TRY(hipStreamSynchronize(0));
  return DSV_OK;
}


}  // extern "C"
