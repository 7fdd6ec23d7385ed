// dsv_device.hip — the device-pointer entry points of include/dsv.h: challenge hash, the three verify
// schemes over affine inputs resident in HBM (`PublicKey::verify`, `PublicKeyDouble::verify`,
// `PublicKeyVarGen::verify`, /root/reference/src/keys/public.rs:121-130, :222-244, :401-415) over affine
// points, projective points or Montgomery limbs, the second stage alone, and mixed single + double batches
// (device-side split by kind).  The body verify_on is what the host pipeline and the other units call per
// sub-batch.
#include "dsv_host.h"

namespace dsvh {
// bodies shared by the device-pointer entry points and the host pipeline (context resolved)
// Small batches (eight-lane kernel): the window tables of (PK, R) do not depend on the challenge, so
// they are built on one of the lane's internal streams WHILE k_challenge runs on the caller's: fork
// by an event here; the caller enqueues the hash, then waits for the returned join event on its own
// stream in front of the verify kernel.  nullptr: not a small batch (or the overlap is off, or no
// lane could be had) — the verify kernel then builds its tables itself.
thread_local bool t_pipeline_part = false;
thread_local size_t t_chunk_first = 0;
hipEvent_t prep_tables_beside_hash(Context& ctx, const void* PK_uv, const void* R_uv, size_t n,
                                   u32* tables, hipStream_t user) {
  if (!(ctx.quad && ctx.small_overlap && n <= kQuadMaxItems) || t_pipeline_part) return nullptr;
  SplitLane* lane = nullptr;
  if (acquire_lane(ctx, user, lane) != DSV_OK) return nullptr;
  std::lock_guard<std::mutex> lk(ctx.lane_mu);
  if (hipEventRecord(lane->fork, user) != hipSuccess ||
      hipStreamWaitEvent(lane->side, lane->fork, 0) != hipSuccess)
    return nullptr;
  launch_prep_var_tables((const uint8_t*)PK_uv, (const uint8_t*)R_uv, n, tables, lane->side);
  if (hipEventRecord(lane->side_join, lane->side) != hipSuccess) {
    // the prep kernel is already writing this call's table slots: it must have finished before the
    // verify kernel, told to build its tables itself, writes the same slots from the caller's stream
    (void)hipStreamSynchronize(lane->side);
    return nullptr;
  }
  return lane->side_join;
}
void launch_hash(const Items& in, size_t n, uint8_t* c, uint8_t* valid, hipStream_t s, const uint8_t* valid_in) {
  launch_challenge(in.Rp() != nullptr, in.R(), in.Rp(), in.m, n, c, valid, s, valid_in);
}
void launch_verify(const Context& ctx, const Items& in, const uint8_t* c, const uint8_t* valid, size_t n,
                   uint8_t* ok, u32* tables, hipStream_t s, bool prebuilt, const u32* gate) {
  if (in.scheme == 0)
    launch_verify_fixed(ctx, false, in.u, c, in.PK(), in.R(), 0, valid, n, ok, tables, s, prebuilt, gate);
  else if (in.scheme == 1)
    launch_verify_fixed_double(ctx, in.u, c, in.PK(), in.R(), in.PKp(), in.Rp(), valid, n, ok, tables, s, prebuilt,
                               gate);
  else  // (no tables to prebuild: k_vargen builds its own)
    launch_verify_var(in.u, c, in.PK(), in.Gen(), in.R(), valid, n, ok, tables, s, gate);
}
int verify_on(Context& ctx, const Items& in, size_t n, void* ok, void* workspace, hipStream_t stream,
              const uint8_t* valid_in) {
  uint8_t* pok = (uint8_t*)ok;
  Context* cp = &ctx;
  return run_split(ctx, n, workspace, stream, [=](size_t off, size_t cnt, const Workspace& w, hipStream_t s) {
    const Items at = in.at(off);
    // (only for an unsplit call: inside run_split's loop the lane lock is held and cnt > 2^14 anyway,
    //  except for a short last part, which simply builds its tables in the kernel)
    hipEvent_t ready = layout(in.scheme).fixed && cnt == n
                           ? prep_tables_beside_hash(*cp, at.PK(), at.R(), cnt, w.tables, s)
                           : nullptr;
    launch_hash(at, cnt, w.c, w.valid, s, valid_in ? valid_in + off : nullptr);
    if (ready && hipStreamWaitEvent(s, ready, 0) != hipSuccess) return;  // (surfaces through hipGetLastError)
    launch_verify(*cp, at, w.c, w.valid, cnt, pok + off, w.tables, s, ready != nullptr);
  });
}
void normalize_on(int scheme, const uint8_t* const* in, uint8_t* const* out, size_t n, uint8_t* valid, u32* prefix,
                  hipStream_t s, const uint8_t* u_mont, const uint8_t* m_mont, uint8_t* u_out, uint8_t* m_out,
                  int per_lane, int block) {
  const int np = layout(scheme).points;
  NormalizeArgs a = {};
  for (int k = 0; k < np; k++) {
    a.in[k] = in[k];
    a.out[k] = out[k];
  }
  if (u_mont) {
    a.u_mont = u_mont;
    a.m_mont = m_mont;
    a.u_out = u_out;
    a.m_out = m_out;
  }
  launch_normalize_uvz(a, np, n, valid, prefix, s, per_lane, block);
}
int decompress_on(Context& ctx, const void* in, size_t in_stride, size_t n, void* out_uv, void* ok,
                  int accumulate, hipStream_t stream) {
  if (!in || !out_uv || !ok || in_stride < 32 || (in_stride & 15) || ((uintptr_t)in & 15))
    return fail(DSV_ERR_INVALID_ARGUMENT, "bad pointer / stride (need 16-byte alignment)");
  launch_decompress((const uint8_t*)in, in_stride, n, (uint8_t*)out_uv, (uint8_t*)ok, accumulate, ctx.ts_cancel, ctx.ts_hash, stream);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

// ---- projective inputs / Montgomery limbs resident in HBM (dsv_host.hip: what they are) ----------
namespace {
struct ExtWs {
  uint8_t* pts[4];
  uint8_t* valid;
  u32* prefix;
  void* vws;
};
size_t ext_workspace_bytes(size_t n) {
  return 4 * align_up(n * 64, 256) + align_up(n, 256) + align_up(normalize_prefix_bytes(n, 4), 256) +
         align_up(dsv_workspace_bytes(n), 256) + 256;
}
size_t mont_workspace_bytes(size_t n) { return 2 * align_up(n * 32, 256) + ext_workspace_bytes(n); }
ExtWs carve_ext(void* ws, size_t n) {
  Stager st(static_cast<uint8_t*>(ws));
  ExtWs w;
  for (int k = 0; k < 4; k++) w.pts[k] = st.take(n * 64);
  w.valid = st.take(n);
  w.prefix = reinterpret_cast<u32*>(st.take(normalize_prefix_bytes(n, 4)));
  w.vws = st.take(dsv_workspace_bytes(n));
  return w;
}
// in.pt: the scheme's points, each n x 96 B (u || v || z).  kMont: in.u / in.m are Montgomery limbs,
// converted by the normalisation kernel into two arrays carved in front of the ext workspace
int verify_ext_on(Context& ctx, int form, const Items& in, size_t n, void* ok, void* workspace, hipStream_t s) {
  Stager st(static_cast<uint8_t*>(workspace));
  Items aff = in;
  uint8_t *cu = nullptr, *cm = nullptr;
  if (form == kMont) {
    cu = st.take(n * 32), cm = st.take(n * 32);
    aff.u = cu, aff.m = cm;
  }
  const ExtWs w = carve_ext(st.take(0), n);
  normalize_on(in.scheme, in.pt, w.pts, n, w.valid, w.prefix, s, cu ? in.u : nullptr, in.m, cu, cm);
  for (int k = 0; k < 4; k++) aff.pt[k] = in.pt[k] ? w.pts[k] : nullptr;
  if (int rc = verify_on(ctx, aff, n, ok, w.vws, s, w.valid)) return rc;
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}
// the verify entry points over device pointers: affine (u, points, m), projective or Montgomery limbs
int verify_dev(int form, const Items& in, size_t n, void* ok, void* workspace, void* stream) {
  if (n && (in.any_null() || !ok || !workspace)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_DEV_PROLOGUE(n, ok);
  if (form == kAffine) return verify_on(ctx, in, n, ok, workspace, (hipStream_t)stream);
  return verify_ext_on(ctx, form, in, n, ok, workspace, (hipStream_t)stream);
}
}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

int dsv_challenge_single_dev(const void* R_uv, const void* m, size_t n, void* c, void* valid,
                             void* stream) {
  if (n && (!R_uv || !m || !c)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_DEV_PROLOGUE(n, c);
  launch_challenge(false, (const uint8_t*)R_uv, (const uint8_t*)nullptr, (const uint8_t*)m, n, (uint8_t*)c, (uint8_t*)valid, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}
int dsv_challenge_double_dev(const void* R_uv, const void* Rp_uv, const void* m, size_t n, void* c,
                             void* valid, void* stream) {
  if (n && (!R_uv || !Rp_uv || !m || !c)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_DEV_PROLOGUE(n, c);
  launch_challenge(true, (const uint8_t*)R_uv, (const uint8_t*)Rp_uv, (const uint8_t*)m, n, (uint8_t*)c, (uint8_t*)valid, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}


int dsv_verify_single_dev(const void* u, const void* R_uv, const void* PK_uv, const void* m,
                          size_t n, void* ok, void* workspace, void* stream) {
  return verify_dev(kAffine, make_items(0, u, {R_uv, PK_uv}, m), n, ok, workspace, stream);
}
int dsv_verify_double_dev(const void* u, const void* R_uv, const void* Rp_uv, const void* PK_uv,
                          const void* PKp_uv, const void* m, size_t n, void* ok, void* workspace,
                          void* stream) {
  return verify_dev(kAffine, make_items(1, u, {R_uv, Rp_uv, PK_uv, PKp_uv}, m), n, ok, workspace, stream);
}
int dsv_verify_vargen_dev(const void* u, const void* R_uv, const void* PK_uv, const void* Gen_uv,
                          const void* m, size_t n, void* ok, void* workspace, void* stream) {
  return verify_dev(kAffine, make_items(2, u, {R_uv, PK_uv, Gen_uv}, m), n, ok, workspace, stream);
}

// projective points (u || v || z, 96 B): the device does to_hash_inputs first
size_t dsv_ext_workspace_bytes(size_t n) { return ext_workspace_bytes(n); }
int dsv_verify_single_ext_dev(const void* u, const void* R_uvz, const void* PK_uvz, const void* m,
                              size_t n, void* ok, void* workspace, void* stream) {
  return verify_dev(kExt, make_items(0, u, {R_uvz, PK_uvz}, m), n, ok, workspace, stream);
}
int dsv_verify_double_ext_dev(const void* u, const void* R_uvz, const void* Rp_uvz, const void* PK_uvz,
                              const void* PKp_uvz, const void* m, size_t n, void* ok, void* workspace,
                              void* stream) {
  return verify_dev(kExt, make_items(1, u, {R_uvz, Rp_uvz, PK_uvz, PKp_uvz}, m), n, ok, workspace, stream);
}
int dsv_verify_vargen_ext_dev(const void* u, const void* R_uvz, const void* PK_uvz, const void* Gen_uvz,
                              const void* m, size_t n, void* ok, void* workspace, void* stream) {
  return verify_dev(kExt, make_items(2, u, {R_uvz, PK_uvz, Gen_uvz}, m), n, ok, workspace, stream);
}

// Montgomery limbs (the Rust types' in-memory form) resident in HBM
size_t dsv_mont_workspace_bytes(size_t n) { return mont_workspace_bytes(n); }
int dsv_verify_single_mont_dev(const void* u, const void* R_uvz, const void* PK_uvz, const void* m,
                               size_t n, void* ok, void* workspace, void* stream) {
  return verify_dev(kMont, make_items(0, u, {R_uvz, PK_uvz}, m), n, ok, workspace, stream);
}
int dsv_verify_double_mont_dev(const void* u, const void* R_uvz, const void* Rp_uvz, const void* PK_uvz,
                               const void* PKp_uvz, const void* m, size_t n, void* ok, void* workspace,
                               void* stream) {
  return verify_dev(kMont, make_items(1, u, {R_uvz, Rp_uvz, PK_uvz, PKp_uvz}, m), n, ok, workspace, stream);
}
int dsv_verify_vargen_mont_dev(const void* u, const void* R_uvz, const void* PK_uvz, const void* Gen_uvz,
                               const void* m, size_t n, void* ok, void* workspace, void* stream) {
  return verify_dev(kMont, make_items(2, u, {R_uvz, PK_uvz, Gen_uvz}, m), n, ok, workspace, stream);
}

// second stage alone (c and valid already computed): lets callers time / profile the dominant
// kernel separately, and re-use one challenge for several key pairs
int dsv_verify_core_dev(const void* u, const void* c, const void* valid, const void* PK_uv,
                        const void* R_uv, int which, int accumulate, size_t n, void* ok,
                        void* workspace, void* stream) {
  if (n && (!u || !c || !valid || !PK_uv || !R_uv || !ok || !workspace || which < 0 || which > 1))
    return fail(DSV_ERR_INVALID_ARGUMENT, "bad argument");
  DSV_DEV_PROLOGUE(n, ok);
  Workspace w = carve(workspace, n);
  launch_verify_fixed(ctx, accumulate != 0, u, c, PK_uv, R_uv, which, valid, n, ok, w.tables,
                      (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}
// both equations of a double signature from a precomputed challenge, one launch
int dsv_verify_core_double_dev(const void* u, const void* c, const void* valid, const void* PK_uv,
                               const void* R_uv, const void* PKp_uv, const void* Rp_uv, size_t n,
                               void* ok, void* workspace, void* stream) {
  if (n && (!u || !c || !valid || !PK_uv || !R_uv || !PKp_uv || !Rp_uv || !ok || !workspace))
    return fail(DSV_ERR_INVALID_ARGUMENT, "bad argument");
  DSV_DEV_PROLOGUE(n, ok);
  Workspace w = carve(workspace, n);
  launch_verify_fixed_double(ctx, u, c, PK_uv, R_uv, PKp_uv, Rp_uv, valid, n, ok, w.tables,
                             (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

// ---- mixed batches: device-side split by kind ---------------------------------------------
namespace {
struct SplitScratch {
  u32* tile_counts;
  u32* totals;
};
size_t split_scratch_bytes(size_t n) {
  const size_t tiles = (n + kSplitTile - 1) / kSplitTile;
  return align_up(tiles * 8, 256) + 256;
}
SplitScratch carve_split(void* p, size_t n) {
  const size_t tiles = (n + kSplitTile - 1) / kSplitTile;
  SplitScratch s;
  s.tile_counts = static_cast<u32*>(p);
  s.totals = reinterpret_cast<u32*>(static_cast<uint8_t*>(p) + align_up(tiles * 8, 256));
  return s;
}
int split_on(const void* kinds, size_t n, void* idx_single, size_t cap_single, void* idx_double,
             size_t cap_double, void* scratch, hipStream_t s) {
  if ((uintptr_t)kinds & 15) return fail(DSV_ERR_INVALID_ARGUMENT, "kinds must be 16-byte aligned");
  SplitScratch sc = carve_split(scratch, n);
  launch_split_kinds((const uint8_t*)kinds, n, sc.tile_counts, sc.totals, (u32*)idx_single, cap_single,
                     (u32*)idx_double, cap_double, s);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}
// limit (device u32, may be null): only min(count, *limit) index entries are dereferenced
int gather_on(const void* src, size_t src_rows, size_t row_bytes, const void* idx, size_t count,
              const void* limit, void* dst, hipStream_t s) {
  if (row_bytes == 0 || (row_bytes & 15) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
    return fail(DSV_ERR_INVALID_ARGUMENT, "rows must be multiples of 16 bytes, 16-byte aligned");
  if (count == 0) return DSV_OK;
  launch_gather_rows(src, src_rows, (u32)(row_bytes / 16), (const u32*)idx, count, (const u32*)limit, dst, s);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}
}  // namespace

size_t dsv_split_scratch_bytes(size_t n) { return split_scratch_bytes(n); }

int dsv_split_kinds_dev(const void* kinds, size_t n, void* idx_single, size_t cap_single,
                        void* idx_double, size_t cap_double, void* scratch, void* stream) {
  if (n && (!kinds || !idx_single || !idx_double || !scratch))
    return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_DEV_PROLOGUE(n, scratch);
  return split_on(kinds, n, idx_single, cap_single, idx_double, cap_double, scratch, (hipStream_t)stream);
}
int dsv_gather_rows_dev(const void* src, size_t src_rows, size_t row_bytes, const void* idx,
                        size_t count, const void* count_limit, void* dst, void* stream) {
  if (count && (!src || !idx || !dst)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_DEV_PROLOGUE(count, dst);
  return gather_on(src, src_rows, row_bytes, idx, count, count_limit, dst, (hipStream_t)stream);
}
int dsv_scatter_verdicts_dev(const void* src, const void* idx, size_t count, const void* count_limit,
                             void* dst, size_t dst_len, void* stream) {
  if (count && (!src || !idx || !dst)) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_DEV_PROLOGUE(count, dst);
  launch_scatter_bytes((const uint8_t*)src, (const u32*)idx, count, (const u32*)count_limit, (uint8_t*)dst,
                       dst_len, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

size_t dsv_mixed_workspace_bytes(size_t n) {
  // split scratch | idx_single[n] | idx_double[n] | compacted rows (<= 320 B per item) |
  // per-kind verdicts | verify workspace
  return split_scratch_bytes(n) + 2 * align_up(n * 4, 256) + 6 * align_up(n * 64, 256) +
         2 * align_up(n, 256) + align_up(dsv_workspace_bytes(n), 256) + 256;
}

// One batch holding single (kind 0) and double (kind 1) signatures in any interleaving, as a
// structure of arrays over ALL n items (Rp_uv / PKp_uv rows of single items are ignored).
// n_double = number of kind-1 items (the caller knows its batch); every other item must be kind 0.
extern "C++" {
namespace {
// fast: both kinds' groups through the batch fast accept (verify_rlc_on: enqueue-only); *accepted =
// every group of both kinds was decided by its aggregates
int verify_mixed_dev(const void* kinds, const void* u, const void* R_uv, const void* Rp_uv, const void* PK_uv,
                     const void* PKp_uv, const void* m, size_t n, size_t n_double, void* ok, void* workspace,
                     void* stream, bool fast, int* accepted) {
  hipStream_t s = (hipStream_t)stream;
  if (fast)
    if (int r = refuse_capture(s, "the fast accept")) return r;
  if (n == 0 || !fast) {
    if (int r = rlc_clear_accepted(accepted)) return r;
  }
  if (n && (!kinds || !u || !R_uv || !Rp_uv || !PK_uv || !PKp_uv || !m || !ok || !workspace))
    return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  if (n_double > n) return fail(DSV_ERR_INVALID_ARGUMENT, "n_double exceeds n");
  DSV_DEV_PROLOGUE(n, ok);
  RlcVerdictTarget vt;
  if (fast)
    if (int r = rlc_verdict_target(ctx, accepted, vt)) return r;
  const size_t ns = n - n_double, nd = n_double;
  Stager st(static_cast<uint8_t*>(workspace));
  void* scratch = st.take(split_scratch_bytes(n));
  u32* idx_s = reinterpret_cast<u32*>(st.take(n * 4));
  u32* idx_d = reinterpret_cast<u32*>(st.take(n * 4));
  uint8_t *cu = st.take(n * 32), *cm = st.take(n * 32);   // singles first, doubles behind them
  uint8_t *cR = st.take(n * 64), *cPK = st.take(n * 64);
  uint8_t *cRp = st.take(n * 64), *cPKp = st.take(n * 64);  // doubles only
  uint8_t *oks = st.take(n), *okd = st.take(n);
  void* vws = st.take(fast ? dsv_rlc_workspace_bytes(n, 0) : dsv_workspace_bytes(n));
  HIP_TRY(hipMemsetAsync(ok, 0, n, s));  // items of an invalid kind keep verdict 0
  if (int r = split_on(kinds, n, idx_s, ns, idx_d, nd, scratch, s)) return r;
  // Only index entries the split really wrote are dereferenced: every gather / scatter is bounded
  // on the device by the split's own totals (and skips an index >= n), whatever the caller
  // declared.  With a wrong n_double the compacted rows are partly stale workspace bytes — the
  // verify kernels take any bytes (out-of-contract inputs never fault) and k_mixed_check zeroes
  // the whole verdict vector at the end.
  const u32* totals = carve_split(scratch, n).totals;
  struct Col { const void* src; size_t bytes; uint8_t* dst; };
  const Col single_cols[4] = {{u, 32, cu}, {m, 32, cm}, {R_uv, 64, cR}, {PK_uv, 64, cPK}};
  for (const Col& c : single_cols)
    if (int r = gather_on(c.src, n, c.bytes, idx_s, ns, totals, c.dst, s)) return r;
  const Col double_cols[6] = {{u, 32, cu + ns * 32},      {m, 32, cm + ns * 32},
                              {R_uv, 64, cR + ns * 64},   {PK_uv, 64, cPK + ns * 64},
                              {Rp_uv, 64, cRp},           {PKp_uv, 64, cPKp}};
  for (const Col& c : double_cols)
    if (int r = gather_on(c.src, n, c.bytes, idx_d, nd, totals + 1, c.dst, s)) return r;
  if (ns) {
    const Items in = make_items(0, cu, {cR, cPK}, cm);
    if (int r = fast ? verify_rlc_on(ctx, in, ns, oks, vws, s, 0, vt.dev) : verify_on(ctx, in, ns, oks, vws, s)) return r;
    launch_scatter_bytes(oks, idx_s, ns, totals, (uint8_t*)ok, n, s);
  }
  if (nd) {
    const Items in = make_items(1, cu + ns * 32, {cR + ns * 64, cRp, cPK + ns * 64, cPKp}, cm + ns * 32);
    if (int r = fast ? verify_rlc_on(ctx, in, nd, okd, vws, s, 0, vt.dev, /*and_into*/ ns != 0)
                     : verify_on(ctx, in, nd, okd, vws, s))
      return r;
    launch_scatter_bytes(okd, idx_d, nd, totals + 1, (uint8_t*)ok, n, s);
  }
  launch_mixed_check(totals, (u32)ns, (u32)nd, (uint8_t*)ok, n, s);
  HIP_TRY(hipGetLastError());
  return fast ? rlc_verdict_wait(vt, s) : (int)DSV_OK;
}
}  // namespace
}  // extern "C++"
int dsv_verify_mixed_dev(const void* kinds, const void* u, const void* R_uv, const void* Rp_uv,
                         const void* PK_uv, const void* PKp_uv, const void* m, size_t n,
                         size_t n_double, void* ok, void* workspace, void* stream) {
  return verify_mixed_dev(kinds, u, R_uv, Rp_uv, PK_uv, PKp_uv, m, n, n_double, ok, workspace, stream, false, nullptr);
}
// the same with each kind's items through the batch fast accept (a wrong n_double: every verdict 0, as above)
size_t dsv_mixed_rlc_workspace_bytes(size_t n) {
  return dsv_mixed_workspace_bytes(n) - align_up(dsv_workspace_bytes(n), 256) + align_up(dsv_rlc_workspace_bytes(n, 0), 256);
}
int dsv_verify_mixed_rlc_dev(const void* kinds, const void* u, const void* R_uv, const void* Rp_uv,
                             const void* PK_uv, const void* PKp_uv, const void* m, size_t n, size_t n_double,
                             void* ok, void* workspace, void* stream, int* accepted) {
  return verify_mixed_dev(kinds, u, R_uv, Rp_uv, PK_uv, PKp_uv, m, n, n_double, ok, workspace, stream, true, accepted);
}

}  // extern "C"
