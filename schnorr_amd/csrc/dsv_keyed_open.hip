// dsv_keyed_open.hip — registered key sets as a key cache (include/dsv.h: dsv_verify_keyed_open*,
// dsv_verify_vargen_keyed_open*; keyed_open.h): the open-set form of verify by key value.  The
// verdicts are those of the unkeyed call on the same columns for every input; an item under a valid registered key
// is decided by the key's tables, every other item by the unkeyed equation.  Device form, one stream,
// enqueue-only: lookup, challenge hash and keyed kernel over all n (a miss gets 0 there), the list of the misses,
// the unkeyed equation over that list.  Host form: the same per chunk through the context's staging.  Single and
// double signatures through the generic call, the var-generator scheme through a call of its own (the generic
// one refuses its sets); both are one body here.
#include "keyset_host.h"

namespace dsvh {
// ---- the miss branch (keyset_host.h) ---------------------------------------------------------------------------
size_t open_miss_bytes(KeyForm form, int scheme, size_t n) {
  const size_t own = form == kKeyRecord ? (size_t)keyset_points(scheme) * align_up(n * 64, 256) : 0;
  return align_up(4 * n, 256) + 256 + var_table_bytes(n, kTablesPerLane) + own;
}
MissBranch carve_miss_branch(Stager& x, KeyForm form, int scheme, size_t n, const void* key_a, const void* key_b) {
  MissBranch b{};
  b.list = reinterpret_cast<uint32_t*>(x.take(4 * n));
  b.count = reinterpret_cast<uint32_t*>(x.take(4));
  b.tables = reinterpret_cast<uint32_t*>(x.take(var_table_bytes(n, kTablesPerLane)));
  if (form == kKeyRecord) {
    b.records = static_cast<const uint8_t*>(key_a);
    b.key_a = b.own_a = x.take(n * 64);
    b.key_b = b.own_b = keyset_points(scheme) == 2 ? x.take(n * 64) : nullptr;
  } else {
    b.key_a = static_cast<const uint8_t*>(key_a);
    b.key_b = static_cast<const uint8_t*>(key_b);
  }
  return b;
}
int enqueue_miss_branch(const Context& ctx, const Items& in, const uint32_t* idx, size_t n, uint8_t* ok,
                        const MissBranch& b, const Workspace& w, hipStream_t s) {
  HIP_TRY(launch_miss_list(idx, n, b.list, b.count, s));
  if (b.records) {
    launch_decompress_listed(keyset_points(in.scheme), b.records, n, b.list, b.count, b.own_a, b.own_b, w.valid,
                             ctx.ts_cancel, ctx.ts_hash, s);
    HIP_TRY(hipGetLastError());
  }
  if (in.scheme == 2) {
    launch_verify_var_listed(in.u, w.c, b.key_a, b.key_b, in.R(), w.valid, n, ok, b.tables, b.list, b.count, s);
    HIP_TRY(hipGetLastError());
    return DSV_OK;
  }
  const ChainOperands op0{b.key_a, in.R(), ctx.table[0]};
  const ChainOperands op1{b.key_b, in.Rp(), ctx.table[1]};
  launch_verify_listed(in.scheme == 1 ? 2 : 1, in.u, w.c, op0, op1, w.valid, n, ok, b.tables, b.list, b.count, s);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

namespace {

// vargen: the call is dsv_verify_vargen_keyed_open*, which takes var-generator sets and no others
int open_scheme_ok(int scheme, bool vargen) {
  if (vargen && scheme != 2)
    return fail(DSV_ERR_INVALID_ARGUMENT,
                "dsv_verify_vargen_keyed_open takes a var-generator key set (key set of scheme %d: "
                "dsv_verify_keyed_open)",
                scheme);
  if (!vargen && scheme == 2)
    return fail(DSV_ERR_INVALID_ARGUMENT,
                "the open-set form has no var-generator scheme (key set of scheme 2); "
                "dsv_verify_vargen_keyed_open takes such a set");
  return DSV_OK;
}

// ---- the two forms, for the generic call (vargen = false: single and double sets, key_a / key_b = PK / PK') and
// for the var-generator one (vargen = true: no second nonce point, key_a / key_b = PK / Gen) -------------------
int open_dev(bool vargen, const dsv_keyset* ks, const void* u, const void* R_uv, const void* Rp_uv,
             const void* key_a, const void* key_b, const void* m, size_t n, void* ok, void* workspace,
             size_t workspace_bytes, void* stream, void* misses) {
  if (int r = library_up(ks)) return r;
  {
    std::shared_lock<std::shared_mutex> rl(keyset_mutex());
    Context* cp = nullptr;
    if (int r = check_set(ks, -1, n, cp)) return r;
    if (int r = open_scheme_ok(ks->scheme, vargen)) return r;
  }
  // the workspace in order: idx | list | count | window tables | c | valid; run_keyed_dev checks and hands on the
  // index pointer, which is the workspace itself
  MissBranch b{};
  Items items;
  return run_keyed_dev(
      ks, -1,
      [=](int scheme) { return affine_inputs_null(scheme, u, R_uv, Rp_uv, m, key_a, key_b); },
      [=](int scheme) { return align_up(4 * n, 256) + open_miss_bytes(kKeyAffine, scheme, n); }, workspace, n, ok,
      workspace, workspace_bytes, stream,
      [&](const Context& ctx, int scheme, Stager& x, hipStream_t s, Items& in, const uint8_t*&) {
        if (int r = open_scheme_ok(scheme, vargen)) return r;  // (the handle was reused between the two locks)
        if (int r = check_key_alignment(kKeyAffine, scheme, key_a, key_b)) return r;
        if (int r = check_misses(ks, &ctx, misses)) return r;
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * n));
        b = carve_miss_branch(x, kKeyAffine, scheme, n, key_a, key_b);
        if (int r = enqueue_lookup(ks, kKeyAffine, key_a, key_b, n, idx, static_cast<uint32_t*>(misses), s)) return r;
        items = in = make_items(scheme, u, {R_uv, keyed_sig_points(scheme) == 2 ? Rp_uv : nullptr}, m);
        return (int)DSV_OK;
      },
      [&](const Context& ctx, hipStream_t s, const Workspace& w) {
        return enqueue_miss_branch(ctx, items, static_cast<const uint32_t*>(workspace), n, static_cast<uint8_t*>(ok),
                                   b, w, s);
      });
}

int open_host(bool vargen, const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
              const uint8_t* key_a, const uint8_t* key_b, const uint8_t* m, size_t n, uint8_t* ok, size_t* misses) {
  return run_by_value_host(
      ks, -1, [=](int scheme) { return open_scheme_ok(scheme, vargen); },
      [=](int scheme) { return affine_inputs_null(scheme, u, R_uv, Rp_uv, m, key_a, key_b); },
      [=](int scheme, size_t cnt) {
        return affine_chunk_bytes(scheme, cnt) + keyed_ws_bytes(cnt) + open_miss_bytes(kKeyAffine, scheme, cnt);
      },
      n, ok, 1, misses,
      [=](Context& ctx, int scheme, Stager& st, size_t off, size_t cnt, uint32_t* dmiss, const void*& dout) {
        AffineChunk c;
        if (int r = stage_affine_chunk(scheme, st, u, R_uv, Rp_uv, m, key_a, key_b, off, cnt, c)) return r;
        const MissBranch b = carve_miss_branch(st, kKeyAffine, scheme, cnt, c.key_a, c.key_b);
        void* ws = st.take(keyed_ws_bytes(cnt));
        dout = c.ok;
        if (int r = enqueue_lookup(ks, kKeyAffine, c.key_a, c.key_b, cnt, c.idx, dmiss, 0)) return r;
        enqueue_keyed(ctx, ks, c.in, c.idx, cnt, c.ok, ws, 0);
        HIP_TRY(hipGetLastError());
        return enqueue_miss_branch(ctx, c.in, c.idx, cnt, c.ok, b, carve(ws, cnt), 0);
      });
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyed_open_workspace_bytes(size_t n) {
  return align_up(4 * n, 256) + keyed_ws_bytes(n) + open_miss_bytes(kKeyAffine, 0, n);
}

int dsv_verify_keyed_open_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* Rp_uv,
                              const void* key_a, const void* key_b, const void* m, size_t n, void* ok,
                              void* workspace, size_t workspace_bytes, void* stream, void* misses) {
  return open_dev(false, ks, u, R_uv, Rp_uv, key_a, key_b, m, n, ok, workspace, workspace_bytes, stream, misses);
}
int dsv_verify_keyed_open(const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                          const uint8_t* key_a, const uint8_t* key_b, const uint8_t* m, size_t n, uint8_t* ok,
                          size_t* misses) {
  return open_host(false, ks, u, R_uv, Rp_uv, key_a, key_b, m, n, ok, misses);
}

int dsv_verify_vargen_keyed_open_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* PK_uv,
                                     const void* Gen_uv, const void* m, size_t n, void* ok, void* workspace,
                                     size_t workspace_bytes, void* stream, void* misses) {
  return open_dev(true, ks, u, R_uv, nullptr, PK_uv, Gen_uv, m, n, ok, workspace, workspace_bytes, stream, misses);
}
int dsv_verify_vargen_keyed_open(const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint8_t* PK_uv,
                                 const uint8_t* Gen_uv, const uint8_t* m, size_t n, uint8_t* ok, size_t* misses) {
  return open_host(true, ks, u, R_uv, nullptr, PK_uv, Gen_uv, m, n, ok, misses);
}

}  // extern "C"
