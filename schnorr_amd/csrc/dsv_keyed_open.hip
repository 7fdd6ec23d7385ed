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

// the miss branch's part of the workspace: list | count | per-lane window tables
size_t open_miss_bytes(size_t n) { return align_up(4 * n, 256) + 256 + var_table_bytes(n, kTablesPerLane); }
struct MissBranch {
  uint32_t *list, *count, *tables;
};
MissBranch carve_miss_branch(Stager& x, size_t n) {
  MissBranch b;
  b.list = reinterpret_cast<uint32_t*>(x.take(4 * n));
  b.count = reinterpret_cast<uint32_t*>(x.take(4));
  b.tables = reinterpret_cast<uint32_t*>(x.take(var_table_bytes(n, kTablesPerLane)));
  return b;
}
// behind the keyed kernel on s: the misses of idx are listed and decided by the unkeyed equation from the c /
// valid the challenge hash left in w; in: the keyed call's items, key_a / key_b: the items' own key columns (the
// var-generator scheme: PK / Gen, one three-base chain)
int enqueue_miss_branch(const Context& ctx, const Items& in, const void* key_a, const void* key_b,
                        const uint32_t* idx, size_t n, uint8_t* ok, const MissBranch& b, const Workspace& w,
                        hipStream_t s) {
  HIP_TRY(launch_miss_list(idx, n, b.list, b.count, s));
  if (in.scheme == 2) {
    launch_verify_var_listed(in.u, w.c, static_cast<const uint8_t*>(key_a), static_cast<const uint8_t*>(key_b), in.R(),
                             w.valid, n, ok, b.tables, b.list, b.count, s);
    HIP_TRY(hipGetLastError());
    return DSV_OK;
  }
  const ChainOperands op0{static_cast<const uint8_t*>(key_a), in.R(), ctx.table[0]};
  const ChainOperands op1{static_cast<const uint8_t*>(key_b), in.Rp(), ctx.table[1]};
  launch_verify_listed(in.scheme == 1 ? 2 : 1, in.u, w.c, op0, op1, w.valid, n, ok, b.tables, b.list, b.count, s);
  HIP_TRY(hipGetLastError());
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
      [=](int scheme) {
        return !u || !R_uv || (keyed_sig_points(scheme) == 2 && !Rp_uv) || !m || keys_null(scheme, key_a, key_b);
      },
      [=](int) { return align_up(4 * n, 256) + open_miss_bytes(n); }, workspace, n, ok, workspace, workspace_bytes,
      stream,
      [&](const Context& ctx, int scheme, Stager& x, hipStream_t s, Items& in, const uint8_t*&) {
        if (int r = open_scheme_ok(scheme, vargen)) return r;  // (the handle was reused between the two locks)
        if (int r = check_key_alignment(scheme, key_a, key_b)) return r;
        if (int r = check_misses(ks, &ctx, misses)) return r;
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * n));
        b = carve_miss_branch(x, n);
        if (int r = enqueue_lookup(ks, key_a, key_b, n, idx, static_cast<uint32_t*>(misses), s)) return r;
        items = in = make_items(scheme, u, {R_uv, keyed_sig_points(scheme) == 2 ? Rp_uv : nullptr}, m);
        return (int)DSV_OK;
      },
      [&](const Context& ctx, hipStream_t s, const Workspace& w) {
        return enqueue_miss_branch(ctx, items, key_a, key_b, static_cast<const uint32_t*>(workspace), n,
                                   static_cast<uint8_t*>(ok), b, w, s);
      });
}

int open_host(bool vargen, const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
              const uint8_t* key_a, const uint8_t* key_b, const uint8_t* m, size_t n, uint8_t* ok, size_t* misses) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (int r = open_scheme_ok(ks->scheme, vargen)) return r;
  if (n == 0) {
    if (misses) *misses = 0;
    return DSV_OK;
  }
  // nonce-point and key columns: 1 + 1, 2 + 2, and 1 + 2 for the var-generator scheme
  const int scheme = ks->scheme, ns = keyed_sig_points(scheme), np = keyset_points(scheme);
  if (!u || !R_uv || (ns == 2 && !Rp_uv) || !m || keys_null(scheme, key_a, key_b) || !ok)
    return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const size_t chunk = n < kLookupHostChunk ? n : kLookupHostChunk;
  const size_t per_item = 32 + 32 + 4 + 1 + 64 * (size_t)(ns + np);
  if (int r = ensure_stage(ctx, chunk * per_item + keyed_ws_bytes(chunk) + open_miss_bytes(chunk) + 12 * 256))
    return r;
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
    const MissBranch b = carve_miss_branch(st, cnt);
    void* ws = st.take(keyed_ws_bytes(cnt));
    H2D(du, u + off * 32, cnt * 32);
    H2D(dm, m + off * 32, cnt * 32);
    H2D(dR, R_uv + off * 64, cnt * 64);
    if (dRp) H2D(dRp, Rp_uv + off * 64, cnt * 64);
    H2D(da, key_a + off * 64, cnt * 64);
    if (db) H2D(db, key_b + off * 64, cnt * 64);
    if (int r = enqueue_lookup(ks, da, db, cnt, di, dmiss, 0)) return r;
    const Items in = make_items(scheme, du, {dR, dRp}, dm);
    enqueue_keyed(ctx, ks, in, di, cnt, dok, ws, 0);
    HIP_TRY(hipGetLastError());
    if (int r = enqueue_miss_branch(ctx, in, da, db, di, cnt, dok, b, carve(ws, cnt), 0)) return r;
    uint32_t missed = 0;
    D2H(ok + off, dok, cnt);
    D2H(&missed, dmiss, 4);
    HIP_TRY(hipStreamSynchronize(0));
    total += missed;
  }
  if (misses) *misses = total;
  return DSV_OK;
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyed_open_workspace_bytes(size_t n) {
  return align_up(4 * n, 256) + keyed_ws_bytes(n) + open_miss_bytes(n);
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
