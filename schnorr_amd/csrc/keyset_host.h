// keyset_host.h — what the host units know about a registered key set (keyed.h: the tables): the handle,
// the registry's lock and checks (dsv_keyset.hip), what a keyed call reads of its items.
#pragma once
#include <memory>
#include <mutex>
#include <shared_mutex>

#include "dsv_host.h"
#include "keyed_lookup.h"
#include "keyed_open.h"
#include "keyed_open_wire.h"
#include "keyed_wire.h"

// Everything but k is fixed when the set is created: the allocations are sized for `capacity` keys and never
// move.  k is read under the registry's shared lock and raised by dsv_keyset_append under the exclusive one, so a
// call that holds the shared lock sees one k from its first check to its last launch.  The bytes of registered keys
// change only under the exclusive lock, on a device that has run dry (dsv_keyset_replace).
struct dsv_keyset {
  int scheme = 0;
  size_t k = 0;         // keys registered
  size_t capacity = 0;  // keys the allocations hold (the plain constructors: k)
  int device = -1;
  size_t bytes = 0;     // of the table allocation: keyset_total_bytes(scheme, capacity)
  uint32_t* tables = nullptr;  // one allocation: the tables, then key_ok
  uint8_t* key_ok = nullptr;   // behind keyset_table_bytes(scheme, capacity)
  // the indices over the set's own keys (keyed_lookup.h), by KeyForm — affine bytes, compressed records — an
  // allocation each: the rows for `capacity` keys, then the slots; both have keyset_index_cap(capacity) slots
  struct KeyIndex {
    uint8_t* rows = nullptr;
    uint32_t* slots = nullptr;
  };
  KeyIndex index[dsv::kKeyForms];
  size_t slot_mask = 0;  // keyset_index_cap(capacity) - 1
  bool alive = false;
  // one appender at a time per set (shared with the appender: it outlives a handle destroyed under a waiting one)
  std::shared_ptr<std::mutex> append_mu = std::make_shared<std::mutex>();
};

namespace dsvh {

// A keyed call's items are make_items(scheme, u, {R[, R']}, m): the signature's points in their canonical slots,
// the key slots (PK, PK', Gen) null — the keys come from the set.
inline bool keyed_any_null(const Items& in) { return !in.u || !in.R() || (in.scheme == 1 && !in.Rp()) || !in.m; }

inline size_t keyed_ws_bytes(size_t n) { return align_up(n * 32, 256) + align_up(n, 256); }
// live key sets: verify calls read under the shared lock, create / destroy / shutdown write under the exclusive one
std::shared_mutex& keyset_mutex();
// (shared lock held) n is in range; ks is live, of `scheme` (negative: whatever the set's own is), on an
// initialised device: ctx = its context
int check_set(const dsv_keyset* ks, int scheme, size_t n, Context*& ctx);
// (shared lock held, check_set passed, n > 0) the rest of a keyed _dev call's checks, in this order: null
// pointers, the window bits (0 for the per-signature forms), workspace_bytes >= need, `ok` on the set's device
// (ctx: the set's context)
// inputs_null: one of the call's input pointers other than idx is null (affine items: keyed_any_null; the wire
// form: the records or m)
int check_keyed_dev(const dsv_keyset* ks, const Context* ctx, bool inputs_null, const void* idx, const void* ok,
                    const void* workspace, size_t workspace_bytes, int window_bits, size_t need);
// challenge hash, then the keyed kernel; every pointer device memory of ctx's device
// valid_in (may be null): per-item bytes of an earlier stage (the wire form's decoder), AND-ed in by the hash
void enqueue_keyed(const Context& ctx, const dsv_keyset* ks, const Items& in, const uint32_t* idx, size_t n,
                   uint8_t* ok, void* workspace, hipStream_t s, const uint8_t* valid_in = nullptr);

// The body of the per-signature keyed _dev calls (affine, wire, typed objects), enqueue-only on `stream` under the
// registry's shared lock.  scheme: the entry point's, or negative for the set's own.  A form supplies
//   inputs_null(scheme)   one of its input pointers other than idx is null,
//   cols_bytes(scheme)    the workspace bytes of its preparation step, in front of keyed_ws_bytes(n),
//   prep(ctx, scheme, x, s, in, valid_in)   carves those bytes from x, enqueues the preparation launch on s, and
//                         leaves the keyed call's items and the per-item verdicts its hash ANDs in (null: none);
//                         a non-zero return ends the call with nothing more enqueued.
//   after(ctx, s, w)      (optional) enqueues on s what follows the keyed kernel; w: the c / valid the challenge
//                         hash wrote (the open-set form's miss branch reads them).
template <class Null, class Bytes, class Prep, class After>
int run_keyed_dev(const dsv_keyset* ks, int scheme, Null inputs_null, Bytes cols_bytes, const void* idx, size_t n,
                  void* ok, void* workspace, size_t workspace_bytes, void* stream, Prep prep, After after) {
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, scheme, n, cp)) return r;
  if (n == 0) return DSV_OK;
  scheme = ks->scheme;
  if (int r = check_keyed_dev(ks, cp, inputs_null(scheme), idx, ok, workspace, workspace_bytes, 0,
                              cols_bytes(scheme) + keyed_ws_bytes(n)))
    return r;
  Context& ctx = *cp;
  DSV_ON_DEVICE(ctx);
  const hipStream_t s = (hipStream_t)stream;
  Stager x(static_cast<uint8_t*>(workspace));
  Items in;
  const uint8_t* valid_in = nullptr;
  if (int r = prep(ctx, scheme, x, s, in, valid_in)) return r;
  void* keyed_ws = x.take(keyed_ws_bytes(n));
  enqueue_keyed(ctx, ks, in, (const uint32_t*)idx, n, (uint8_t*)ok, keyed_ws, s, valid_in);
  HIP_TRY(hipGetLastError());
  return after(ctx, s, carve(keyed_ws, n));
}
template <class Null, class Bytes, class Prep>
int run_keyed_dev(const dsv_keyset* ks, int scheme, Null inputs_null, Bytes cols_bytes, const void* idx, size_t n,
                  void* ok, void* workspace, size_t workspace_bytes, void* stream, Prep prep) {
  return run_keyed_dev(ks, scheme, inputs_null, cols_bytes, idx, n, ok, workspace, workspace_bytes, stream, prep,
                       [](const Context&, hipStream_t, const Workspace&) { return (int)DSV_OK; });
}

// One key form (affine host bytes, wire records, typed objects) for m keys, as the constructors and the appends
// hand it to the one body that registers keys (dsv_keyset.hip):
//   check_pointers()   the form's own argument checks (m > 0 only),
//   own_bytes          device scratch of the form's, behind the affine points,
//   stage(ctx, P, own, s, valid)   brings the m keys' affine points to P (point p of key j at p * m * 64 + j * 64)
//                      on stream s, working in `own`; valid = the per-key verdicts of its decoding for the table
//                      build to AND in (left null: none).
// The form may hold host buffers of its own for the transfer: it lives until the call returns, behind the
// stream's synchronisation.
using KeysetStage = std::function<int(Context& ctx, uint8_t* P, uint8_t* own, hipStream_t s, uint8_t*& valid)>;
struct KeysetForm {
  std::function<int()> check_pointers;
  size_t own_bytes;
  KeysetStage stage;
};
// One constructor call, on the calling thread's current device: the checks in this order — null `out`, unknown
// scheme, k > 2^32 - 1 (reserved: capacity < k, capacity > 2^32 - 2), then for k > 0 the form's own
// check_pointers() — then both allocations for `capacity` keys, and the k keys appended to the empty set by the
// body dsv_keyset_append runs; blocks, registers the set, *out = its handle.
// reserved: dsv_keyset_create_reserved (the plain constructors pass capacity = k).
int create_keyset(int scheme, size_t k, size_t capacity, bool reserved, dsv_keyset** out, const KeysetForm& form);
// dsv_keyset_append*: m more keys of the form form_of(the set's scheme) into a live set, in place, on a stream of
// its own; blocks.  *first_index (may be null) = the index of the first of them.
int append_keyset(dsv_keyset* ks, size_t m, uint32_t* first_index,
                  const std::function<KeysetForm(int scheme)>& form_of);
// dsv_keyset_replace*: the m keys of the form form_of(the set's scheme) take the places indices[0 .. m - 1] (host
// array, pairwise distinct, each below k) of a live set, in place; blocks.  Two phases: under the
// registry's shared lock the keys are staged and their tables built into a scratch of the call's own, on a stream of
// its own, beside the verify calls; under the exclusive lock, after a device-wide wait, one kernel scatters the
// scratch into the set and both indices are rebuilt from the set's own rows in the canonical layout.  Serialised
// with the appends to the set (append_mu).  A HIP failure in the second phase leaves the set dead.
int replace_keyset(dsv_keyset* ks, const uint32_t* indices, size_t m,
                   const std::function<KeysetForm(int scheme)>& form_of);
// the three forms over m keys
KeysetForm keyset_form_affine(int scheme, const uint8_t* pk_uv, const uint8_t* pk2_uv, size_t m);
KeysetForm keyset_form_wire(int scheme, const uint8_t* pk_bytes, size_t m);
KeysetForm keyset_form_mont_cols(int scheme, const dsv_column* cols, size_t m);  // dsv_keyed_mont.hip

// ---- decoded or normalised columns of a keyed batch: what a preparation launch leaves for the keyed call -----
struct KeyedCols {
  uint8_t *u, *m;  // m null: the caller's
  uint8_t *R, *Rp, *valid;
  u32* prefix;     // the normalisation's scratch; null for the wire form
  Items items(int scheme, const void* caller_m = nullptr) const {
    return make_items(scheme, u, {R, Rp}, m ? m : caller_m);
  }
};

// ---- the keyed wire form (dsv_keyed_wire.hip, keyed_wire.h) -----------------------------------------------
// the decoder's outputs for n records, in this order (dsv_keyed_wire_workspace_bytes): u, R, R' (double scheme
// only), valid; each part rounded up to 256 B
inline size_t keyed_wire_cols_bytes(int scheme, size_t n) {
  return align_up(n * 32, 256) + (size_t)keyed_sig_points(scheme) * align_up(n * 64, 256) + align_up(n, 256);
}
KeyedCols carve_keyed_wire(Stager& x, int scheme, size_t n);
// n signature records (device memory, 16-byte aligned) -> out.u, out.R() [, out.Rp()] and valid, one launch on
// `stream`; a step of its own so that it can stand in front of the keyed fast accept as well
void decode_keyed_wire(const Context& ctx, int scheme, const uint8_t* sig, size_t n, const Items& out, uint8_t* valid,
                       hipStream_t stream);

// ---- the by-value forms (dsv_keyed_lookup.hip; dsv_keyed_open.hip builds on them) --------------------------
constexpr size_t kLookupHostChunk = (size_t)1 << 18;  // items per chunk of the host forms
// a call without a handle before dsv_init is told that nothing is up (a handle, live or dead, goes through
// check_set like every keyed call)
int library_up(const dsv_keyset* ks);
// the keys of a batch in `form`: kKeyAffine — columns key_a [, key_b], 64 B per item each; kKeyRecord — records at
// key_a, 32 B per key point, key_b unused
bool keys_null(KeyForm form, int scheme, const void* key_a, const void* key_b);
// the lookup kernel reads a key in 16-byte loads
int check_key_alignment(KeyForm form, int scheme, const void* key_a, const void* key_b);
// misses (may be null): a 4-byte-aligned word on the set's device (ctx: the set's context)
int check_misses(const dsv_keyset* ks, const Context* ctx, const void* misses);
// the lookup of n items on s through the set's `form` index; every pointer device memory of the set's device.  An
// empty set has no index: everything misses.
int enqueue_lookup(const dsv_keyset* ks, KeyForm form, const void* key_a, const void* key_b, size_t n, uint32_t* idx,
                   uint32_t* misses, hipStream_t s);

// a batch's key bytes per item in `form`
inline size_t keys_item_bytes(KeyForm form, int scheme) {
  return (size_t)keyset_points(scheme) * key_point_bytes(form);
}
// host forms: the keys of items off .. off + cnt - 1 carved from st and copied up on the null stream (db null:
// one column)
int stage_keys(KeyForm form, int scheme, Stager& st, const uint8_t* key_a, const uint8_t* key_b, size_t off,
               size_t cnt, uint8_t*& da, uint8_t*& db);
// host forms of verify by affine key value: a chunk's columns carved from st and copied up — u, m, the nonce
// points, the key columns — with room for the index and verdict columns; nonce-point and key columns: 1 + 1,
// 2 + 2, and 1 + 2 for the var-generator scheme
struct AffineChunk {
  Items in;
  uint8_t *key_a, *key_b, *ok;
  uint32_t* idx;
};
int stage_affine_chunk(int scheme, Stager& st, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                       const uint8_t* m, const uint8_t* key_a, const uint8_t* key_b, size_t off, size_t cnt,
                       AffineChunk& c);
inline size_t affine_chunk_bytes(int scheme, size_t cnt) {
  return cnt * (32 + 32 + 4 + 1 + 64 * (size_t)(keyed_sig_points(scheme) + keyset_points(scheme))) + 12 * 256;
}
inline bool affine_inputs_null(int scheme, const void* u, const void* R_uv, const void* Rp_uv, const void* m,
                               const void* key_a, const void* key_b) {
  return !u || !R_uv || (keyed_sig_points(scheme) == 2 && !Rp_uv) || !m || keys_null(kKeyAffine, scheme, key_a, key_b);
}

// The body of the by-value host forms (lookup and verify, closed and open set, affine keys and records), under the
// registry's shared lock: library_up, check_set (scheme: the entry point's, or negative for the set's own), the
// form's scheme check, n == 0 (*misses = 0), null pointers, the context's lock and staging, then chunks of
// kLookupHostChunk items on the null stream, each synchronised once after its output column and its miss word
// were copied back; *misses (may be null) = the sum over the chunks.  A form supplies
//   scheme_check(scheme)       its own check of the set's scheme (DSV_OK: none),
//   inputs_null(scheme)        one of its input pointers is null,
//   stage_bytes(scheme, cnt)   the staging a chunk of cnt items needs, the miss word included,
//   chunk(ctx, scheme, st, off, cnt, dmiss, dout)   carves from st, copies items off .. off + cnt - 1 up, enqueues
//                              with dmiss as the lookup's miss word, and names the output column's device copy.
// out: the caller's output column, out_item bytes per item.
template <class Check, class Null, class Bytes, class Chunk>
int run_by_value_host(const dsv_keyset* ks, int scheme, Check scheme_check, Null inputs_null, Bytes stage_bytes,
                      size_t n, void* out, size_t out_item, size_t* misses, Chunk chunk) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, scheme, n, cp)) return r;
  scheme = ks->scheme;
  if (int r = scheme_check(scheme)) return r;
  if (n == 0) {
    if (misses) *misses = 0;
    return DSV_OK;
  }
  if (inputs_null(scheme) || !out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const size_t per = n < kLookupHostChunk ? n : kLookupHostChunk;
  if (int r = ensure_stage(ctx, stage_bytes(scheme, per))) return r;
  size_t total = 0;
  for (size_t off = 0; off < n; off += per) {
    const size_t cnt = n - off < per ? n - off : per;
    Stager st(ctx.stage);
    uint32_t* dmiss = reinterpret_cast<uint32_t*>(st.take(4));
    const void* dout = nullptr;
    if (int r = chunk(ctx, scheme, st, off, cnt, dmiss, dout)) return r;
    uint32_t missed = 0;
    D2H(static_cast<uint8_t*>(out) + off * out_item, dout, cnt * out_item);
    D2H(&missed, dmiss, 4);
    HIP_TRY(hipStreamSynchronize(0));
    total += missed;
  }
  if (misses) *misses = total;
  return DSV_OK;
}
inline int any_scheme(int) { return DSV_OK; }

// ---- the open-set forms' miss branch (dsv_keyed_open.hip) ---------------------------------------------------
// its part of a workspace: list | count | per-lane window tables, and for kKeyRecord behind them the key columns
// P0 [| P1] it decompresses into, of which only the listed rows are ever written
size_t open_miss_bytes(KeyForm form, int scheme, size_t n);
struct MissBranch {
  uint32_t *list, *count, *tables;
  const uint8_t *key_a, *key_b;  // the items' affine key columns: the caller's, or own_a / own_b
  const uint8_t* records;        // not null: the items' key records, decompressed for the listed items into
  uint8_t *own_a, *own_b;        //   columns of the branch's own
};
// kKeyAffine: key_a / key_b are the caller's columns; kKeyRecord: key_a the records, key_b unused
MissBranch carve_miss_branch(Stager& x, KeyForm form, int scheme, size_t n, const void* key_a, const void* key_b);
// behind the keyed kernel on s: the misses of idx are listed, their keys decompressed if the branch holds records
// (the decode flags AND-ed into w.valid), and decided by the unkeyed equation from the c / valid the challenge hash
// left in w; in: the keyed call's items (the var-generator scheme: key_a / key_b = PK / Gen, one three-base chain)
int enqueue_miss_branch(const Context& ctx, const Items& in, const uint32_t* idx, size_t n, uint8_t* ok,
                        const MissBranch& b, const Workspace& w, hipStream_t s);

}  // namespace dsvh
