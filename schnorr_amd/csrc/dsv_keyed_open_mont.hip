// dsv_keyed_open_mont.hip — the key cache for typed objects (include/dsv.h: dsv_verify_keyed_open_mont_*;
// keyed_open_mont.h): the open-set form of verify over exactly the arguments of the reference's
// `verify_batch` — `Signature*`, `PublicKey*` and `BlsScalar` objects, Montgomery limbs and projective points.  The
// verdicts are those of dsv_verify_*_mont_dev on the same limbs for every input; an item whose key, once
// normalised, is a valid registered key is decided by that key's tables, every other item by the unkeyed equation on
// its own normalised key.  Device form, one stream, enqueue-only: the front kernel (normalisation of every point,
// scalar conversion, lookup of the key in the affine index), challenge hash and keyed kernel over all n (a miss
// gets 0 there), then the miss branch of dsv_keyed_open.hip over key columns of the call's own.  Host form: the
// front kernel once per chunk of the shared host pipeline (dsv_pipeline.h), the rest per sub-batch, under the
// key-set registry's shared lock for the whole call.  Submit: dsv_host.hip's job driver around the host form.
// DSV_OPEN_MONT_FUSED=0 (dsv_context.hip) runs the front as two launches — k_normalize_uvz over all points, then
// k_index_lookup over the normalised key columns — with the same outputs: the cross-check of the front kernel.
#include "dsv_pipeline.h"
#include "keyed_mont.h"
#include "keyed_open_mont.h"

namespace dsv {
namespace {
__global__ void k_add_word(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && *src) atomicAdd(dst, *src);
}
}  // namespace
}  // namespace dsv

namespace dsvh {
namespace {

// what the front writes for n items besides the index column and the miss branch's key columns, in this order:
// u, m, R, R' (double scheme only), valid, the prefix products of all nps + npk points; each part rounded up to
// 256 B (carve_keyed_mont's order: the prefix is the only part that differs from the keyed typed form's)
size_t open_mont_cols_bytes(int scheme, size_t n) {
  const int nps = keyed_sig_points(scheme), np = nps + keyset_points(scheme);
  return 2 * align_up(n * 32, 256) + (size_t)nps * align_up(n * 64, 256) + align_up(n, 256) +
         align_up(normalize_prefix_bytes(n, np), 256);
}
KeyedCols carve_open_mont(Stager& x, int scheme, size_t n) {
  const int nps = keyed_sig_points(scheme), np = nps + keyset_points(scheme);
  KeyedCols w;
  w.u = x.take(n * 32);
  w.m = x.take(n * 32);
  w.R = x.take(n * 64);
  w.Rp = nps == 2 ? x.take(n * 64) : nullptr;
  w.valid = x.take(n);
  w.prefix = reinterpret_cast<u32*>(x.take(normalize_prefix_bytes(n, np)));
  return w;
}
// idx | list | count | window tables | own PK [| own PK' / Gen] | u | m | R [| R'] | valid | prefix
size_t open_mont_front_bytes(int scheme, size_t n) {
  return align_up(4 * n, 256) + open_miss_bytes(kKeyRecord, scheme, n) + open_mont_cols_bytes(scheme, n);
}

// The front of n items on s.  u, m: 32 B Montgomery limbs; sig[0 .. nps), key[0 .. npk): 96 B limbs of u || v || z
// (device memory, 16-byte aligned) -> w, idx, the rows of own_a [, own_b] of the items that miss; misses (may be
// null): the count is ADDED to it.  add_scratch: a device word of the caller's for the two-launch path's own count.
int enqueue_front(const Context& ctx, const dsv_keyset* ks, const uint8_t* u, const uint8_t* const* sig,
                  const uint8_t* const* key, const uint8_t* m, size_t n, const KeyedCols& w, uint8_t* own_a,
                  uint8_t* own_b, uint32_t* idx, uint32_t* misses, uint32_t* add_scratch, hipStream_t s, int per_lane,
                  int block) {
  const int scheme = ks->scheme, nps = keyed_sig_points(scheme), npk = keyset_points(scheme);
  NormalizeArgs a = {};
  a.in[0] = sig[0];
  a.out[0] = w.R;
  if (nps == 2) {
    a.in[1] = sig[1];
    a.out[1] = w.Rp;
  }
  a.in[nps] = key[0];
  a.out[nps] = own_a;
  if (npk == 2) {
    a.in[nps + 1] = key[1];
    a.out[nps + 1] = own_b;
  }
  a.u_mont = u;
  a.m_mont = m;
  a.u_out = w.u;
  a.m_out = w.m;
  if (ctx.open_mont_fused) {
    const dsv_keyset::KeyIndex& ix = ks->index[kKeyAffine];
    launch_normalize_lookup(a, nps, npk, n, w.valid, w.prefix, ix.rows, ix.slots, ks->slot_mask, ks->k, idx, misses, s,
                            per_lane, block);
    HIP_TRY(hipGetLastError());
    return DSV_OK;
  }
  launch_normalize_uvz(a, nps + npk, n, w.valid, w.prefix, s, per_lane, block);
  HIP_TRY(hipGetLastError());
  if (int r = enqueue_lookup(ks, kKeyAffine, own_a, own_b, n, idx, misses ? add_scratch : nullptr, s)) return r;
  launch_unusable_keys_miss(key[0], key[1], npk, n, idx, misses ? add_scratch : nullptr, s);
  HIP_TRY(hipGetLastError());
  if (misses) {
    hipLaunchKernelGGL(k_add_word, dim3(1), dim3(64), 0, s, misses, (const uint32_t*)add_scratch);
    HIP_TRY(hipGetLastError());
  }
  return DSV_OK;
}

int check_limb_alignment(const void* const* cols, int ncols) {
  for (int c = 0; c < ncols; c++)
    if ((uintptr_t)cols[c] & 15) return fail(DSV_ERR_INVALID_ARGUMENT, "input columns must be 16-byte aligned");
  return DSV_OK;
}

// argument checks of an open typed column batch, before the set is looked at (check_keyed_mont_cols's order): n,
// the set pointer, then every column as dsv_verify_*_mont_cols checks it.  The caller holds the shared lock.
int check_open_mont_cols(const dsv_keyset* ks, const dsv_column* cols, size_t n, const uint8_t* ok) {
  if (int r = check_n(n)) return r;
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  if (n == 0) return DSV_OK;
  return check_cols(ks->scheme, cols, n, ok, kMont);
}

}  // namespace

// host objects: per chunk ONE preprocessing launch (the front kernel over all the chunk's points), per sub-batch
// the challenge hash and the keyed kernel with the front's validity bytes as valid_in, then the miss branch on the
// sub-batch's rows.  The lane's verify workspace is c | valid | window tables and no more, so the keyed workspace
// and the listed kernel's tables are the lane's own, and the miss list with its length word lies in the lane's
// scratch behind it (4 B per item).  misses (may be null): one device word lent by the context, zeroed before the
// first chunk, added to by every chunk's front, read back once behind the last verdict.
int verify_keyed_open_mont_cols_locked(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok,
                                       size_t* misses) {
  if (int r = check_open_mont_cols(ks, cols, n, ok)) return r;
  const int scheme = ks->scheme;
  Context* cp = nullptr;
  if (int r = check_set(ks, scheme, n, cp)) return r;
  if (n == 0) {
    if (misses) *misses = 0;
    return DSV_OK;
  }
  const int nps = keyed_sig_points(scheme), npk = keyset_points(scheme), np = nps + npk;
  HostIn ins[kMaxHostIn];
  const size_t nin = column_inputs(scheme, kMont, cols, 0, ins);
  // the call's sum: one of the context's 64 miss words, lent for the call (no allocation, no device-wide wait)
  struct MissWord {
    Context& ctx;
    int w = -1;
    ~MissWord() {
      if (w < 0) return;
      std::lock_guard<std::mutex> lk(ctx.miss_words_mu);
      ctx.miss_words_used &= ~((uint64_t)1 << w);
    }
  } word{*cp};
  uint32_t* dmiss = nullptr;
  if (misses) {
    DSV_ON_DEVICE(*cp);
    {
      std::lock_guard<std::mutex> lk(cp->miss_words_mu);
      if (!cp->miss_words) HIP_TRY(hipMalloc(&cp->miss_words, 64 * sizeof(uint32_t)));
      for (int w = 0; w < 64 && word.w < 0; w++)
        if (!(cp->miss_words_used >> w & 1)) word.w = w;
      if (word.w < 0) return fail(DSV_ERR_HIP, "more than 64 open typed calls in flight on device %d", cp->device);
      cp->miss_words_used |= (uint64_t)1 << word.w;
    }
    dmiss = cp->miss_words + word.w;
    launch_store_word(dmiss, 0, hipStreamPerThread);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
  }
  // scratch of the chunk's front per item: idx, u, m, the nonce points, valid, the prefix products, the key columns
  const size_t prep_item_bytes = 4 + 64 + (size_t)nps * 64 + 1 + (size_t)np * kLimbs * 4 + (size_t)npk * 64;
  const int rc = run_pipelined(
      *cp, ins, nin, ok, n, prep_item_bytes, 4,
      [=](const void* const* d, size_t c, Stager& x, hipStream_t st, Staged& g) {
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * c));
        uint8_t* own_a = x.take(c * 64);
        uint8_t* own_b = npk == 2 ? x.take(c * 64) : nullptr;
        const KeyedCols w = carve_open_mont(x, scheme, c);
        const uint8_t* sig[2] = {(const uint8_t*)d[1], nps == 2 ? (const uint8_t*)d[2] : nullptr};
        const uint8_t* key[2] = {(const uint8_t*)d[1 + nps], npk == 2 ? (const uint8_t*)d[2 + nps] : nullptr};
        uint32_t* chunk_count = reinterpret_cast<uint32_t*>(x.take(4));  // (the two-launch path's, per chunk)
        if (int r = enqueue_front(*cp, ks, (const uint8_t*)d[0], sig, key, (const uint8_t*)d[1 + np], c, w, own_a,
                                  own_b, idx, dmiss, chunk_count, st, cp->norm_per_lane, cp->norm_block))
          return r;
        // staged as u, R, R' (null unless double), key_idx, m, own PK, own PK' / Gen (null for single)
        g.p[0] = w.u, g.p[1] = w.R, g.p[2] = w.Rp, g.p[3] = (const uint8_t*)idx, g.p[4] = w.m, g.p[5] = own_a,
        g.p[6] = own_b;
        g.bytes[0] = g.bytes[4] = 32, g.bytes[1] = g.bytes[2] = g.bytes[5] = g.bytes[6] = 64, g.bytes[3] = 4;
        g.valid = w.valid;
        return (int)DSV_OK;
      },
      [=](const Staged& g, size_t off, size_t cnt, void* dok, void* ws, Stager& extra, hipStream_t st) {
        const Items in = make_items(scheme, g.p[0] + off * 32,
                                    {g.p[1] + off * 64, g.p[2] ? g.p[2] + off * 64 : nullptr}, g.p[4] + off * 32);
        const uint32_t* idx = reinterpret_cast<const uint32_t*>(g.p[3] + off * 4);
        enqueue_keyed(*cp, ks, in, idx, cnt, static_cast<uint8_t*>(dok), ws, st, g.valid + off);
        HIP_TRY(hipGetLastError());
        const Workspace w = carve(ws, cnt);
        MissBranch b{};
        b.list = reinterpret_cast<uint32_t*>(extra.take(4 * cnt));
        b.count = reinterpret_cast<uint32_t*>(extra.take(4));
        b.tables = w.tables;
        b.key_a = g.p[5] + off * 64;
        b.key_b = g.p[6] ? g.p[6] + off * 64 : nullptr;
        return enqueue_miss_branch(*cp, in, idx, cnt, static_cast<uint8_t*>(dok), b, w, st);
      },
      0);
  if (rc) return rc;
  if (misses) {
    DSV_ON_DEVICE(*cp);
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, dmiss, 4, hipMemcpyDeviceToHost, hipStreamPerThread));
    HIP_TRY(hipStreamSynchronize(hipStreamPerThread));
    *misses = total;
  }
  return DSV_OK;
}

}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyed_open_mont_workspace_bytes(int scheme, size_t n) {
  return scheme_ok(scheme) ? open_mont_front_bytes(scheme, n) + keyed_ws_bytes(n) : 0;
}

int dsv_verify_keyed_open_mont_dev(const dsv_keyset* ks, const void* u, const void* R_uvz, const void* Rp_uvz,
                                   const void* key_a_uvz, const void* key_b_uvz, const void* m, size_t n, void* ok,
                                   void* workspace, size_t workspace_bytes, void* stream, void* misses) {
  if (int r = library_up(ks)) return r;
  // the workspace in order: open_mont_front_bytes | c | valid; run_keyed_dev checks and hands on the index pointer,
  // which is the workspace itself
  MissBranch b{};
  Items items;
  return run_keyed_dev(
      ks, -1,
      [=](int scheme) {
        return !u || !R_uvz || (keyed_sig_points(scheme) == 2 && !Rp_uvz) || !m ||
               keys_null(kKeyAffine, scheme, key_a_uvz, key_b_uvz);
      },
      [=](int scheme) { return open_mont_front_bytes(scheme, n); }, workspace, n, ok, workspace, workspace_bytes,
      stream,
      [&](const Context& ctx, int scheme, Stager& x, hipStream_t s, Items& in, const uint8_t*& valid_in) {
        const int nps = keyed_sig_points(scheme), npk = keyset_points(scheme);
        const void* limbs[6] = {u, m, R_uvz, key_a_uvz, nps == 2 ? Rp_uvz : u, npk == 2 ? key_b_uvz : u};
        if (int r = check_limb_alignment(limbs, 6)) return r;
        if (int r = check_misses(ks, &ctx, misses)) return r;
        uint32_t* idx = reinterpret_cast<uint32_t*>(x.take(4 * n));
        b = carve_miss_branch(x, kKeyRecord, scheme, n, nullptr, nullptr);  // key columns of its own, no records
        const KeyedCols w = carve_open_mont(x, scheme, n);
        items = in = w.items(scheme);
        valid_in = w.valid;
        uint32_t* dmiss = static_cast<uint32_t*>(misses);
        if (dmiss) {
          launch_store_word(dmiss, 0, s);
          HIP_TRY(hipGetLastError());
        }
        const uint8_t* sig[2] = {(const uint8_t*)R_uvz, (const uint8_t*)Rp_uvz};
        const uint8_t* key[2] = {(const uint8_t*)key_a_uvz, (const uint8_t*)key_b_uvz};
        // (the two-launch path counts into the miss list's length word, which the miss branch resets behind it)
        return enqueue_front(ctx, ks, (const uint8_t*)u, sig, key, (const uint8_t*)m, n, w, b.own_a, b.own_b, idx,
                             dmiss, b.count, s, 0, 0);
      },
      [&](const Context& ctx, hipStream_t s, const Workspace& w) {
        return enqueue_miss_branch(ctx, items, static_cast<const uint32_t*>(workspace), n, static_cast<uint8_t*>(ok),
                                   b, w, s);
      });
}

int dsv_verify_keyed_open_mont_cols(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok,
                                    size_t* misses) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  return verify_keyed_open_mont_cols_locked(ks, cols, n, ok, misses);
}

int dsv_verify_keyed_open_mont_cols_submit(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok,
                                           dsv_job** job) {
  if (!job) return fail(DSV_ERR_INVALID_ARGUMENT, "null job pointer");
  *job = nullptr;
  if (int r = library_up(ks)) return r;
  int ncols = 0;
  {
    std::shared_lock<std::shared_mutex> rl(keyset_mutex());
    if (int r = check_open_mont_cols(ks, cols, n, ok)) return r;
    ncols = layout(ks->scheme).points + 2;
  }
  return submit_cols_job(ks, kOpenMontJob, cols, n ? ncols : 0, n, ok, job);
}

}  // extern "C"
