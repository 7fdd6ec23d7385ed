// dsv_keyed_census.hip — the census of a batch's keys against a registered key set (include/dsv.h:
// dsv_keyset_census*; keyed_census.h): what a key cache reads to decide whom to admit and whom
// to evict.  Device forms: enqueue-only on the caller's stream, a straight chain — totals and table cleared, census,
// report; the typed form runs the *_mont forms' normalisation over the key points alone in front of it.  Host
// forms: the same per chunk of kLookupHostChunk items through the context's staging, the chunk reports merged on the
// host by key bytes.
#include <algorithm>
#include <string>
#include <unordered_map>

#include "keyed_census.h"
#include "keyset_host.h"

namespace dsvh {

namespace {
std::atomic<int> g_census_lds_keys{kCensusLdsKeys};
}

void census_configure() {
  int v = kCensusLdsKeys;
  if (const char* e = getenv("DSV_CENSUS_LDS_KEYS")) v = atoi(e);
  g_census_lds_keys.store(v < 0 ? 0 : (v > kCensusLdsKeysMax ? kCensusLdsKeysMax : v), std::memory_order_relaxed);
}

namespace {

// the typed form's part of a workspace behind the table: the normalised key columns, the validity bytes, the prefix
// products of the normalisation over npk points
size_t census_mont_cols_bytes(int scheme, size_t n) {
  const int npk = keyset_points(scheme);
  return (size_t)npk * align_up(n * 64, 256) + align_up(n, 256) + align_up(normalize_prefix_bytes(n, npk), 256);
}

struct CensusOut {
  uint32_t *idx, *hits, *rep, *count, *totals;
};

// the census of n items on s; every pointer device memory of the set's device.  usable: keyed_census.h
int enqueue_census(const dsv_keyset* ks, KeyForm form, const void* key_a, const void* key_b, const uint8_t* usable,
                   size_t n, const CensusOut& o, void* table, hipStream_t s) {
  const dsv_keyset::KeyIndex& ix = ks->index[form];
  launch_census(form, static_cast<const uint8_t*>(key_a), static_cast<const uint8_t*>(key_b), usable,
                keyset_points(ks->scheme), n, ks->k ? ix.rows : nullptr, ks->k ? ix.slots : nullptr, ks->slot_mask,
                ks->k, g_census_lds_keys.load(std::memory_order_relaxed), o.idx, o.hits, o.rep, o.count, o.totals,
                table, s);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

// the typed form on s: the key points (96 B limbs of u || v || z) normalised into columns of the call's own carved
// from x, then the affine census over them; an item whose limbs are unusable has validity byte 0
int enqueue_census_mont(const dsv_keyset* ks, const void* key_a, const void* key_b, size_t n, const CensusOut& o,
                        void* table, Stager& x, hipStream_t s, uint8_t** own_a_out = nullptr,
                        uint8_t** own_b_out = nullptr) {
  const int npk = keyset_points(ks->scheme);
  uint8_t* own_a = x.take(n * 64);
  uint8_t* own_b = npk == 2 ? x.take(n * 64) : nullptr;
  uint8_t* valid = x.take(n);
  u32* prefix = reinterpret_cast<u32*>(x.take(normalize_prefix_bytes(n, npk)));
  NormalizeArgs a = {};
  a.in[0] = static_cast<const uint8_t*>(key_a);
  a.out[0] = own_a;
  if (npk == 2) {
    a.in[1] = static_cast<const uint8_t*>(key_b);
    a.out[1] = own_b;
  }
  launch_normalize_uvz(a, npk, n, valid, prefix, s);
  HIP_TRY(hipGetLastError());
  if (own_a_out) *own_a_out = own_a;
  if (own_b_out) *own_b_out = own_b;
  return enqueue_census(ks, kKeyAffine, own_a, own_b, valid, n, o, table, s);
}

// the _dev forms; mont: the typed form (key columns of limbs, read as the affine form's two columns)
int census_dev(KeyForm form, bool mont, const dsv_keyset* ks, const void* key_a, const void* key_b, size_t n,
               void* key_idx_out, void* hits, void* miss_rep, void* miss_count, void* totals, void* workspace,
               size_t workspace_bytes, void* stream) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  if (n == 0) return DSV_OK;
  if (keys_null(form, ks->scheme, key_a, key_b) || !miss_rep || !miss_count || !totals || !workspace)
    return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  if (int r = check_key_alignment(form, ks->scheme, key_a, key_b)) return r;
  if (((uintptr_t)key_idx_out | (uintptr_t)hits | (uintptr_t)miss_rep | (uintptr_t)miss_count | (uintptr_t)totals) & 3)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key_idx_out, hits, miss_rep, miss_count and totals must be 4-byte aligned");
  if ((uintptr_t)workspace & 15) return fail(DSV_ERR_INVALID_ARGUMENT, "workspace must be 16-byte aligned");
  const size_t need = census_table_bytes(n) + (mont ? census_mont_cols_bytes(ks->scheme, n) : 0);
  if (workspace_bytes < need)
    return fail(DSV_ERR_INVALID_ARGUMENT, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  Context* octx = nullptr;
  if (int r = device_context(totals, octx)) return r;
  if (octx != cp)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key set of device %d used on device %d", ks->device, octx->device);
  DSV_ON_DEVICE(*cp);
  const CensusOut o = {static_cast<uint32_t*>(key_idx_out), static_cast<uint32_t*>(hits),
                       static_cast<uint32_t*>(miss_rep), static_cast<uint32_t*>(miss_count),
                       static_cast<uint32_t*>(totals)};
  Stager x(static_cast<uint8_t*>(workspace));
  void* table = x.take(census_table_bytes(n));
  if (mont) return enqueue_census_mont(ks, key_a, key_b, n, o, table, x, (hipStream_t)stream);
  return enqueue_census(ks, form, key_a, key_b, nullptr, n, o, table, (hipStream_t)stream);
}

// What a host form supplies: its keys' chunk staged and the census enqueued on the null stream (stage), what it
// needs per item of staging (item_bytes), what it copies back before the chunk's wait (collect; may be empty), and
// the key bytes of item `rep` of the chunk at `off`, as the merge compares them (key).
struct HostKeys {
  std::function<bool(int scheme)> null;
  std::function<size_t(int scheme)> item_bytes;
  std::function<int(int scheme, Stager& st, size_t off, size_t cnt, const CensusOut& o, void* table)> stage;
  std::function<int(size_t cnt)> collect;
  std::function<std::string(int scheme, size_t off, uint32_t rep)> key;
};

// The body of the host forms: the plain chunk loop (not the pipeline), blocking.  The device's hits for the whole
// call accumulate in one staged array, added to the caller's at the end; a chunk's report names items of the chunk,
// merged into the call's by key bytes — chunks come in order, so the first representative seen is the lowest.
int census_host(const dsv_keyset* ks, const HostKeys& form, size_t n, uint32_t* key_idx_out, uint32_t* hits,
                uint32_t* miss_rep, uint32_t* miss_count, size_t totals[4]) {
  if (int r = library_up(ks)) return r;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, -1, n, cp)) return r;
  const int scheme = ks->scheme;
  if (n == 0) {
    if (totals) totals[0] = totals[1] = totals[2] = totals[3] = 0;
    return DSV_OK;
  }
  if (form.null(scheme) || !miss_rep || !miss_count || !totals) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const size_t k = ks->k, per = n < kLookupHostChunk ? n : kLookupHostChunk;
  if (int r = ensure_stage(ctx, align_up(4 * (k + 1), 256) + per * (form.item_bytes(scheme) + 12) +
                                    census_table_bytes(per) + 40 * 256))
    return r;
  struct Entry {
    uint32_t rep, count;
  };
  std::vector<Entry> report;
  std::unordered_map<std::string, size_t> place;
  std::vector<uint32_t> rep, count;
  size_t missed = 0, unusable = 0;
  uint32_t* dhits = nullptr;
  for (size_t off = 0; off < n; off += per) {
    const size_t cnt = n - off < per ? n - off : per;
    Stager st(ctx.stage);
    uint32_t* dh = reinterpret_cast<uint32_t*>(st.take(4 * (k + 1)));  // (the same bytes in every chunk)
    if (hits && !dhits) {
      dhits = dh;
      HIP_TRY(hipMemsetAsync(dhits, 0, 4 * k, 0));
    }
    CensusOut o;
    o.hits = dhits;
    o.idx = key_idx_out ? reinterpret_cast<uint32_t*>(st.take(4 * cnt)) : nullptr;
    o.rep = reinterpret_cast<uint32_t*>(st.take(4 * cnt));
    o.count = reinterpret_cast<uint32_t*>(st.take(4 * cnt));
    o.totals = reinterpret_cast<uint32_t*>(st.take(16));
    void* table = st.take(census_table_bytes(cnt));
    if (int r = form.stage(scheme, st, off, cnt, o, table)) return r;
    uint32_t t[4] = {0, 0, 0, 0};
    if (o.idx) D2H(key_idx_out + off, o.idx, 4 * cnt);
    D2H(t, o.totals, 16);
    if (int r = form.collect(cnt)) return r;
    HIP_TRY(hipStreamSynchronize(0));
    rep.resize(t[0]);
    count.resize(t[0]);
    if (t[0]) {
      D2H(rep.data(), o.rep, 4 * (size_t)t[0]);
      D2H(count.data(), o.count, 4 * (size_t)t[0]);
      HIP_TRY(hipStreamSynchronize(0));
    }
    for (uint32_t j = 0; j < t[0]; j++) {
      const auto at = place.emplace(form.key(scheme, off, rep[j]), report.size());
      if (at.second) report.push_back({(uint32_t)(off + rep[j]), count[j]});
      else report[at.first->second].count += count[j];
    }
    missed += t[1];
    unusable += t[2];
  }
  if (dhits && k) {
    std::vector<uint32_t> h(k);
    D2H(h.data(), dhits, 4 * k);
    HIP_TRY(hipStreamSynchronize(0));
    for (size_t j = 0; j < k; j++) hits[j] += h[j];
  }
  std::sort(report.begin(), report.end(),
            [](const Entry& a, const Entry& b) { return a.count != b.count ? a.count > b.count : a.rep < b.rep; });
  for (size_t j = 0; j < report.size(); j++) {
    miss_rep[j] = report[j].rep;
    miss_count[j] = report[j].count;
  }
  totals[0] = report.size();
  totals[1] = missed;
  totals[2] = unusable;
  totals[3] = 0;
  return DSV_OK;
}

// host arrays of key bytes (affine columns or records): staged by stage_keys, compared as they are
HostKeys host_keys_bytes(const dsv_keyset* ks, KeyForm form, const uint8_t* key_a, const uint8_t* key_b) {
  HostKeys f;
  f.null = [=](int scheme) { return keys_null(form, scheme, key_a, key_b); };
  f.item_bytes = [=](int scheme) { return keys_item_bytes(form, scheme); };
  f.stage = [=](int scheme, Stager& st, size_t off, size_t cnt, const CensusOut& o, void* table) {
    uint8_t *da, *db;
    if (int r = stage_keys(form, scheme, st, key_a, key_b, off, cnt, da, db)) return r;
    return enqueue_census(ks, form, da, db, nullptr, cnt, o, table, 0);
  };
  f.collect = [](size_t) { return (int)DSV_OK; };
  f.key = [=](int scheme, size_t off, uint32_t rep) {
    const size_t i = off + rep;
    if (form == kKeyRecord) {
      const size_t w = keys_item_bytes(form, scheme);
      return std::string(reinterpret_cast<const char*>(key_a + i * w), w);
    }
    std::string s(reinterpret_cast<const char*>(key_a + i * 64), 64);
    if (keyset_points(scheme) == 2) s.append(reinterpret_cast<const char*>(key_b + i * 64), 64);
    return s;
  };
  return f;
}

// `PublicKey*` objects where they lie: gathered dense per chunk, normalised on the device; the merge compares the
// normalised bytes, copied back per chunk
HostKeys host_keys_mont(const dsv_keyset* ks, const dsv_column* cols) {
  struct Shared {
    std::vector<uint8_t> dense, norm_a, norm_b;
    uint8_t *own_a = nullptr, *own_b = nullptr;
  };
  auto sh = std::make_shared<Shared>();
  HostKeys f;
  f.null = [=](int scheme) {
    if (!cols) return true;
    for (int p = 0; p < keyset_points(scheme); p++)
      if (!cols[p].base || cols[p].stride < 96) return true;
    return false;
  };
  // limbs + normalised columns + validity + prefix products (normalize_prefix_bytes: 36 B per point and item)
  f.item_bytes = [=](int scheme) { return (size_t)keyset_points(scheme) * (96 + 64 + kLimbs * 4) + 1; };
  f.stage = [=](int scheme, Stager& st, size_t off, size_t cnt, const CensusOut& o, void* table) {
    const int npk = keyset_points(scheme);
    sh->dense.resize((size_t)npk * cnt * 96);
    uint8_t* d[2] = {nullptr, nullptr};
    for (int p = 0; p < npk; p++) {
      copy_strided_plain(sh->dense.data() + (size_t)p * cnt * 96,
                         static_cast<const uint8_t*>(cols[p].base) + off * cols[p].stride, cols[p].stride, 96, cnt);
      d[p] = st.take(cnt * 96);
      H2D(d[p], sh->dense.data() + (size_t)p * cnt * 96, cnt * 96);
    }
    return enqueue_census_mont(ks, d[0], d[1], cnt, o, table, st, 0, &sh->own_a, &sh->own_b);
  };
  f.collect = [=](size_t cnt) {
    sh->norm_a.resize(cnt * 64);
    D2H(sh->norm_a.data(), sh->own_a, cnt * 64);
    if (sh->own_b) {
      sh->norm_b.resize(cnt * 64);
      D2H(sh->norm_b.data(), sh->own_b, cnt * 64);
    }
    return (int)DSV_OK;
  };
  f.key = [=](int, size_t, uint32_t rep) {
    std::string s(reinterpret_cast<const char*>(sh->norm_a.data() + (size_t)rep * 64), 64);
    if (sh->own_b) s.append(reinterpret_cast<const char*>(sh->norm_b.data() + (size_t)rep * 64), 64);
    return s;
  };
  return f;
}

}  // namespace
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyset_census_workspace_bytes(size_t n) { return census_table_bytes(n); }
size_t dsv_keyset_census_mont_workspace_bytes(int scheme, size_t n) {
  return scheme_ok(scheme) ? census_table_bytes(n) + census_mont_cols_bytes(scheme, n) : 0;
}
int dsv_debug_census_lds_keys(void) { return g_census_lds_keys.load(std::memory_order_relaxed); }

int dsv_keyset_census_dev(const dsv_keyset* ks, const void* key_a, const void* key_b, size_t n, void* key_idx_out,
                          void* hits, void* miss_rep, void* miss_count, void* totals, void* workspace,
                          size_t workspace_bytes, void* stream) {
  return census_dev(kKeyAffine, false, ks, key_a, key_b, n, key_idx_out, hits, miss_rep, miss_count, totals,
                    workspace, workspace_bytes, stream);
}
int dsv_keyset_census_wire_dev(const dsv_keyset* ks, const void* pk_records, size_t n, void* key_idx_out, void* hits,
                               void* miss_rep, void* miss_count, void* totals, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return census_dev(kKeyRecord, false, ks, pk_records, nullptr, n, key_idx_out, hits, miss_rep, miss_count, totals,
                    workspace, workspace_bytes, stream);
}
int dsv_keyset_census_mont_dev(const dsv_keyset* ks, const void* key_a_uvz, const void* key_b_uvz, size_t n,
                               void* key_idx_out, void* hits, void* miss_rep, void* miss_count, void* totals,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return census_dev(kKeyAffine, true, ks, key_a_uvz, key_b_uvz, n, key_idx_out, hits, miss_rep, miss_count, totals,
                    workspace, workspace_bytes, stream);
}

int dsv_keyset_census(const dsv_keyset* ks, const uint8_t* key_a, const uint8_t* key_b, size_t n,
                      uint32_t* key_idx_out, uint32_t* hits, uint32_t* miss_rep, uint32_t* miss_count,
                      size_t totals[4]) {
  return census_host(ks, host_keys_bytes(ks, kKeyAffine, key_a, key_b), n, key_idx_out, hits, miss_rep, miss_count,
                     totals);
}
int dsv_keyset_census_wire(const dsv_keyset* ks, const uint8_t* pk_records, size_t n, uint32_t* key_idx_out,
                           uint32_t* hits, uint32_t* miss_rep, uint32_t* miss_count, size_t totals[4]) {
  return census_host(ks, host_keys_bytes(ks, kKeyRecord, pk_records, nullptr), n, key_idx_out, hits, miss_rep,
                     miss_count, totals);
}
int dsv_keyset_census_mont_cols(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint32_t* key_idx_out,
                                uint32_t* hits, uint32_t* miss_rep, uint32_t* miss_count, size_t totals[4]) {
  return census_host(ks, host_keys_mont(ks, cols), n, key_idx_out, hits, miss_rep, miss_count, totals);
}

}  // extern "C"
