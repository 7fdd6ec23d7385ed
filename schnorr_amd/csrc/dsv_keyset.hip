// dsv_keyset.hip — registered key sets (include/dsv.h: dsv_keyset_*, dsv_verify_*_keyed*): creation from
// affine points or wire records, with or without reserved capacity, appending keys to a live set, replacing keys of
// a live set in place (the quiesce, the commit and the index rebuild of k_keyed_replace.hip), the registry that
// dsv_shutdown_device empties, and the keyed verify entry points (k_challenge unchanged, then k_verify_keyed;
// keyed.h).
#include <algorithm>
#include <shared_mutex>

#include "keyset_host.h"

namespace dsvh {
namespace {
// live key sets; verify calls read under the shared lock, create / destroy / shutdown write under the
// exclusive one; an append builds its rows under the shared lock and raises k under the exclusive one; a replace
// builds its tables under the shared lock and writes the set under the exclusive one, on a device that has run dry
std::shared_mutex g_ks_mu;
std::vector<dsv_keyset*> g_keysets;

constexpr size_t kKeyedHostChunk = (size_t)1 << 18;
constexpr size_t kMaxKeys = 0xffffffffu;  // indices are uint32

// the tables and the indices of a set (its device selected)
void free_device_memory(dsv_keyset* ks) {
  if (ks->tables) (void)hipFree(ks->tables);
  ks->tables = nullptr;
  ks->key_ok = nullptr;
  for (dsv_keyset::KeyIndex& ix : ks->index) {
    if (ix.rows) (void)hipFree(ix.rows);
    ix = {};
  }
}

void free_sets_of(int device) {  // (exclusive lock held)
  for (dsv_keyset* ks : g_keysets) {
    if (ks->device != device || !ks->alive) continue;
    free_device_memory(ks);
    ks->alive = false;
  }
}

// the context a key set's device work runs in: its device must still be initialised
int keyset_context(const dsv_keyset* ks, Context*& out) {
  if (!ks->alive || ks->device < 0 || ks->device >= kMaxDevices ||
      !g_ctx[ks->device].ready.load(std::memory_order_acquire))
    return fail(DSV_ERR_NOT_INITIALIZED, "the key set's device was shut down");
  out = &g_ctx[ks->device];
  return DSV_OK;
}

// the calling thread's current device, which must be initialised
int current_context(Context*& out) {
  if (g_primary.load(std::memory_order_acquire) < 0) return fail(DSV_ERR_NOT_INITIALIZED, "dsv_init() has not been called");
  int d = -1;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= kMaxDevices || !g_ctx[d].ready.load(std::memory_order_acquire))
    return fail(DSV_ERR_NOT_INITIALIZED, "the current device %d is not initialised", d);
  out = &g_ctx[d];
  return DSV_OK;
}

// device buffers + stream of one create / append call, released on every path
struct Scratch {
  uint8_t* dev = nullptr;
  hipStream_t s = nullptr;
  ~Scratch() {
    if (s) (void)hipStreamSynchronize(s);
    if (dev) (void)hipFree(dev);
    if (s) (void)hipStreamDestroy(s);
  }
};

// The one body that registers keys: the m keys of `form` become rows first .. first + m - 1 of ks — their affine
// points staged into a scratch of this call's (np x m x 64 B, then the form's own bytes from the next 256-byte
// boundary), their tables and key_ok bytes built, their rows and slots added to both indices — on a stream of the
// call's own (x.s; x.dev: the scratch), synchronised before it returns.  Writes only rows >= first and slots that
// are empty.  ks->k is the caller's to raise.  (ks's device memory held: a new set, or the registry's shared lock.)
int register_keys(Context& ctx, dsv_keyset* ks, size_t first, size_t m, const KeysetForm& form, Scratch& x) {
  if (m == 0) return DSV_OK;
  const int scheme = ks->scheme, np = keyset_points(scheme);
  const size_t off_own = align_up((size_t)np * m * 64, 256);
  HIP_TRY(hipMalloc(&x.dev, off_own + form.own_bytes));
  const uint8_t* P0 = x.dev;
  const uint8_t* P1 = np == 2 ? x.dev + m * 64 : nullptr;
  uint8_t* valid = nullptr;
  if (int r = form.stage(ctx, x.dev, x.dev + off_own, x.s, valid)) return r;
  launch_build_key_tables(P0, P1, valid, np, m, ks->tables + first * (size_t)np * kKeyPointWords, ks->key_ok + first,
                          x.s);
  HIP_TRY(hipGetLastError());
  // the indices, behind the table build (they read key_ok): the affine one, then the same keys by their records
  for (KeyForm f : {kKeyAffine, kKeyRecord}) {
    launch_index_append(f, P0, P1, ks->key_ok + first, np, first, m, ks->index[f].rows, ks->index[f].slots,
                        ks->slot_mask, x.s);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(x.s));
  return DSV_OK;
}

// the `f` index of a set for ks->capacity keys: the rows, then the slots
int allocate_index(dsv_keyset* ks, KeyForm f) {
  dsv_keyset::KeyIndex& ix = ks->index[f];
  HIP_TRY(hipMalloc(&ix.rows, keyset_index_total_bytes(f, ks->scheme, ks->capacity)));
  ix.slots = reinterpret_cast<uint32_t*>(ix.rows + keyset_index_rows_bytes(f, ks->scheme, ks->capacity));
  return DSV_OK;
}

// the allocations of a set for ks->capacity keys, never moved afterwards: key_ok zeroed, every slot empty (on s)
int allocate_keyset(dsv_keyset* ks, hipStream_t s) {
  const int scheme = ks->scheme;
  const size_t cap = ks->capacity;
  ks->bytes = keyset_total_bytes(scheme, cap);
  if (cap == 0) return DSV_OK;
  HIP_TRY(hipMalloc(&ks->tables, ks->bytes));
  ks->key_ok = reinterpret_cast<uint8_t*>(ks->tables) + keyset_table_bytes(scheme, cap);
  ks->slot_mask = keyset_index_cap(cap) - 1;
  if (int r = allocate_index(ks, kKeyAffine)) return r;
  HIP_TRY(hipMemsetAsync(ks->key_ok, 0, ks->bytes - keyset_table_bytes(scheme, cap), s));
  HIP_TRY(launch_clear_key_index(ks->index[kKeyAffine].slots, ks->slot_mask, s));
  if (int r = allocate_index(ks, kKeyRecord)) return r;
  HIP_TRY(launch_clear_key_index(ks->index[kKeyRecord].slots, ks->slot_mask, s));
  return DSV_OK;
}

bool registered(const dsv_keyset* ks) {  // (a registry lock held)
  return std::find(g_keysets.begin(), g_keysets.end(), ks) != g_keysets.end();
}
}  // namespace

int create_keyset(int scheme, size_t k, size_t capacity, bool reserved, dsv_keyset** out, const KeysetForm& form) {
  if (!out) return fail(DSV_ERR_INVALID_ARGUMENT, "null output handle");
  *out = nullptr;
  if (!scheme_ok(scheme)) return fail(DSV_ERR_INVALID_ARGUMENT, "unknown scheme %d", scheme);
  if (reserved) {
    if (capacity < k) return fail(DSV_ERR_INVALID_ARGUMENT, "capacity %zu below the %zu keys given", capacity, k);
    if (capacity > kMaxKeys - 1)
      return fail(DSV_ERR_TOO_LARGE, "capacity %zu: indices are 32-bit and DSV_KEY_NONE is taken", capacity);
  }
  if (k > kMaxKeys) return fail(DSV_ERR_TOO_LARGE, "%zu keys: indices are 32-bit", k);
  if (k)
    if (int r = form.check_pointers()) return r;
  Context* cp = nullptr;
  if (int r = current_context(cp)) return r;
  Context& ctx = *cp;
  DSV_ON_DEVICE(ctx);
  dsv_keyset* ks = new dsv_keyset();
  ks->scheme = scheme;
  ks->capacity = capacity;
  ks->device = ctx.device;
  int rc = [&]() -> int {
    if (capacity == 0) return DSV_OK;
    Scratch x;
    HIP_TRY(hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking));
    if (int r = allocate_keyset(ks, x.s)) return r;
    if (int r = register_keys(ctx, ks, 0, k, form, x)) return r;  // k keys appended to the empty set
    HIP_TRY(hipStreamSynchronize(x.s));
    return DSV_OK;
  }();
  ks->k = k;
  std::unique_lock<std::shared_mutex> lk(g_ks_mu);
  if (rc == DSV_OK && !ctx.ready.load(std::memory_order_acquire))
    rc = fail(DSV_ERR_NOT_INITIALIZED, "device %d was shut down", ctx.device);
  if (rc != DSV_OK) {
    free_device_memory(ks);
    delete ks;
    return rc;
  }
  ks->alive = true;
  g_keysets.push_back(ks);
  *out = ks;
  return DSV_OK;
}

int append_keyset(dsv_keyset* ks, size_t m, uint32_t* first_index,
                  const std::function<KeysetForm(int scheme)>& form_of) {
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  std::shared_ptr<std::mutex> mu;
  {
    std::shared_lock<std::shared_mutex> rl(g_ks_mu);
    if (!registered(ks)) return fail(DSV_ERR_INVALID_ARGUMENT, "not a live key set handle");  // (before ks is read)
    mu = ks->append_mu;
  }
  std::lock_guard<std::mutex> one_appender(*mu);
  size_t first = 0;
  {
    // shared, not exclusive: verify calls go on beside the table build; shutdown and destroy wait for it
    std::shared_lock<std::shared_mutex> rl(g_ks_mu);
    if (!registered(ks)) return fail(DSV_ERR_INVALID_ARGUMENT, "not a live key set handle");
    Context* cp = nullptr;
    if (int r = keyset_context(ks, cp)) return r;
    first = ks->k;  // (only an appender raises it, and this is the only one)
    if (m == 0) {
      if (first_index) *first_index = (uint32_t)first;
      return DSV_OK;
    }
    if (m > ks->capacity - first)
      return fail(DSV_ERR_TOO_LARGE, "%zu keys appended to %zu of capacity %zu", m, first, ks->capacity);
    const KeysetForm form = form_of(ks->scheme);
    if (int r = form.check_pointers()) return r;
    DSV_ON_DEVICE(*cp);
    Scratch x;
    HIP_TRY(hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking));
    if (int r = register_keys(*cp, ks, first, m, form, x)) return r;
  }
  // the new rows are complete and visible: calls enqueued from here on may use them
  std::unique_lock<std::shared_mutex> lk(g_ks_mu);
  if (!registered(ks) || !ks->alive)
    return fail(DSV_ERR_NOT_INITIALIZED, "the key set's device was shut down during the append");
  ks->k = first + m;
  if (first_index) *first_index = (uint32_t)first;
  return DSV_OK;
}

// the rebuild of both indices from the set's own rows, on s: the affine rows of the k keys as
// planar columns, one entry per distinct valid key at its lowest index by the append kernel at first = 0 into a
// scratch index (ws: k * np * 64 B of columns, as many of rows, the slots; carved as rebuild_bytes counts them),
// then both live slot arrays cleared and those representatives inserted in order
static size_t rebuild_bytes(const dsv_keyset* ks) {
  const size_t cols = align_up(ks->k * (size_t)keyset_points(ks->scheme) * 64, 256);
  return 2 * cols + align_up(4 * (ks->slot_mask + 1), 256);
}
static int rebuild_indices(dsv_keyset* ks, uint8_t* ws, hipStream_t s) {
  const int np = keyset_points(ks->scheme);
  const size_t k = ks->k;
  Stager x(ws);
  uint8_t* P0 = x.take(k * (size_t)np * 64);
  uint8_t* P1 = np == 2 ? P0 + k * 64 : nullptr;
  uint8_t* rows = x.take(k * (size_t)np * 64);
  uint32_t* reps = reinterpret_cast<uint32_t*>(x.take(4 * (ks->slot_mask + 1)));
  const uint8_t* own = ks->index[kKeyAffine].rows;
  launch_rows_to_planar(np, own, k, P0, P1, s);
  HIP_TRY(hipGetLastError());
  HIP_TRY(launch_clear_key_index(reps, ks->slot_mask, s));
  launch_index_append(kKeyAffine, P0, P1, ks->key_ok, np, 0, k, rows, reps, ks->slot_mask, s);
  HIP_TRY(hipGetLastError());
  for (KeyForm f : {kKeyAffine, kKeyRecord}) {
    HIP_TRY(launch_clear_key_index(ks->index[f].slots, ks->slot_mask, s));
    launch_index_reinsert(f, np, own, reps, ks->index[f].slots, ks->slot_mask, s);
    HIP_TRY(hipGetLastError());
  }
  return DSV_OK;
}

// host nanoseconds the latest replace held the registry's exclusive lock (dsv_debug_keyset_replace_exclusive_ns)
static std::atomic<uint64_t> g_replace_exclusive_ns{0};

int replace_keyset(dsv_keyset* ks, const uint32_t* indices, size_t m,
                   const std::function<KeysetForm(int scheme)>& form_of) {
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  std::shared_ptr<std::mutex> mu;
  {
    std::shared_lock<std::shared_mutex> rl(g_ks_mu);
    if (!registered(ks)) return fail(DSV_ERR_INVALID_ARGUMENT, "not a live key set handle");  // (before ks is read)
    mu = ks->append_mu;
  }
  std::lock_guard<std::mutex> one_writer(*mu);  // replaces and appends to one set take turns
  // the call's scratch, alive through both phases: the staged points and the form's own bytes, the m keys' tables
  // and key_ok, their indices, and what the rebuild works in
  Scratch x;
  uint8_t *P0 = nullptr, *P1 = nullptr, *new_ok = nullptr, *rebuild = nullptr;
  uint32_t *new_tables = nullptr, *dev_indices = nullptr;
  int np = 0;
  {
    // phase 1, shared: the new keys' tables are built beside the verify calls, as an append builds its own
    std::shared_lock<std::shared_mutex> rl(g_ks_mu);
    if (!registered(ks)) return fail(DSV_ERR_INVALID_ARGUMENT, "not a live key set handle");
    Context* cp = nullptr;
    if (int r = keyset_context(ks, cp)) return r;
    if (m == 0) return DSV_OK;
    const KeysetForm form = form_of(ks->scheme);
    if (!indices) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
    if (int r = form.check_pointers()) return r;
    const size_t k = ks->k;  // (only an appender raises it, and append_mu is held)
    if (m > k) return fail(DSV_ERR_INVALID_ARGUMENT, "%zu distinct indices cannot all lie below k = %zu", m, k);
    std::vector<uint32_t> sorted(indices, indices + m);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.back() >= k) return fail(DSV_ERR_INVALID_ARGUMENT, "index %u of %zu keys", sorted.back(), k);
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      return fail(DSV_ERR_INVALID_ARGUMENT, "an index is given twice");
    np = keyset_points(ks->scheme);
    DSV_ON_DEVICE(*cp);
    HIP_TRY(hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking));
    const size_t own_bytes = align_up((size_t)np * m * 64, 256) + align_up(form.own_bytes, 256) +
                             align_up(m * (size_t)np * kKeyPointBytes, 256) + align_up(m, 256) + align_up(4 * m, 256);
    HIP_TRY(hipMalloc(&x.dev, own_bytes + rebuild_bytes(ks)));
    Stager st(x.dev);
    P0 = st.take((size_t)np * m * 64);
    P1 = np == 2 ? P0 + m * 64 : nullptr;
    uint8_t* own = st.take(form.own_bytes);
    new_tables = reinterpret_cast<uint32_t*>(st.take(m * (size_t)np * kKeyPointBytes));
    new_ok = st.take(m);
    dev_indices = reinterpret_cast<uint32_t*>(st.take(4 * m));
    rebuild = x.dev + st.off;
    HIP_TRY(hipMemcpyAsync(dev_indices, indices, 4 * m, hipMemcpyHostToDevice, x.s));
    uint8_t* valid = nullptr;
    if (int r = form.stage(*cp, P0, own, x.s, valid)) return r;
    launch_build_key_tables(P0, P1, valid, np, m, new_tables, new_ok, x.s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(x.s));
  }
  // phase 2, exclusive: no library call is enqueueing on any key set; the device runs dry before the first byte of
  // the set changes, so a call enqueued earlier decides on the old set and a later one on the new
  std::unique_lock<std::shared_mutex> lk(g_ks_mu);
  const auto t0 = std::chrono::steady_clock::now();
  if (!registered(ks) || !ks->alive)
    return fail(DSV_ERR_NOT_INITIALIZED, "the key set's device was shut down during the replace");
  DeviceGuard guard(ks->device);
  if (guard.err != hipSuccess) return fail(DSV_ERR_HIP, "cannot select device %d", ks->device);
  HIP_TRY(hipDeviceSynchronize());
  const int rc = [&]() -> int {
    launch_replace_commit(np, dev_indices, m, new_tables, new_ok, P0, P1, ks->tables, ks->key_ok,
                          ks->index[kKeyAffine].rows, ks->index[kKeyRecord].rows, x.s);
    HIP_TRY(hipGetLastError());
    if (int r = rebuild_indices(ks, rebuild, x.s)) return r;
    HIP_TRY(hipStreamSynchronize(x.s));
    return DSV_OK;
  }();
  if (rc != DSV_OK) {  // the set may hold a mixture: it is dead from here on
    free_device_memory(ks);
    ks->alive = false;
  }
  g_replace_exclusive_ns.store(
      (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(),
      std::memory_order_relaxed);
  return rc;
}

KeysetForm keyset_form_affine(int scheme, const uint8_t* pk_uv, const uint8_t* pk2_uv, size_t m) {
  const bool two = keyset_points(scheme) == 2;
  return {[=] { return !pk_uv || (two && !pk2_uv) ? fail(DSV_ERR_INVALID_ARGUMENT, "null pointer") : DSV_OK; }, 0,
          [=](Context&, uint8_t* P, uint8_t*, hipStream_t s, uint8_t*&) {
            HIP_TRY(hipMemcpyAsync(P, pk_uv, m * 64, hipMemcpyHostToDevice, s));
            if (two) HIP_TRY(hipMemcpyAsync(P + m * 64, pk2_uv, m * 64, hipMemcpyHostToDevice, s));
            return (int)DSV_OK;
          }};
}
KeysetForm keyset_form_wire(int scheme, const uint8_t* pk_bytes, size_t m) {
  // behind the points: the records, then the decoder's verdicts
  const int np = keyset_points(scheme);
  const size_t rec = 32 * (size_t)np, off_valid = align_up(m * rec, 256);
  return {[=] { return !pk_bytes ? fail(DSV_ERR_INVALID_ARGUMENT, "null pointer") : DSV_OK; },
          off_valid + align_up(m, 256),
          [=](Context& ctx, uint8_t* P, uint8_t* own, hipStream_t s, uint8_t*& valid) {
            valid = own + off_valid;
            HIP_TRY(hipMemcpyAsync(own, pk_bytes, m * rec, hipMemcpyHostToDevice, s));
            for (int p = 0; p < np; p++)
              if (int r = decompress_on(ctx, own + 32 * p, rec, m, P + (size_t)p * m * 64, valid, p > 0, s)) return r;
            return (int)DSV_OK;
          }};
}

namespace {
// the affine form: the caller's columns as they are, no preparation launch
int verify_keyed_dev(const dsv_keyset* ks, const Items& items, const void* idx, size_t n, void* ok, void* workspace,
                     size_t workspace_bytes, void* stream) {
  return run_keyed_dev(
      ks, items.scheme, [&](int) { return keyed_any_null(items); }, [](int) { return (size_t)0; }, idx, n, ok,
      workspace, workspace_bytes, stream, [&](const Context&, int, Stager&, hipStream_t, Items& in, const uint8_t*&) {
        in = items;
        return (int)DSV_OK;
      });
}

// host arrays: chunks through the context's staging, on its null stream
int verify_keyed_host(const dsv_keyset* ks, const Items& in, const uint32_t* idx, size_t n, uint8_t* ok) {
  std::shared_lock<std::shared_mutex> rl(g_ks_mu);
  Context* cp = nullptr;
  if (int r = check_set(ks, in.scheme, n, cp)) return r;
  if (n == 0) return DSV_OK;
  if (keyed_any_null(in) || !idx || !ok) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  const int np = keyed_sig_points(in.scheme);
  const size_t chunk = n < kKeyedHostChunk ? n : kKeyedHostChunk;
  const size_t per_item = 32 + 32 + 4 + 1 + 64 * (size_t)np;
  if (int r = ensure_stage(ctx, chunk * per_item + keyed_ws_bytes(chunk) + 8 * 256)) return r;
  for (size_t off = 0; off < n; off += chunk) {
    const size_t cnt = n - off < chunk ? n - off : chunk;
    Stager st(ctx.stage);
    uint8_t* du = st.take(cnt * 32);
    uint8_t* dm = st.take(cnt * 32);
    uint8_t* di = st.take(cnt * 4);
    uint8_t* dok = st.take(cnt);
    uint8_t* dR = st.take(cnt * 64);
    uint8_t* dRp = np == 2 ? st.take(cnt * 64) : nullptr;
    void* ws = st.take(keyed_ws_bytes(cnt));
    H2D(du, in.u + off * 32, cnt * 32);
    H2D(dm, in.m + off * 32, cnt * 32);
    H2D(di, idx + off, cnt * 4);
    H2D(dR, in.R() + off * 64, cnt * 64);
    if (dRp) H2D(dRp, in.Rp() + off * 64, cnt * 64);
    enqueue_keyed(ctx, ks, make_items(in.scheme, du, {dR, dRp}, dm), (const uint32_t*)di, cnt, dok, ws, 0);
    HIP_TRY(hipGetLastError());
    D2H(ok + off, dok, cnt);
    HIP_TRY(hipStreamSynchronize(0));
  }
  return DSV_OK;
}
}  // namespace

// checks shared by the _dev and host forms (shared lock held)
int check_set(const dsv_keyset* ks, int scheme, size_t n, Context*& ctx) {
  if (int r = check_n(n)) return r;
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  if (int r = keyset_context(ks, ctx)) return r;
  if (scheme >= 0 && ks->scheme != scheme)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key set of scheme %d used with scheme %d", ks->scheme, scheme);
  return DSV_OK;
}
int check_keyed_dev(const dsv_keyset* ks, const Context* ctx, bool inputs_null, const void* idx, const void* ok,
                    const void* workspace, size_t workspace_bytes, int window_bits, size_t need) {
  if (inputs_null || !idx || !ok || !workspace) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  if (int r = check_rlc_bits(window_bits)) return r;
  if (workspace_bytes < need)
    return fail(DSV_ERR_INVALID_ARGUMENT, "workspace of %zu bytes, %zu needed", workspace_bytes, need);
  Context* octx = nullptr;
  if (int r = device_context(ok, octx)) return r;
  if (octx != ctx)
    return fail(DSV_ERR_INVALID_ARGUMENT, "key set of device %d used on device %d", ks->device, octx->device);
  return DSV_OK;
}
std::shared_mutex& keyset_mutex() { return g_ks_mu; }
// challenge hash, then the keyed kernel; every pointer device memory of ctx's device
void enqueue_keyed(const Context& ctx, const dsv_keyset* ks, const Items& in, const uint32_t* idx, size_t n,
                   uint8_t* ok, void* workspace, hipStream_t s, const uint8_t* valid_in) {
  const Workspace w = carve(workspace, n);
  launch_hash(in, n, w.c, w.valid, s, valid_in);
  launch_verify_keyed(ks->scheme, in.u, w.c, w.valid, in.R(), in.Rp(), idx, n, ks->tables, ks->key_ok, ks->k,
                      ctx.table[0], ctx.table[1], ok, s);
}


// dsv_shutdown_device: the live key sets of `device` lose their device memory (the context is released
// right after, under the same locks)
void keysets_release_device(int device) {
  std::unique_lock<std::shared_mutex> lk(g_ks_mu);
  DeviceGuard guard(device);
  free_sets_of(device);
}
}  // namespace dsvh

using namespace dsvh;

extern "C" {

size_t dsv_keyset_bytes(int scheme, size_t k) { return scheme_ok(scheme) ? keyset_total_bytes(scheme, k) : 0; }
size_t dsv_keyed_workspace_bytes(size_t n) { return keyed_ws_bytes(n); }

int dsv_keyset_create(int scheme, const uint8_t* pk_uv, const uint8_t* pk2_uv, size_t k, dsv_keyset** out) {
  return create_keyset(scheme, k, k, false, out, keyset_form_affine(scheme, pk_uv, pk2_uv, k));
}
int dsv_keyset_create_wire(int scheme, const uint8_t* pk_bytes, size_t k, dsv_keyset** out) {
  return create_keyset(scheme, k, k, false, out, keyset_form_wire(scheme, pk_bytes, k));
}
int dsv_keyset_create_reserved(int scheme, const uint8_t* pk_uv, const uint8_t* pk2_uv, size_t k, size_t capacity,
                               dsv_keyset** out) {
  return create_keyset(scheme, k, capacity, true, out, keyset_form_affine(scheme, pk_uv, pk2_uv, k));
}

int dsv_keyset_append(dsv_keyset* ks, const uint8_t* pk_uv, const uint8_t* pk2_uv, size_t m, uint32_t* first_index) {
  return append_keyset(ks, m, first_index, [=](int scheme) { return keyset_form_affine(scheme, pk_uv, pk2_uv, m); });
}
int dsv_keyset_append_wire(dsv_keyset* ks, const uint8_t* pk_bytes, size_t m, uint32_t* first_index) {
  return append_keyset(ks, m, first_index, [=](int scheme) { return keyset_form_wire(scheme, pk_bytes, m); });
}

int dsv_keyset_replace(dsv_keyset* ks, const uint32_t* indices, const uint8_t* pk_uv, const uint8_t* pk2_uv,
                       size_t m) {
  return replace_keyset(ks, indices, m, [=](int scheme) { return keyset_form_affine(scheme, pk_uv, pk2_uv, m); });
}
int dsv_keyset_replace_wire(dsv_keyset* ks, const uint32_t* indices, const uint8_t* pk_bytes, size_t m) {
  return replace_keyset(ks, indices, m, [=](int scheme) { return keyset_form_wire(scheme, pk_bytes, m); });
}
uint64_t dsv_debug_keyset_replace_exclusive_ns(void) {
  return g_replace_exclusive_ns.load(std::memory_order_relaxed);
}
int dsv_debug_keyset_slots(const dsv_keyset* ks, int form, uint32_t* out, size_t room, size_t* slots_out) {
  if (int r = library_up(ks)) return r;
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  if (form != kKeyAffine && form != kKeyRecord) return fail(DSV_ERR_INVALID_ARGUMENT, "unknown key form %d", form);
  std::shared_lock<std::shared_mutex> rl(g_ks_mu);
  Context* cp = nullptr;
  if (int r = keyset_context(ks, cp)) return r;
  const size_t slots = ks->capacity ? ks->slot_mask + 1 : 0, n = slots < room ? slots : room;
  if (slots_out) *slots_out = slots;
  if (n == 0) return DSV_OK;
  if (!out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_ON_DEVICE(*cp);
  HIP_TRY(hipMemcpy(out, ks->index[form].slots, 4 * n, hipMemcpyDeviceToHost));
  return DSV_OK;
}

int dsv_keyset_capacity(const dsv_keyset* ks, size_t* capacity) {
  if (!ks || !capacity) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  std::shared_lock<std::shared_mutex> rl(g_ks_mu);
  *capacity = ks->capacity;
  return DSV_OK;
}

int dsv_keyset_destroy(dsv_keyset* ks) {
  if (!ks) return DSV_OK;
  std::unique_lock<std::shared_mutex> lk(g_ks_mu);
  auto it = std::find(g_keysets.begin(), g_keysets.end(), ks);
  if (it == g_keysets.end()) return fail(DSV_ERR_INVALID_ARGUMENT, "not a live key set handle");
  g_keysets.erase(it);
  int rc = DSV_OK;
  if (ks->alive && ks->tables) {
    DeviceGuard guard(ks->device);
    if (guard.err != hipSuccess) rc = fail(DSV_ERR_HIP, "cannot select device %d", ks->device);
    (void)hipDeviceSynchronize();  // work in flight may still read the tables
    free_device_memory(ks);
  }
  delete ks;
  return rc;
}

int dsv_keyset_info(const dsv_keyset* ks, int* scheme, size_t* k, size_t* bytes, int* device) {
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  std::shared_lock<std::shared_mutex> rl(g_ks_mu);
  if (scheme) *scheme = ks->scheme;
  if (k) *k = ks->k;
  if (bytes) *bytes = ks->bytes;
  if (device) *device = ks->device;
  return DSV_OK;
}

int dsv_keyset_key_ok_n(const dsv_keyset* ks, uint8_t* out, size_t room, size_t* k_out) {
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  std::shared_lock<std::shared_mutex> rl(g_ks_mu);
  Context* cp = nullptr;
  if (int r = keyset_context(ks, cp)) return r;
  const size_t k = ks->k, n = k < room ? k : room;  // (one read of k: what is copied is what is reported)
  if (k_out) *k_out = k;
  if (n == 0) return DSV_OK;
  if (!out) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  DSV_ON_DEVICE(*cp);
  HIP_TRY(hipMemcpy(out, ks->key_ok, n, hipMemcpyDeviceToHost));
  return DSV_OK;
}
int dsv_keyset_key_ok(const dsv_keyset* ks, uint8_t* out) { return dsv_keyset_key_ok_n(ks, out, (size_t)-1, nullptr); }

int dsv_verify_single_keyed_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* key_idx,
                                const void* m, size_t n, void* ok, void* workspace, size_t workspace_bytes,
                                void* stream) {
  return verify_keyed_dev(ks, make_items(0, u, {R_uv}, m), key_idx, n, ok, workspace, workspace_bytes, stream);
}
int dsv_verify_double_keyed_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* Rp_uv,
                                const void* key_idx, const void* m, size_t n, void* ok, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return verify_keyed_dev(ks, make_items(1, u, {R_uv, Rp_uv}, m), key_idx, n, ok, workspace, workspace_bytes,
                          stream);
}
int dsv_verify_vargen_keyed_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* key_idx,
                                const void* m, size_t n, void* ok, void* workspace, size_t workspace_bytes,
                                void* stream) {
  return verify_keyed_dev(ks, make_items(2, u, {R_uv}, m), key_idx, n, ok, workspace, workspace_bytes, stream);
}

int dsv_verify_single_keyed(const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint32_t* key_idx,
                            const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_keyed_host(ks, make_items(0, u, {R_uv}, m), key_idx, n, ok);
}
int dsv_verify_double_keyed(const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint8_t* Rp_uv,
                            const uint32_t* key_idx, const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_keyed_host(ks, make_items(1, u, {R_uv, Rp_uv}, m), key_idx, n, ok);
}
int dsv_verify_vargen_keyed(const dsv_keyset* ks, const uint8_t* u, const uint8_t* R_uv, const uint32_t* key_idx,
                            const uint8_t* m, size_t n, uint8_t* ok) {
  return verify_keyed_host(ks, make_items(2, u, {R_uv}, m), key_idx, n, ok);
}

int dsv_debug_keyset_entry(const dsv_keyset* ks, size_t key, int point, int window, int digit, uint8_t out64[64]) {
  if (!ks || !out64) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  std::shared_lock<std::shared_mutex> rl(g_ks_mu);
  Context* cp = nullptr;
  if (int r = keyset_context(ks, cp)) return r;
  if (key >= ks->k || point < 0 || point >= keyset_points(ks->scheme) || window < 0 || window >= kKeyWindows ||
      digit < -(kKeyEntries - 1) || digit > kKeyEntries - 1)
    return fail(DSV_ERR_INVALID_ARGUMENT, "entry out of range");
  Context& ctx = *cp;
  DSV_HOST_LOCK();
  if (int r = ensure_stage(ctx, 256)) return r;
  const int mag = digit < 0 ? -digit : digit;
  const uint32_t* entry = ks->tables + (key * keyset_points(ks->scheme) + (size_t)point) * kKeyPointWords +
                          ((size_t)window * kKeyEntries + (size_t)mag) * kEntryWords;
  launch_key_entry(entry, digit < 0, ctx.stage, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(out64, ctx.stage, 64, hipMemcpyDeviceToHost));
  return DSV_OK;
}

}  // extern "C"
