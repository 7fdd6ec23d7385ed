// dsv_keyed_rlc.hip — the batch fast accept over a registered key set (keyed_rlc.h; DESIGN.md §10, "Keyed
// fast accept"): control and the dsv_verify_*_keyed_rlc_dev entry points of include/dsv.h.
//
// Per group of at most kRlcMaxGroup items, cut into sub-groups as the unkeyed fast accept cuts them
// (dsv_rlc.hip: rlc_group_plan, rlc_split_groups, dsv_debug_rlc_subgroups), all of it enqueued on the caller's
// stream: the challenge hash, the keyed prep (k_keyed_rlc.hip), k_rlc.hip's bucket pass, the keys' subgroup
// tests and terms, k_rlc.hip's tail with the key term in its identity test, then the keyed per-signature
// kernel gated by every sub-group's flag words (no work where the aggregate accepted) and the one-thread
// verdict kernel.  The keyed calls keep history counters of their own (rlc_keyed_history): an unkeyed call
// behaves as if they did not exist.  Not here: the unkeyed path's sample check and guarded second stage.
#include "keyed_rlc.h"
#include "keyset_host.h"

using namespace dsvh;

extern "C++" {
namespace dsvh {
// ksum, touched, bad back to back: one memset (launch_keyed_rlc_prep)
void carve_keyed_rlc_buffers(Stager& st, const RlcPlan& p, int scheme, size_t k, KeyedRlcBuffers& kb) {
  const size_t G = p.groups;
  kb.ksum = reinterpret_cast<unsigned long long*>(st.take(G * k * (size_t)keyed_scalars(scheme) * 8 * 8));
  kb.touched = reinterpret_cast<u32*>(st.take(G * k * sizeof(u32)));
  kb.bad = reinterpret_cast<u32*>(st.take(k * sizeof(u32)));
  kb.partial = reinterpret_cast<u32*>(st.take(G * keyed_term_blocks(k) * 36 * sizeof(u32)));
  kb.terms = reinterpret_cast<u32*>(st.take(G * 36 * sizeof(u32)));
}
}  // namespace dsvh
namespace {
// Below this many items of a group (automatic window bits) the aggregate does not pay for its latency-bound
// tail (~0.9 ms whatever the batch): the group goes to the keyed per-signature kernel as it is.  Measured (DESIGN.md
// §10, 64 keys, all valid): at 2^18 items the aggregate takes 1.36 x (single), 1.06 x (double), 1.19 x
// (var-generator) the keyed per-signature time, at 2^20 0.84 / 0.74 / 0.73 x.
size_t keyed_rlc_min_auto(int) { return (size_t)1 << 19; }

struct KeyedCarve {
  Workspace w;       // c / valid of the group, where enqueue_keyed's carve puts them
  u32* flags_area;   // kRlcFlagBlocks flag blocks: block 2 g is group g's (k_rlc_verdict's layout)
  RlcBuffers b;
  KeyedRlcBuffers kb;
  size_t bytes;
};
// nmax: items of the call's largest group; cnt: of this one
KeyedCarve carve_keyed_rlc(void* ws, size_t nmax, size_t cnt, const RlcPlan& p, int scheme, size_t k) {
  KeyedCarve r;
  r.w = carve(ws, cnt);
  Stager st(static_cast<uint8_t*>(ws) + keyed_ws_bytes(nmax));
  r.flags_area = reinterpret_cast<u32*>(st.take(kRlcFlagBlocks * kRlcGroupFlagWords * sizeof(u32)));
  r.b.flags = r.flags_area;
  carve_rlc_buffers(st, p, r.b);
  carve_keyed_rlc_buffers(st, p, scheme, k, r.kb);
  r.bytes = keyed_ws_bytes(nmax) + st.off;
  return r;
}
// the largest workspace any plan of a call of n items over k keys takes (the unkeyed rule: sized for
// min(n, 2^22) items whatever the group count, so that it never drops as n grows)
size_t keyed_rlc_workspace_for(size_t n, size_t k, int window_bits) {
  const size_t g = n < kRlcMaxGroup ? n : kRlcMaxGroup;
  // (from 2 kSplitItems items on, sub-groups are whole sub-batches: fewer and larger — the finer cut just
  //  below takes more buffers, and the size must not drop there)
  const size_t fine = g < 2 * kSplitItems ? g : 2 * kSplitItems - 1;
  size_t most = 0;
  for (const size_t items : {g, fine})
    for (int G = 1; G <= kRlcMaxSub; G++) {
      // the double scheme's needs: two nonce points, two fixed-base terms, two scalars per key
      const RlcPlan p = rlc_group_plan(1, items, window_bits, G, true);
      const size_t b = carve_keyed_rlc(reinterpret_cast<void*>((uintptr_t)4096), g, items, p, 1, k).bytes;
      most = b > most ? b : most;
    }
  return most;
}

// enqueues everything on `s`; *accepted_dev (device-accessible, may be null) = every group was decided by its aggregates
int keyed_rlc_on(Context& ctx, const dsv_keyset* ks, const Items& in, const uint32_t* idx, size_t n, uint8_t* ok,
                 void* workspace, hipStream_t s, int window_bits, u32* accepted_dev, u32* history_words) {
  const int scheme = in.scheme;
  const size_t group = rlc_group_items(n);
  const int force_groups = rlc_forced_groups();
  const u32 history = *reinterpret_cast<volatile u32*>(history_words);  // (written by the verdict kernels; never waited for)
  // (the caller holds the registry's shared lock: one k for the whole call, whatever an append does meanwhile)
  const KeyedRlcKeys keys{ks->tables, ks->key_ok, ks->k};
  RlcVerdictArgs va = {};
  u32* flags_area = nullptr;
  for (size_t off = 0, g = 0; off < n; off += group, g++) {
    const size_t cnt = n - off < group ? n - off : group;
    if (g >= kRlcMaxGroupsPerCall) return fail(DSV_ERR_TOO_LARGE, "more than %zu groups", kRlcMaxGroupsPerCall);
    va.ngroups = (u32)g + 1;
    const Items gin = in.at(off);
    if (!window_bits && cnt < keyed_rlc_min_auto(scheme)) {
      va.subs[g] = 0;  // (the verdict kernel: not decided by an aggregate)
      enqueue_keyed(ctx, ks, gin, idx + off, cnt, ok + off, workspace, s);
      continue;
    }
    const int G = force_groups > 0 ? force_groups : (history > 0 ? rlc_split_groups(cnt, window_bits) : 1);
    const RlcPlan plan = rlc_group_plan(scheme, cnt, window_bits, G, true);
    KeyedCarve cv = carve_keyed_rlc(workspace, group, cnt, plan, scheme, keys.k);
    flags_area = cv.flags_area;
    cv.b.flags = cv.flags_area + (2 * g) * kRlcGroupFlagWords;
    va.subs[g] = (uint8_t)plan.groups;
    va.second[g] = 0;
    ChaChaKey key;
    if (int r = rlc_random_key(key)) return r;
    HIP_TRY(launch_rlc_begin(cv.b, s));
    launch_hash(gin, cnt, cv.w.c, cv.w.valid, s);
    RlcInputs ri = {};
    ri.u = gin.u, ri.c = cv.w.c, ri.valid = cv.w.valid;
    ri.r[0] = gin.R(), ri.r[1] = gin.Rp();
    HIP_TRY(launch_keyed_rlc_prep(scheme, plan, cv.b, cv.kb, ri, idx + off, keys, key, ok + off, s));
    // The keys' terms (a few dozen dependent point operations on a few workgroups: ~0.2 ms of latency at 64
    // keys) need only the prep: they run on an internal stream beside the bucket pass and join before the tail
    // (the split path's lane of this caller's stream; its events are recorded and waited for under the lane lock)
    SplitLane* lane = nullptr;
    if (ctx.split && acquire_lane(ctx, s, lane) == DSV_OK) {
      std::lock_guard<std::mutex> lk(ctx.lane_mu);
      HIP_TRY(hipEventRecord(lane->fork, s));
      HIP_TRY(hipStreamWaitEvent(lane->stream[0], lane->fork, 0));
      HIP_TRY(launch_keyed_rlc_terms(scheme, plan, cv.b, cv.kb, keys, lane->stream[0]));
      HIP_TRY(hipEventRecord(lane->join[0], lane->stream[0]));
      HIP_TRY(launch_rlc_sort(plan, cv.b, false, s));
      HIP_TRY(hipStreamWaitEvent(s, lane->join[0], 0));
    } else {
      HIP_TRY(launch_rlc_sort(plan, cv.b, false, s));
      HIP_TRY(launch_keyed_rlc_terms(scheme, plan, cv.b, cv.kb, keys, s));
    }
    HIP_TRY(launch_rlc_finish(plan, cv.b, ctx.table[0], ctx.table[1], false, s, cv.kb.terms));
    launch_keyed_fallback(scheme, plan, gin.u, cv.w.c, cv.w.valid, gin.R(), gin.Rp(), idx + off, keys, ctx.table[0],
                          ctx.table[1], ok + off, cv.b.flags, s);
    HIP_TRY(hipGetLastError());
  }
  if (!flags_area)  // (every group went to the per-signature kernel: the flag blocks' place does not depend on the plan)
    flags_area = carve_keyed_rlc(workspace, group, group, rlc_group_plan(scheme, group, 8, 1, true), scheme, keys.k).flags_area;
  launch_rlc_verdict(flags_area, va, accepted_dev, history_words, s);
  HIP_TRY(hipGetLastError());
  return DSV_OK;
}

int verify_keyed_rlc_dev(const dsv_keyset* ks, const Items& in, const void* idx, size_t n, void* ok, void* workspace,
                         size_t workspace_bytes, void* stream, int window_bits, int* accepted) {
  const hipStream_t s = (hipStream_t)stream;
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  Context* cp = nullptr;
  if (int r = check_set(ks, in.scheme, n, cp)) return r;
  if (int r = refuse_capture(s, "the keyed fast accept")) return r;
  if (n == 0) return rlc_clear_accepted(accepted);
  // (0 bytes for window bits out of range: check_keyed_dev looks at the bits first)
  if (int r = check_keyed_dev(ks, cp, keyed_any_null(in), idx, ok, workspace, workspace_bytes, window_bits,
                              dsv_keyed_rlc_workspace_bytes(n, ks->k, window_bits)))
    return r;
  Context& ctx = *cp;
  DSV_ON_DEVICE(ctx);
  u32* history_words = rlc_keyed_history(ctx);
  if (!history_words) return fail(DSV_ERR_HIP, "no pinned memory for the keyed history counters");
  RlcVerdictTarget vt;
  if (int r = rlc_verdict_target(ctx, accepted, vt)) return r;
  if (int r = keyed_rlc_on(ctx, ks, in, (const uint32_t*)idx, n, (uint8_t*)ok, workspace, s, window_bits, vt.dev,
                           history_words))
    return r;
  return rlc_verdict_wait(vt, s);
}
}  // namespace
}  // extern "C++"

extern "C" {

size_t dsv_keyed_rlc_workspace_bytes(size_t n, size_t k, int window_bits) {
  if (window_bits && !rlc_bits_ok(window_bits)) return 0;
  if (n == 0) return 256;
  return keyed_rlc_workspace_for(n, k, window_bits) + 256;
}

// out[24]: the fields of dsv_rlc_plan_info, of the keyed plan; out[23] = workspace bytes of this plan for k keys
int dsv_keyed_rlc_plan_info(int scheme, size_t n, size_t k, int window_bits, int groups, uint64_t* out) {
  if (!out || !scheme_ok(scheme) || n == 0 || n > kRlcMaxGroup || groups < 0 || groups > kRlcMaxSub)
    return fail(DSV_ERR_INVALID_ARGUMENT, "bad argument");
  if (int r = check_rlc_bits(window_bits)) return r;
  const RlcPlan p = rlc_group_plan(scheme, n, window_bits, groups, true);
  rlc_plan_words(p, carve_keyed_rlc(reinterpret_cast<void*>((uintptr_t)4096), n, n, p, scheme, k).bytes, out);
  return DSV_OK;
}

int dsv_verify_single_keyed_rlc_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* key_idx,
                                    const void* m, size_t n, void* ok, void* workspace, size_t workspace_bytes,
                                    void* stream, int window_bits, int* accepted) {
  return verify_keyed_rlc_dev(ks, make_items(0, u, {R_uv}, m), key_idx, n, ok, workspace, workspace_bytes, stream,
                              window_bits, accepted);
}
int dsv_verify_double_keyed_rlc_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* Rp_uv,
                                    const void* key_idx, const void* m, size_t n, void* ok, void* workspace,
                                    size_t workspace_bytes, void* stream, int window_bits, int* accepted) {
  return verify_keyed_rlc_dev(ks, make_items(1, u, {R_uv, Rp_uv}, m), key_idx, n, ok, workspace, workspace_bytes,
                              stream, window_bits, accepted);
}
int dsv_verify_vargen_keyed_rlc_dev(const dsv_keyset* ks, const void* u, const void* R_uv, const void* key_idx,
                                    const void* m, size_t n, void* ok, void* workspace, size_t workspace_bytes,
                                    void* stream, int window_bits, int* accepted) {
  return verify_keyed_rlc_dev(ks, make_items(2, u, {R_uv}, m), key_idx, n, ok, workspace, workspace_bytes, stream,
                              window_bits, accepted);
}

}  // extern "C"
