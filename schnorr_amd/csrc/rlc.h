// rlc.h — geometry and launchers of k_rlc.hip (random-linear-combination fast accept, SURVEY.md
// §8(f)-4), shared with the host side (dsv_rlc.hip).  Kept out of launch.h: that header is part of the
// dominant kernel's translation unit, whose sources are what the recorded roofline evidence is
// valid for (schnorr_amd/build.py: unit_sources_sha256).
#pragma once
#include "launch.h"

namespace dsv {

// One GROUP of at most kRlcMaxGroup items is decided by `groups` independent aggregates over SUB-GROUPS of
// `sub` consecutive items each (the last one may be shorter).  groups == 1 is the steady state of a caller
// whose batches are valid; after a rejected group the host cuts the next ones into several sub-groups
// (dsv_rlc.hip), so that one wrong signature sends only its own sub-group to the per-signature kernels.
// All sub-groups run through ONE set of launches (blockIdx.y = sub-group): the latency-bound tail of an
// aggregate (~250 dependent point operations on 13 workgroups) is paid once, not per sub-group.
//
// Per sub-group, c-bit unsigned windows: wpk windows over the 252-bit scalars z_i c_i of the keys, wr
// windows over the 128-bit z_i of the nonce points (separate buckets: k_rlc.hip says why).  A window's
// 2^c buckets are a 2^half x 2^half matrix; row / column sums run in nseg segments, the per-bit subset
// sums over them in nseg2 segments, so that no serial chain exceeds ~32 additions.
//
// Buckets are filled from a two-pass partition of the digits (k_rlc_part1 / k_rlc_part2): every (window,
// point slot) pair owns one ROW of `row_stride` 16-bit digits; pass 1 scatters a row's entries into
// `1 << coarse_bits` BINS per window by the digit's high bits (workgroup-aggregated reservations), pass 2
// sorts one bin — 2^fine_bits buckets, a few thousand entries — by the low bits through LDS and writes
// every bucket's run (start, count).  The digits are uniform by construction (secret random weights), so a
// bin of `bin_cap` = mean + 8 sigma slots never overflows on inputs a caller can produce; if one does, the
// entries beyond it are dropped and the sub-group is flagged (kRlcOverflow): it takes the per-signature path.
struct RlcPlan {
  uint32_t n;             // items of this bucket pass ...
  uint32_t first, total;  // ... which are items first .. first + n of a sub-group of `total` (groups == 1 only: a host
                          // call may run its bucket pass in two ranges, the first while the second is still on the bus)
  uint32_t groups, sub;   // sub-groups; items of each but the last
  uint32_t items;         // items of the whole group
  int lpts, spts, fixed;  // per item: points with 252-bit scalars, points with the z themselves, fixed-base terms
  int c, half, wpk, wr, windows, nseg, nseg2;
  int fine_bits, coarse_bits;
  uint32_t kmul;        // floor(2^(wpk c) / r): the keys' scalars get a random multiple of r below it added
  uint32_t rows;        // wpk * lpts + wr * spts digit rows per sub-group
  uint32_t row_stride;  // digits per row (sub rounded up to 8: rows start 16-byte aligned)
  uint32_t bins;        // windows << coarse_bits
  uint32_t bin_cap;     // entries a bin can take
  size_t entries;       // n * rows (digit, point) pairs of this pass
  size_t buckets;       // windows << c
};
constexpr size_t kRlcMaxGroup = (size_t)1 << 22;  // point indices (at most 4 per item) are packed into 24 bits
constexpr int kRlcMaxSub = 16;                    // sub-groups per group: at most
// below this an aggregate is slower than the per-signature kernels (its tail does not shrink with the
// batch): with automatic window bits such groups skip it.  The host forms (typed objects, records in host
// memory) use kRlcMinAuto for every scheme; device-resident calls rlc_min_auto(scheme): a double or
// var-generator signature is twice the per-signature work, and their kernels are latency-bound below 2^16
// items (r06, same box, all valid, 12-bit windows: double 2^14 items 1.15 x, 2^15 1.39 x, 2^16 1.40 x;
// var-generator 1.28 / 1.25 / 1.23 x; single 2^16 items 0.96 x, 2^17 1.36 x)
constexpr size_t kRlcMinAuto = (size_t)1 << 17;
inline size_t rlc_min_auto(int scheme) { return scheme == 0 ? kRlcMinAuto : (size_t)1 << 14; }
constexpr int kRlcFsumBlocks = 256;  // (64-thread workgroups riding on k_rlc_sum<0>: 64 of them took longer than the sums themselves)
constexpr int kRlcTile = 8192;  // digits one workgroup of k_rlc_part1 partitions
// flags of one sub-group (4 words): [0] defects, [1] = 1 once the chain of kernels ran to its end.
// A sub-group is ACCEPTED iff [0] == 0 and [1] == 1: the per-signature kernels launched behind the
// aggregate take a pointer to these words as their `gate` (launch.h) and return at once when it says so.
enum : uint32_t { kRlcOffCurve = 1, kRlcTorsion = 2, kRlcSum = 4, kRlcOverflow = 8 };
// the flag block of one group: word 0 = "skip the aggregate" (the sample found a wrong item), words
// 4 + 4 g .. the flags of sub-group g
constexpr int kRlcGroupFlagWords = 4 + 4 * kRlcMaxSub;
constexpr size_t kRlcMaxGroupsPerCall = 64;  // DSV_MAX_BATCH / kRlcMaxGroup
// a group owns TWO flag blocks: [2k] its aggregate(s), [2k + 1] the sub-group aggregates of a second stage that
// runs only where the first one rejected (dsv_rlc.hip: "guarded" calls)
constexpr size_t kRlcFlagBlocks = 2 * kRlcMaxGroupsPerCall;
inline int rlc_default_bits(size_t n) {
  // (r06, all valid, same box: 2^19 items 3.005 ms at 14 bits, 3.068 at 16; 2^17 items 1.318 at 14, 1.341 at 12,
  //  1.497 at 16; 2^16 items 1.070 at 12, 1.081 at 14; 2^15 items 0.983 at 12, 1.456 at 8)
  return n >= ((size_t)1 << 20) ? 16 : n >= ((size_t)1 << 17) ? 14 : n >= ((size_t)1 << 14) ? 12 : 8;
}
// even, and the keys' windows cover 252 or 256 bits exactly (10 would need 260: a ninth scalar word)
inline bool rlc_bits_ok(int c) { return c == 4 || c == 6 || c == 8 || c == 12 || c == 14 || c == 16; }
// the plan of a range [first, first + cnt) of a group planned as `whole` (one sub-group): same bucket
// geometry, fewer pairs
inline RlcPlan rlc_range(const RlcPlan& whole, size_t first, size_t cnt) {
  RlcPlan p = whole;
  p.n = (uint32_t)cnt;
  p.first = (uint32_t)first;
  p.entries = cnt * (size_t)p.rows;
  return p;
}
// scheme: 0 single, 1 double, 2 var-generator (k_rlc.hip: k_rlc_prep says which point gets which scalar);
// `items` in `groups` sub-groups (of ceil(items / groups) items rounded up to `align`; fewer sub-groups if
// that leaves some empty).  keyed: the pass of a registered key set (keyed_rlc.h) — the keys' terms are one
// fixed-base product per key outside the buckets, so only the nonce points have rows: no key windows
// (wpk = 0, lpts = 0), the fixed-base terms on G / G' as in the unkeyed plan
inline RlcPlan rlc_plan(int scheme, size_t items, int c, int groups = 1, size_t align = 1, bool keyed = false) {
  RlcPlan p;
  if (groups < 1) groups = 1;
  if (groups > kRlcMaxSub) groups = kRlcMaxSub;
  size_t sub = (items + groups - 1) / groups;
  sub = (sub + align - 1) / align * align;
  if (sub > items) sub = items;
  if (sub == 0) sub = 1;
  p.groups = items ? (uint32_t)((items + sub - 1) / sub) : 1u;
  p.sub = (uint32_t)sub;
  p.items = (uint32_t)items;
  p.n = p.sub;
  p.first = 0;
  p.total = p.sub;
  p.lpts = keyed ? 0 : (scheme == 0 ? 1 : 2);
  p.spts = scheme == 1 ? 2 : 1;
  p.fixed = scheme == 0 ? 1 : (scheme == 1 ? 2 : 0);
  p.c = c;
  p.half = c / 2;
  p.wpk = keyed ? 0 : (252 + c - 1) / c;
  p.wr = (128 + c - 1) / c;
  p.windows = p.wpk + p.wr;
  const int side = 1 << p.half;
  p.nseg = side >= 32 ? side / 16 : 1;
  p.nseg2 = side >= 64 ? side / 32 : 1;
  p.kmul = p.wpk * c == 256 ? 17u : 1u;  // floor(2^256 / r) = 17, floor(2^252 / r) = 1
  p.fine_bits = c < 8 ? c : 8;
  p.coarse_bits = c - p.fine_bits;
  p.rows = (uint32_t)(p.wpk * p.lpts + p.wr * p.spts);
  p.row_stride = (uint32_t)((sub + 7) / 8 * 8);
  p.bins = (uint32_t)p.windows << p.coarse_bits;
  {
    // a window holds at most max(lpts, spts) * sub entries, spread uniformly over its bins
    const size_t most = (size_t)(p.lpts > p.spts ? p.lpts : p.spts) * sub;
    size_t cap = most;
    if (p.coarse_bits) {
      // (the TOP window of the keys' scalars is uniform over [0, kmul r / 2^((wpk - 1) c)) only — 0.905 of
      //  the digits when wpk c = 252, 0.962 when it is 256 —: its bins take up to 1.105 x the mean)
      const size_t mean = (most >> p.coarse_bits) * 9 / 8 + 1;
      size_t root = 1;
      while (root * root < mean) root++;
      cap = mean + 8 * root + 64;
      if (cap > most) cap = most;
    }
    p.bin_cap = (uint32_t)((cap + 63) / 64 * 64);
  }
  p.entries = sub * (size_t)p.rows;
  p.buckets = (size_t)p.windows << c;
  return p;
}
struct RlcInputs {
  const uint8_t* u;
  const uint8_t* c;      // k_challenge's output for the group
  const uint8_t* valid;  // ... and its validity bytes
  const uint8_t* pk[2];  // PK, PK' (double)
  const uint8_t* r[2];   // R, R' (double)
  const uint8_t* gen;    // Gen (var-generator)
};
// Device buffers of one group; every array holds `groups` sub-groups `*_stride` elements apart.
struct RlcBuffers {
  uint32_t* pts;       // (lpts + spts) sub x 32 words: the long points, then the negated short ones, as affine niels
  uint32_t* fsc;       // fixed x sub x 8 words: z_i u_i mod r (z'_i u_i)
  uint32_t* fpart;     // 2 x kRlcFsumBlocks x 8 words per sub-group
  uint32_t* fsum;      // 2 x 8 words per sub-group
  uint16_t* digits;    // rows x row_stride: the window digits (0: the entry enters no bucket)
  uint32_t* counters;  // bins (entries of each bin) + 256 (buckets of each run length) + 256 (cursors of k_rlc_order)
  uint32_t* binned;    // bins x bin_cap: (low digit bits << 24 | point index), bin by bin
  uint32_t* sorted;    // bins x bin_cap: point indices, bucket by bucket inside each bin
  uint32_t* start;     // buckets: first entry of the bucket's run in `sorted`
  uint32_t* cnt;       // buckets: its length
  uint32_t* order;     // buckets: bucket numbers, longest run first
  uint32_t* buckets;   // buckets x 36 words (extended niels)
  uint32_t* buckets2;  // the same for a second range (groups == 1)
  uint32_t* tmp[2];    // rlc_tmp_points(p, k) x 36 words
  uint32_t* flags;     // kRlcGroupFlagWords of this group
  size_t pts_stride, fsc_stride, digits_stride, counters_stride, bin_stride, bucket_stride, tmp_stride[2];  // in elements
};
inline size_t rlc_tmp_points(const RlcPlan& p, int k) {
  const size_t side = (size_t)1 << p.half, w = (size_t)p.windows;
  if (k == 0) {
    size_t a = w * 2 * side * p.nseg, b = w * 2 * p.half * p.nseg2, c = w * p.c + 1;
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
  }
  const size_t a = w * 2 * side, b = w * p.c;
  return a > b ? a : b;
}
// One aggregate from the hash output c / valid of the group `in` (ok[i] = "item i is well-formed", flags out), in
// pieces that never synchronise and return the first error of a launch: begin (flags), the bucket pass of one
// range into b.buckets (second = false) or b.buckets2, and the rest over the whole group (`merged`: the two bucket
// arrays are added first)
hipError_t launch_rlc_begin(const RlcBuffers& b, hipStream_t s);
hipError_t launch_rlc_buckets(int scheme, const RlcPlan& range, const RlcBuffers& b, const RlcInputs& in,
                              ChaChaKey key, uint8_t* ok, bool second, hipStream_t s);
// key_terms (may be null): one extended-niels point per sub-group that the tail adds to its sum before the
// identity test (keyed_rlc.h: the registered keys' terms)
hipError_t launch_rlc_finish(const RlcPlan& whole, const RlcBuffers& b, const uint32_t* tableG,
                             const uint32_t* tableG2, bool merged, hipStream_t s, const uint32_t* key_terms = nullptr);
// the bucket pass after the prep: partition, runs, order, accumulation (b.counters zeroed beforehand)
hipError_t launch_rlc_sort(const RlcPlan& p, const RlcBuffers& b, bool second, hipStream_t s);
// The sample check, on the device: flags[0] of the group = 1 ("skip the aggregate") when one of the `count`
// items from `first` on is well-formed (valid byte set, u < r, every key coordinate < q) and still has
// verdict 0 in sample_ok — a WRONG signature; malformed ones do not count, they stay out of the sum.
// pk1: PK' / Gen, or null.
void launch_rlc_sample_decide(const uint8_t* sample_ok, const uint8_t* valid, const uint8_t* u, const uint8_t* pk0,
                              const uint8_t* pk1, size_t first, size_t count, uint32_t* flags, hipStream_t s);
// The call's verdict from the flag blocks of its groups (kRlcGroupFlagWords apart): *accepted = every
// sub-group of every group accepted (device-accessible memory, may be null); `history` (may be null; pinned
// host memory the context owns): [0] = 8 and [2] = 128 after a call with a rejected sub-group, one less each (not
// below 0) after a call whose aggregates all accepted, unchanged if the call ran none; [1] += 1.
struct RlcVerdictArgs {
  uint32_t ngroups;
  uint32_t and_into;                     // *accepted &= ... (the second kind of a mixed batch)
  uint8_t subs[kRlcMaxGroupsPerCall];    // sub-groups of each group's DECISIVE stage; 0: the group took the per-signature path as it is
  uint8_t second[kRlcMaxGroupsPerCall];  // 1: the decisive flag block is the group's second one
};
void launch_rlc_verdict(const uint32_t* flags, RlcVerdictArgs a, uint32_t* accepted, uint32_t* history, hipStream_t s);
// Between the two stages of a guarded group: if the first stage's (single) aggregate ACCEPTED, mark the second
// stage's block "skip" and its `subs` sub-groups accepted — its kernels and the per-signature launches gated by
// it then return at once; else leave it zeroed: the second stage runs.  One thread; `second` zeroed beforehand.
void launch_rlc_chain(const uint32_t* first, uint32_t* second, uint32_t subs, hipStream_t s);

}  // namespace dsv

#ifdef DSV_RLC_KERNELS
// ---- device helpers of the bucket pass, shared by k_rlc.hip and k_keyed_rlc.hip ------------------------
#include "common.h"
#include "stdrng.h"

namespace dsv {

namespace {
constexpr int kPtWords = 32;     // affine niels (v+u, v-u, 2d*uv): 27 words, padded to one 128-byte line
constexpr int kNielsWords = 36;  // (v+u, v-u, z, 2d*t)

// signed binary expansion of r (non-adjacent form, 85 non-zero digits, top digit +2^252):
// r = kRNafPos - kRNafNeg, checked at compile time below
__device__ constexpr u32 kRNafPos[8] = {0x00004100u, 0x10a01080u, 0x11081084u, 0xa8882094u,
                                        0x01444000u, 0x08884001u, 0x85440029u, 0x1080050au};
__device__ constexpr u32 kRNafNeg[8] = {0x29091449u, 0x40090221u, 0x44400001u, 0x02200000u,
                                        0x00100500u, 0x02210500u, 0x20105080u, 0x02025020u};
constexpr u32 kRWords[8] = DSV_R32;
constexpr bool naf_is_r() {
  const u32 pos[8] = {0x00004100u, 0x10a01080u, 0x11081084u, 0xa8882094u, 0x01444000u, 0x08884001u, 0x85440029u, 0x1080050au};
  const u32 neg[8] = {0x29091449u, 0x40090221u, 0x44400001u, 0x02200000u, 0x00100500u, 0x02210500u, 0x20105080u, 0x02025020u};
  u64 borrow = 0;
  for (int i = 0; i < 8; i++) {
    const u64 d = (u64)pos[i] - neg[i] - borrow;
    if ((u32)d != kRWords[i]) return false;
    borrow = (d >> 63) & 1;
    if (pos[i] & neg[i]) return false;
  }
  return borrow == 0;
}
static_assert(naf_is_r(), "kRNafPos - kRNafNeg must be the subgroup order r");

DSV_DEV void fr_add(u32 (&out)[8], const u32 (&a)[8], const u32 (&b)[8]) {  // a + b mod r (a, b < r)
  u32 s[8], d[8];
  u32 carry = 0, borrow = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const u64 y = (u64)a[j] + b[j] + carry;
    s[j] = (u32)y;
    carry = (u32)(y >> 32);
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const u64 y = (u64)s[j] - kR32[j] - borrow;
    d[j] = (u32)y;
    borrow = (u32)(y >> 63);
  }
  const bool ge = borrow == 0;  // (r < 2^252: a + b never carries out of 256 bits)
#pragma unroll
  for (int j = 0; j < 8; j++) out[j] = ge ? d[j] : s[j];
}

DSV_DEV void store_pt(u32* p, const ANiels& n) {
  uint4* q = reinterpret_cast<uint4*>(p);
  u32 w[28];
#pragma unroll
  for (int i = 0; i < NL; i++) {
    w[i] = n.vpu.l[i];
    w[NL + i] = n.vmu.l[i];
    w[2 * NL + i] = n.t2d.l[i];
  }
  w[27] = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) q[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
DSV_DEV ANiels load_pt(const u32* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  u32 w[28];
#pragma unroll
  for (int k = 0; k < 7; k++) {
    const uint4 x = q[k];
    w[4 * k] = x.x, w[4 * k + 1] = x.y, w[4 * k + 2] = x.z, w[4 * k + 3] = x.w;
  }
  ANiels n;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    n.vpu.l[i] = w[i];
    n.vmu.l[i] = w[NL + i];
    n.t2d.l[i] = w[2 * NL + i];
  }
  return n;
}
DSV_DEV void store_niels(u32* p, const Niels& n) {
  uint4* q = reinterpret_cast<uint4*>(p);
  u32 w[kNielsWords];
#pragma unroll
  for (int i = 0; i < NL; i++) {
    w[i] = n.vpu.l[i];
    w[NL + i] = n.vmu.l[i];
    w[2 * NL + i] = n.z.l[i];
    w[3 * NL + i] = n.t2d.l[i];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) q[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}
DSV_DEV Niels load_niels(const u32* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  u32 w[kNielsWords];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const uint4 x = q[k];
    w[4 * k] = x.x, w[4 * k + 1] = x.y, w[4 * k + 2] = x.z, w[4 * k + 3] = x.w;
  }
  Niels n;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    n.vpu.l[i] = w[i];
    n.vmu.l[i] = w[NL + i];
    n.z.l[i] = w[2 * NL + i];
    n.t2d.l[i] = w[3 * NL + i];
  }
  return n;
}
DSV_DEV Niels niels_neg(const Niels& n) {
  Niels r;
  r.vpu = n.vmu;
  r.vmu = n.vpu;
  r.z = n.z;
  r.t2d = fe_neg2(n.t2d);
  return r;
}

// -u^2 + v^2 == 1 + d u^2 v^2, as 2 v^2 == 2 u^2 + 2 + (2d) u^2 v^2 (u, v: fe_mul outputs)
DSV_DEV bool on_curve(const Fe& u, const Fe& v) {
  const Fe uu = fe_sqr(u), vv = fe_sqr(v);
  const Fe rhs = fe_mul(fe_mul(uu, vv), fe_const(kD2));
  const Fe a = fe_carry(fe_dbl(vv));                                           // < 3q
  const Fe b0 = fe_carry(fe_add(fe_dbl(uu), fe_dbl(fe_one())));                // < 5q
  const Fe b = fe_carry(fe_add(b0, rhs));                                      // < 6.5q, limbs < 2^29 + 8
  return fe_equal(a, b);
}
// (v+u, v-u, 2d*uv) of (u, v), or of (-u, v) — forms as ext_to_niels stores them
DSV_DEV ANiels affine_niels(const Fe& u, const Fe& v, bool negate) {
  ANiels n;
  const Fe s = fe_carry(fe_add(v, u)), d = fe_sub2(v, u);
  const Fe t = fe_mul(fe_mul(u, v), fe_const(kD2));
  n.vpu = negate ? d : s;
  n.vmu = negate ? s : d;
  n.t2d = negate ? fe_neg2(t) : t;
  return n;
}
}  // namespace

// ---- per item ---------------------------------------------------------------------------------
namespace {
// which items a workgroup's sub-group covers (rlc.h: RlcPlan)
struct SubView {
  u32 g;      // the sub-group (blockIdx.y)
  u32 base;   // its first item in the group's arrays
  u32 first;  // first item of this pass inside the sub-group
  u32 n;      // items of this pass
  u32 total;  // items of the sub-group
};
DSV_DEV SubView sub_view(const RlcPlan& p) {
  SubView v;
  v.g = blockIdx.y;
  if (p.groups == 1) {
    v.base = 0, v.first = p.first, v.n = p.n, v.total = p.total;
  } else {
    v.base = v.g * p.sub;
    const u32 left = p.items - v.base;
    v.total = left < p.sub ? left : p.sub;
    v.first = 0, v.n = v.total;
  }
  return v;
}
struct PrepOut {
  size_t gi;  // the item's place in the group's arrays (inputs, ok)
  u32 i;      // ... in its sub-group (points, weights)
  u32 il;     // ... and in the range this pass covers (the digit rows)
  u32 total;  // items of the sub-group
  const RlcPlan& p;
  u32* pts;
  uint16_t* digits;
};
// loads one point, folds its range check into `good`, returns "is on the curve", stores it as affine niels
DSV_DEV bool prep_point(const PrepOut& o, const uint8_t* __restrict__ uv, int slot, bool negate, bool& good) {
  Fe pu, pv;
  good &= load_fq(pu, uv, 2 * o.gi);
  good &= load_fq(pv, uv, 2 * o.gi + 1);
  store_pt(o.pts + ((size_t)slot * o.total + o.i) * kPtWords, affine_niels(pu, pv, negate));
  return on_curve(pu, pv);
}
// e' = e + k r, k uniform below floor(2^(wpk c) / r): the same multiple of a point of the prime-order
// subgroup (any other point fails the subgroup test anyway), but uniform over ALL wpk * c bits —
// without it the top window of a 252-bit scalar has a few thousand (c = 16: 2^12) digits only, and
// its buckets get runs 16 times as long as the others: a lane per bucket would wait for those.
// Then one digit per window into the point's row of that window (digit 0: the entry enters no bucket).
DSV_DEV void emit_long(const PrepOut& o, u32 (&e)[8], u32 kr, int slot) {
  const RlcPlan& p = o.p;
  u64 carry = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const u64 t = (u64)kR32[k] * kr + e[k] + carry;
    e[k] = (u32)t;
    carry = t >> 32;
  }
  const u32 mask = (1u << p.c) - 1u;
#pragma unroll 1
  for (int w = 0; w < p.wpk; w++) {
    const u32 d = e[0] & mask;
#pragma unroll
    for (int k = 0; k < 7; k++) e[k] = __funnelshift_r(e[k], e[k + 1], p.c);
    e[7] >>= p.c;
    o.digits[(size_t)(w * p.lpts + slot) * p.row_stride + o.il] = (uint16_t)d;
  }
}
DSV_DEV void emit_short(const PrepOut& o, const u32 (&zz)[8], int slot) {
  const RlcPlan& p = o.p;
  u32 z[5] = {zz[0], zz[1], zz[2], zz[3], zz[4]};
  const u32 mask = (1u << p.c) - 1u;
  const size_t first = (size_t)p.wpk * p.lpts;
#pragma unroll 1
  for (int w = 0; w < p.wr; w++) {
    const u32 d = z[0] & mask;
#pragma unroll
    for (int k = 0; k < 4; k++) z[k] = __funnelshift_r(z[k], z[k + 1], p.c);
    z[4] >>= p.c;
    o.digits[(first + (size_t)(w * p.spts + slot)) * p.row_stride + o.il] = (uint16_t)d;
  }
}
// wr * c >= 128 random bits from five keystream words: every window of z is uniform
DSV_DEV void draw_z(u32 (&z)[8], const u32* blk, int zbits, bool good) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int left = zbits - 32 * k;
    const u32 m = left >= 32 ? ~0u : (left > 0 ? (1u << left) - 1u : 0u);
    z[k] = (good && k < 5) ? (blk[k] & m) : 0u;
  }
}
}  // namespace

}  // namespace dsv
#endif
