// k_keyed_rlc.hip — the batch fast accept over a registered key set (keyed_rlc.h says what it proves).
// Kernels (launch order; blockIdx.y = the sub-group; the bucket pass and the tail between them are
// k_rlc.hip's, through their launchers):
//   k_keyed_rlc_prep     per item: eligibility, weights, -R (-R') as points and digit rows, z u (fixed-base
//                        terms), and the per-key sums: in LDS first for small sets, one flush per touched key
//   [k_rlc_part1 .. k_rlc_accumulate]
//   k_keyed_rlc_torsion  r * P == O for every point of every referenced key, eight lanes per point
//   k_keyed_rlc_terms    s_k PK_k (...) per (sub-group, key), eight lanes per key, summed per workgroup
//   k_keyed_rlc_reduce   the workgroups' sums -> one point per sub-group
//   [k_rlc_sum<0..3>, k_rlc_scale: the key term enters the final identity test]
//   k_keyed_fallback     the keyed per-signature kernel, gated by the sub-group's flag words
#define DSV_RLC_KERNELS 1
#define DSV_KEYED_KERNELS 1
#include "keyed.h"
#include "keyed_rlc.h"

namespace dsv {

namespace {
// sum_j x_j 2^(32 j) mod r for eight chunks x_j < 2^54 (at most 2^22 terms of 32 bits each)
DSV_DEV void reduce_key_sum(u32 (&s)[8], const unsigned long long* __restrict__ x) {
  u32 lo[8];
  u64 carry = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const u64 t = (u64)x[j] + carry;
    lo[j] = (u32)t;
    carry = t >> 32;
  }
  // lo * 2^-256 (a Montgomery product with 1 is exact for any lo < 2^256), then * 2^512 through R^2;
  // the carry word (< 2^23) times 2^256 the same way
  const u32 one[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  const u32 hi[8] = {(u32)carry, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  u32 t[8], a[8], h[8];
  fr_mont_mul(t, lo, one);
  fr_mont_mul(a, t, kFrR2);
  fr_mont_mul(h, hi, kFrR2);
  fr_add(s, a, h);
}
// the sum over `width` adjacent lanes (a power of two <= 64), in every one of them; every lane takes part
DSV_DEV Ext lane_sum(Ext acc, int width) {
#pragma unroll 1
  for (int m = 1; m < width; m <<= 1) {
    const Niels mine = ext_to_niels(acc);
    Niels other;
#pragma unroll
    for (int i = 0; i < NL; i++) {
      other.vpu.l[i] = (u32)__shfl_xor((int)mine.vpu.l[i], m);
      other.vmu.l[i] = (u32)__shfl_xor((int)mine.vmu.l[i], m);
      other.z.l[i] = (u32)__shfl_xor((int)mine.z.l[i], m);
      other.t2d.l[i] = (u32)__shfl_xor((int)mine.t2d.l[i], m);
    }
    acc = ext_add_niels(acc, other);
  }
  return acc;
}
DSV_DEV bool ext_is_identity(const Ext& p) { return (bool)((int)fe_equal(p.u, fe_zero()) & (int)fe_equal(p.v, p.z)); }
// the workgroup's sum (four waves, every lane holding its wave's sum) -> out, by thread 0
DSV_DEV void workgroup_store_sum(Ext acc, u32* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) u32 sh[4 * kNielsWords];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) store_niels(sh + wave * kNielsWords, ext_to_niels(acc));
  __syncthreads();
  if (threadIdx.x == 0) {
    Ext tot = ext_from_niels(load_niels(sh));
#pragma unroll 1
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) tot = ext_add_niels(tot, load_niels(sh + w * kNielsWords));
    store_niels(out, ext_to_niels(tot));
  }
}
}  // namespace

template <int SCHEME>
__global__ void __launch_bounds__(256)
k_keyed_rlc_prep(RlcInputs in, const u32* __restrict__ key_idx, KeyedRlcKeys keys, ChaChaKey key, RlcPlan p,
                 RlcBuffers b, KeyedRlcBuffers kb, uint8_t* __restrict__ ok) {
  constexpr int NS = SCHEME == 0 ? 1 : 2;
  __shared__ unsigned long long lsum[kKeyedLdsKeys * NS * 8];
  __shared__ u32 ltouch[kKeyedLdsKeys];
  const bool lds = keys.k <= (size_t)kKeyedLdsKeys;  // (uniform)
  const SubView v = sub_view(p);
  if (lds) {
    for (u32 t = threadIdx.x; t < (u32)(kKeyedLdsKeys * NS * 8); t += 256) lsum[t] = 0;
    ltouch[threadIdx.x] = 0;
    __syncthreads();
  }
  const u32 il = blockIdx.x * 256 + threadIdx.x;
  if (il < v.n) {
    const u32 i = v.first + il;
    const size_t gi = (size_t)v.base + i;
    const PrepOut o{gi, i, il, v.total, p, b.pts + (size_t)v.g * b.pts_stride, b.digits + (size_t)v.g * b.digits_stride};
    u32* fsc = b.fsc + (size_t)v.g * b.fsc_stride;
    const u32 idx = key_idx[gi];
    const bool in_set = (size_t)idx < keys.k;
    bool good = (in.valid[gi] != 0) && in_set && keys.key_ok[in_set ? idx : 0u] != 0;  // (no read beyond the set)
    u32 us[8], cs[8];
    load_words8(us, in.u, gi);
    load_words8(cs, in.c, gi);
    good &= words_lt(us, kR32);
    // point slots: -R, then -R' (no long points: the keys are outside the buckets)
    bool curve = prep_point(o, in.r[0], 0, true, good);
    if (SCHEME == 1) curve &= prep_point(o, in.r[1], 1, true, good);
    if (good && !curve) atomicOr(&b.flags[4 + 4 * v.g], kRlcOffCurve);
    ok[gi] = good ? 1 : 0;
    u32 blk[16];
    chacha12_block(blk, key.w, (u64)gi);
    if (!good) {
      us[7] &= 0x0fffffffu;  // keep fr_mul's inputs in range; the products are 0 anyway
      cs[7] &= 0x0fffffffu;
    }
    u32 sc[NS][8];  // the item's per-key scalars: z c (z' c), or z c and z u (var-generator)
#pragma unroll
    for (int eq = 0; eq < (SCHEME == 1 ? 2 : 1); eq++) {
      u32 z[8], e[8];
      draw_z(z, blk + 8 * eq, p.wr * p.c, good);
      fr_mul(sc[eq], z, cs);
      fr_mul(e, z, us);
      if constexpr (SCHEME == 2) {
#pragma unroll
        for (int j = 0; j < 8; j++) sc[1][j] = e[j];
      } else {
        store_words8(reinterpret_cast<uint8_t*>(fsc), (size_t)eq * v.total + i, e);
      }
      emit_short(o, z, eq);
    }
    if (good) {
      if (lds) {
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
          for (int j = 0; j < 8; j++) atomicAdd(&lsum[(idx * NS + s) * 8 + j], (unsigned long long)sc[s][j]);
        ltouch[idx] = 1u;
      } else {
        unsigned long long* dst = kb.ksum + ((size_t)v.g * keys.k + idx) * NS * 8;
#pragma unroll
        for (int s = 0; s < NS; s++)
#pragma unroll
          for (int j = 0; j < 8; j++) atomicAdd(dst + s * 8 + j, (unsigned long long)sc[s][j]);
        kb.touched[(size_t)v.g * keys.k + idx] = 1u;
      }
    }
  }
  if (lds) {  // one flush per key this workgroup touched
    __syncthreads();
    unsigned long long* dst = kb.ksum + (size_t)v.g * keys.k * NS * 8;
    const u32 words = (u32)keys.k * NS * 8;
    for (u32 t = threadIdx.x; t < words; t += 256)
      if (ltouch[t / (NS * 8)]) atomicAdd(dst + t, lsum[t]);
    if (threadIdx.x < keys.k && ltouch[threadIdx.x]) kb.touched[(size_t)v.g * keys.k + threadIdx.x] = 1u;
  }
}

// kKeyParts lanes per (key, point): r * P from the point's table, for keys some sub-group references
__global__ void __launch_bounds__(256)
k_keyed_rlc_torsion(KeyedRlcKeys keys, KeyedRlcBuffers kb, int np, u32 groups) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int part = (int)(t % kKeyParts);
  const size_t kp = t / kKeyParts, key = kp / (size_t)np;
  const int pt = (int)(kp % (size_t)np);
  bool used = false;
  if (key < keys.k)
    for (u32 g = 0; g < groups; g++) used |= kb.touched[(size_t)g * keys.k + key] != 0u;
  Ext acc = ext_identity();
  if (used) {
    u32 r[8];
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = kR32[j];
    acc = key_accumulate_part(acc, r, keys.tables + (key * np + pt) * kKeyPointWords, part);
  }
  acc = lane_sum(acc, kKeyParts);
  if (used && part == 0 && !ext_is_identity(acc)) kb.bad[key] = 1u;
}

// kKeyParts lanes per (sub-group, key): the key's term s_k PK_k (+ s'_k PK'_k | + a_k Gen_k), the sum of the
// workgroup's terms into kb.partial; a referenced key that failed the subgroup test rejects the sub-group
template <int SCHEME>
__global__ void __launch_bounds__(kKeyedTermBlock)
k_keyed_rlc_terms(KeyedRlcKeys keys, KeyedRlcBuffers kb, u32* __restrict__ gflags) {
  constexpr int NP = SCHEME == 0 ? 1 : 2;
  const u32 g = blockIdx.y;
  const size_t t = (size_t)blockIdx.x * kKeyedTermBlock + threadIdx.x;
  const size_t key = t / kKeyParts;
  const int part = (int)(t % kKeyParts);
  Ext acc = ext_identity();
  if (key < keys.k && kb.touched[(size_t)g * keys.k + key]) {
    if (part == 0 && kb.bad[key]) atomicOr(&gflags[4 + 4 * g], kRlcTorsion);
    const unsigned long long* x = kb.ksum + ((size_t)g * keys.k + key) * NP * 8;
#pragma unroll 1
    for (int s = 0; s < NP; s++) {
      u32 sk[8];
      reduce_key_sum(sk, x + s * 8);
      acc = key_accumulate_part(acc, sk, keys.tables + (key * NP + s) * kKeyPointWords, part);
    }
  }
  acc = lane_sum(acc, 64);
  workgroup_store_sum(acc, kb.partial + ((size_t)g * gridDim.x + blockIdx.x) * kNielsWords);
}

__global__ void __launch_bounds__(256)
k_keyed_rlc_reduce(KeyedRlcBuffers kb, u32 blocks) {
  const u32 g = blockIdx.y;
  const u32* in = kb.partial + (size_t)g * blocks * kNielsWords;
  Ext acc = ext_identity();
#pragma unroll 1
  for (u32 j = threadIdx.x; j < blocks; j += 256) acc = ext_add_niels(acc, load_niels(in + (size_t)j * kNielsWords));
  acc = lane_sum(acc, 64);
  workgroup_store_sum(acc, kb.terms + (size_t)g * kNielsWords);
}

// the keyed per-signature kernel over sub-group blockIdx.y, returning at once where its aggregate accepted
template <int SCHEME>
__global__ void __launch_bounds__(kKeyedBlock)
k_keyed_fallback(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c, const uint8_t* __restrict__ valid,
                 const uint8_t* __restrict__ R_uv, const uint8_t* __restrict__ Rp_uv, const u32* __restrict__ key_idx,
                 KeyedRlcKeys keys, const u32* __restrict__ gtab0, const u32* __restrict__ gtab1,
                 uint8_t* __restrict__ ok, const u32* __restrict__ gflags, u32 sub, u32 items) {
  const u32 g = blockIdx.y;
  if (gate_says_done(gflags + 4 + 4 * g)) return;
  const size_t lo = (size_t)g * sub, hi = lo + sub < items ? lo + sub : items;
#pragma unroll 1
  for (size_t i = lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (size_t)gridDim.x * blockDim.x)
    ok[i] = keyed_item_ok<SCHEME>(u, c, valid, R_uv, Rp_uv, key_idx, i, keys.tables, keys.key_ok, keys.k, gtab0,
                                  gtab1) ? 1 : 0;
}

// ---- host side ----------------------------------------------------------------------------------------
hipError_t launch_keyed_rlc_prep(int scheme, const RlcPlan& p, const RlcBuffers& b, const KeyedRlcBuffers& kb,
                                 const RlcInputs& in, const uint32_t* key_idx, const KeyedRlcKeys& keys,
                                 ChaChaKey key, uint8_t* ok, hipStream_t s) {
  const unsigned G = p.groups;
  hipError_t err = hipMemsetAsync(b.counters, 0, (size_t)G * b.counters_stride * sizeof(uint32_t), s);
  if (err != hipSuccess) return err;
  // ksum, touched and bad are carved back to back (dsv_keyed_rlc.hip): one memset
  const size_t zero = (size_t)(reinterpret_cast<uint8_t*>(kb.bad + keys.k) - reinterpret_cast<uint8_t*>(kb.ksum));
  if (zero) err = hipMemsetAsync(kb.ksum, 0, zero, s);
  if (err != hipSuccess) return err;
  const dim3 grid(grid_for(p.n), G), block(256);
  if (scheme == 0) hipLaunchKernelGGL(k_keyed_rlc_prep<0>, grid, block, 0, s, in, key_idx, keys, key, p, b, kb, ok);
  else if (scheme == 1) hipLaunchKernelGGL(k_keyed_rlc_prep<1>, grid, block, 0, s, in, key_idx, keys, key, p, b, kb, ok);
  else hipLaunchKernelGGL(k_keyed_rlc_prep<2>, grid, block, 0, s, in, key_idx, keys, key, p, b, kb, ok);
  return hipGetLastError();
}

hipError_t launch_keyed_rlc_terms(int scheme, const RlcPlan& p, const RlcBuffers& b, const KeyedRlcBuffers& kb,
                                  const KeyedRlcKeys& keys, hipStream_t s) {
  const unsigned G = p.groups;
  const int np = keyset_points(scheme);
  if (keys.k)
    hipLaunchKernelGGL(k_keyed_rlc_torsion, dim3(grid_for(keys.k * (size_t)np * kKeyParts)), dim3(256), 0, s, keys, kb,
                       np, (u32)G);
  const unsigned tb = (unsigned)keyed_term_blocks(keys.k);
  const dim3 grid(tb, G), block(kKeyedTermBlock);
  if (scheme == 0) hipLaunchKernelGGL(k_keyed_rlc_terms<0>, grid, block, 0, s, keys, kb, b.flags);
  else if (scheme == 1) hipLaunchKernelGGL(k_keyed_rlc_terms<1>, grid, block, 0, s, keys, kb, b.flags);
  else hipLaunchKernelGGL(k_keyed_rlc_terms<2>, grid, block, 0, s, keys, kb, b.flags);
  hipLaunchKernelGGL(k_keyed_rlc_reduce, dim3(1, G), dim3(256), 0, s, kb, (u32)tb);
  return hipGetLastError();
}

void launch_keyed_fallback(int scheme, const RlcPlan& p, const uint8_t* u, const uint8_t* c, const uint8_t* valid,
                           const uint8_t* R_uv, const uint8_t* Rp_uv, const uint32_t* key_idx,
                           const KeyedRlcKeys& keys, const uint32_t* gtab0, const uint32_t* gtab1, uint8_t* ok,
                           const uint32_t* gflags, hipStream_t s) {
  if (p.items == 0) return;
  const unsigned G = p.groups;
  const unsigned per = kMaxKeyedGrid / G, want = grid_for(p.sub, kKeyedBlock);
  const dim3 grid(want < per ? want : per, G), block(kKeyedBlock);
  if (scheme == 0)
    hipLaunchKernelGGL(k_keyed_fallback<0>, grid, block, 0, s, u, c, valid, R_uv, Rp_uv, key_idx, keys, gtab0, gtab1, ok,
                       gflags, p.sub, p.items);
  else if (scheme == 1)
    hipLaunchKernelGGL(k_keyed_fallback<1>, grid, block, 0, s, u, c, valid, R_uv, Rp_uv, key_idx, keys, gtab0, gtab1, ok,
                       gflags, p.sub, p.items);
  else
    hipLaunchKernelGGL(k_keyed_fallback<2>, grid, block, 0, s, u, c, valid, R_uv, Rp_uv, key_idx, keys, gtab0, gtab1, ok,
                       gflags, p.sub, p.items);
}

}  // namespace dsv
