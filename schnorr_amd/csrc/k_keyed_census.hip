// k_keyed_census.hip — the census of a batch's keys against a registered key set (keyed_census.h, where the method
// and its invariants are described): the lookup's walk of keyed_lookup.h per item, a count per
// registered key, and the call's table of the distinct keys that missed.  Bytes in, counts out: no field
// arithmetic, no table of keyed.h is read.  k_keyed_lookup.hip is not touched: the walk, the hash and the key forms
// are the shared ones of keyed_lookup.h.
#define DSV_INDEX_KERNELS
#include "keyed_census.h"

namespace dsv {
namespace {

constexpr unsigned kCensusFlushShare = 16;  // LDS path: a workgroup sees at least 16 items per bin it flushes ...
constexpr unsigned kCensusMinGrid = 512;    // ... as long as that leaves two waves per SIMD of the device

// lane `src`'s copy of a row word (src wave-uniform)
__device__ __forceinline__ uint32_t lane_word(uint32_t v, int src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, src);
}
template <int W>
__device__ __forceinline__ bool same_as_lane(const Words<W>& w, int src) {
  bool eq = true;
#pragma unroll
  for (int j = 0; j < W; j++) {
    eq &= w.q[j].x == lane_word(w.q[j].x, src);
    eq &= w.q[j].y == lane_word(w.q[j].y, src);
    eq &= w.q[j].z == lane_word(w.q[j].z, src);
    eq &= w.q[j].w == lane_word(w.q[j].w, src);
  }
  return eq;
}

// ------------------------------------------------------------------------------------------
// `c` items under the key w (hash h), the lowest of them item i, into the call's miss table: the walk of
// k_index_append with item indices for key indices.  An occupant's key is read from the call's input columns at the
// occupant's row.  Never waits: every step is one atomic and a comparison.
// ------------------------------------------------------------------------------------------
template <class Form>
__device__ __forceinline__ void table_insert(const Words<Form::W>& w, uint32_t h, uint32_t i, uint32_t c,
                                             const uint8_t* __restrict__ key_a, const uint8_t* __restrict__ key_b,
                                             size_t n, uint32_t* tslots, uint32_t* tcounts, size_t tmask) {
  constexpr int W = Form::W;
  size_t slot = h & tmask;
#pragma unroll 1
  for (size_t probe = 0;; probe++) {
    const uint32_t old = atomicCAS(&tslots[slot], kSlotEmpty, i);
    if (old == kSlotEmpty) {
      atomicAdd(&tcounts[slot], c);
      return;
    }
    // (no slot holds an index >= n; were there one, the lane reads its own row instead, in bounds, and goes on)
    const bool known = old < n;
    const Words<W> occ = Form::item(key_a, key_b, known ? old : i);
    if (known && same_words<W>(w, occ)) {
      atomicMin(&tslots[slot], i);
      atomicAdd(&tcounts[slot], c);
      return;
    }
    if (probe == tmask) return;  // unreachable: at most n distinct keys in >= 2n slots, an empty slot comes first
    slot = (slot + 1) & tmask;
  }
}

}  // namespace

// slots to kSlotEmpty, counts to 0: one lane per 16 bytes of each, grid-stride (quads: cap / 4, cap >= 64)
__global__ void __launch_bounds__(kLookupBlock)
k_census_clear(uint4* __restrict__ tslots, uint4* __restrict__ tcounts, size_t quads) {
  const uint4 empty = make_uint4(kSlotEmpty, kSlotEmpty, kSlotEmpty, kSlotEmpty), zero = make_uint4(0, 0, 0, 0);
#pragma unroll 1
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t)gridDim.x * blockDim.x) {
    tslots[q] = empty;
    tcounts[q] = zero;
  }
}

// ------------------------------------------------------------------------------------------
// One lane per item, grid-stride in whole waves (every lane of a wave makes the same number of trips, so the
// ballots see all 64).  lds_k: k when the workgroup counts its hits in the LDS histogram `hist` (k words of dynamic
// LDS), 0 when the waves combine them.  totals[1] += items that got kSlotEmpty, totals[2] += unusable items; one
// atomic each per workgroup that has any.
// ------------------------------------------------------------------------------------------
template <class Form>
__global__ void __launch_bounds__(kLookupBlock)
k_census(const uint8_t* __restrict__ key_a, const uint8_t* __restrict__ key_b, const uint8_t* __restrict__ usable,
         size_t n, const uint8_t* __restrict__ rows, const uint32_t* __restrict__ slots, size_t mask, size_t k,
         uint32_t lds_k, uint32_t* __restrict__ key_idx, uint32_t* __restrict__ hits, uint32_t* tslots,
         uint32_t* tcounts, size_t tmask, uint32_t* __restrict__ totals) {
  constexpr int W = Form::W;
  extern __shared__ uint32_t hist[];
  __shared__ uint32_t block_missed, block_unusable;
  if (threadIdx.x == 0) block_missed = block_unusable = 0;
  for (uint32_t b = threadIdx.x; b < lds_k; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  const int lane = (int)(threadIdx.x & (uint32_t)(warpSize - 1));
  uint32_t missed = 0, unusable = 0;
#pragma unroll 1
  for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x - (uint32_t)lane); base < n;
       base += (size_t)gridDim.x * blockDim.x) {
    const size_t i = base + (size_t)lane;
    const bool active = i < n;
    const size_t row = active ? i : n - 1;  // (a lane past the end reads the last row and takes no part)
    const Words<W> w = Form::item(key_a, key_b, row);
    const bool has_key = active && (usable == nullptr || usable[row] != 0);
    uint32_t found = kSlotEmpty;
    if (has_key) found = find_key<W>(w, rows, slots, mask, k);  // (keyed_lookup.h's walk; k = 0: nothing is read)
    if (active && key_idx) key_idx[i] = found;
    const bool hit = found != kSlotEmpty;
    const bool miss = has_key && !hit;
    missed += (active && !hit) ? 1u : 0u;
    unusable += (active && !has_key) ? 1u : 0u;

    // ---- hits ----
    if (hits) {  // (uniform)
      if (lds_k) {
        if (hit) atomicAdd(&hist[found], 1u);
      } else {
        // the wave's lanes with one index: the lowest of them adds their number
        unsigned long long pend = __ballot(hit);
        while (pend) {
          const int leader = __builtin_ctzll(pend);
          const uint32_t f = lane_word(found, leader);
          const unsigned long long group = __ballot(hit && found == f);
          if (lane == leader) atomicAdd(&hits[f], (uint32_t)__popcll(group));
          pend &= ~group;
        }
      }
    }

    // ---- misses: the wave's lanes with one key, then one walk per distinct key ----
    unsigned long long pend = __ballot(miss);
    if (pend == 0) continue;
    const uint32_t h = home_hash<W>(w);
    bool pending = miss, walker = false;
    uint32_t group_items = 0;
    while (pend) {
      const int leader = __builtin_ctzll(pend);
      bool same = pending && h == lane_word(h, leader);
      // another lane has the leader's hash: equal only if every word of the key is
      if (__ballot(same) != (1ull << leader)) same = same && same_as_lane<W>(w, leader);
      const unsigned long long group = __ballot(same);
      if (lane == leader) {
        walker = true;
        group_items = (uint32_t)__popcll(group);
      }
      pending = pending && !same;
      pend &= ~group;
    }
    // (the leader is its group's lowest lane: i is the group's lowest item index)
    if (walker) table_insert<Form>(w, h, (uint32_t)i, group_items, key_a, key_b, n, tslots, tcounts, tmask);
  }

  if (lds_k) {
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < lds_k; b += blockDim.x) {
      const uint32_t c = hist[b];
      if (c) atomicAdd(&hits[b], c);
    }
  }
#pragma unroll
  for (int off = warpSize / 2; off > 0; off >>= 1) {
    missed += __shfl_down(missed, off);
    unusable += __shfl_down(unusable, off);
  }
  if (lane == 0 && missed) atomicAdd(&block_missed, missed);
  if (lane == 0 && unusable) atomicAdd(&block_unusable, unusable);
  __syncthreads();
  if (threadIdx.x == 0 && block_missed) atomicAdd(&totals[1], block_missed);
  if (threadIdx.x == 0 && block_unusable) atomicAdd(&totals[2], block_unusable);
}

// ------------------------------------------------------------------------------------------
// One lane per slot of the miss table, grid-stride in whole waves: a wave that holds occupied slots reserves their
// places in the report with ONE atomic on totals[0] (k_miss_list's scheme), a lane's place is the reserved base plus
// the number of occupied slots in the lanes below it.  At most n places are ever reserved (one per distinct key).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLookupBlock)
k_census_report(const uint32_t* __restrict__ tslots, const uint32_t* __restrict__ tcounts, size_t cap,
                uint32_t* __restrict__ miss_rep, uint32_t* __restrict__ miss_count, uint32_t* __restrict__ totals) {
  const uint32_t lane = threadIdx.x & (uint32_t)(warpSize - 1);
#pragma unroll 1
  for (size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < cap;
       base += (size_t)gridDim.x * blockDim.x) {
    const size_t slot = base + lane;  // (cap is a multiple of 64: always below cap)
    const uint32_t rep = tslots[slot];
    const bool occupied = rep != kSlotEmpty;
    const unsigned long long wave = __ballot(occupied);
    if (wave == 0) continue;
    uint32_t first = 0;
    if (lane == (uint32_t)__builtin_ctzll(wave)) first = atomicAdd(&totals[0], (uint32_t)__popcll(wave));
    first = __shfl(first, __builtin_ctzll(wave));
    if (occupied) {
      const uint32_t place = first + (uint32_t)__popcll(wave & ((1ull << lane) - 1ull));
      miss_rep[place] = rep;
      miss_count[place] = tcounts[slot];
    }
  }
}

void launch_census(KeyForm form, const uint8_t* key_a, const uint8_t* key_b, const uint8_t* usable, int npoints,
                   size_t n, const uint8_t* rows, const uint32_t* slots, size_t mask, size_t k, int lds_keys,
                   uint32_t* key_idx, uint32_t* hits, uint32_t* miss_rep, uint32_t* miss_count, uint32_t* totals,
                   void* table, hipStream_t s) {
  const size_t cap = keyset_index_cap(n);
  uint32_t* tslots = static_cast<uint32_t*>(table);
  uint32_t* tcounts = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(table) + lookup_round256(4 * cap));
  for (int t = 0; t < 4; t++) launch_store_word(totals + t, 0, s);
  const unsigned gc = grid_for(cap / 4, kLookupBlock);
  hipLaunchKernelGGL(k_census_clear, dim3(gc < kMaxLookupGrid ? gc : kMaxLookupGrid), dim3(kLookupBlock), 0, s,
                     reinterpret_cast<uint4*>(tslots), reinterpret_cast<uint4*>(tcounts), cap / 4);
  // the LDS histogram: for a set that has keys and fits; then fewer, longer workgroups, so that the flushes (one
  // global atomic per non-zero bin and workgroup) stay small against the item loop
  if (lds_keys > kCensusLdsKeysMax) lds_keys = kCensusLdsKeysMax;
  const uint32_t lds_k = hits && k != 0 && k <= (size_t)(lds_keys > 0 ? lds_keys : 0) ? (uint32_t)k : 0u;
  unsigned g = grid_for(n, kLookupBlock);
  if (g > kMaxLookupGrid) g = kMaxLookupGrid;
  if (lds_k) {
    const size_t share = n / ((size_t)kCensusFlushShare * lds_k);
    const unsigned want = share > kCensusMinGrid ? (unsigned)(share < kMaxLookupGrid ? share : kMaxLookupGrid)
                                                 : kCensusMinGrid;
    if (g > want) g = want;
  }
  const dim3 grid(g), block(kLookupBlock);
  const size_t lds_bytes = 4 * (size_t)lds_k;
  auto go = [&](auto f) {
    hipLaunchKernelGGL(k_census<decltype(f)>, grid, block, lds_bytes, s, key_a, key_b, usable, n, rows, slots, mask, k,
                       lds_k, key_idx, hits, tslots, tcounts, cap - 1, totals);
  };
  if (form == kKeyAffine) {
    if (npoints == 1) go(AffineKey<1>{}); else go(AffineKey<2>{});
  } else {
    if (npoints == 1) go(RecordKey<1>{}); else go(RecordKey<2>{});
  }
  const unsigned gr = grid_for(cap, kLookupBlock);
  hipLaunchKernelGGL(k_census_report, dim3(gr < kMaxLookupGrid ? gr : kMaxLookupGrid), dim3(kLookupBlock), 0, s,
                     (const uint32_t*)tslots, (const uint32_t*)tcounts, cap, miss_rep, miss_count, totals);
}

}  // namespace dsv
