// k_keyed_lookup.hip — the index of a registered key set over its own keys (keyed_lookup.h): its build, one
// lane per key behind the table build, the insertion of further keys into a live index (dsv_keyset_append),
// and the lookup that turns a batch's key columns into the key_idx column of the keyed kernels, one lane per
// item.  Bytes in, indices out: no field arithmetic, no table of keyed.h is read.
#include "keyed_lookup.h"

namespace dsv {
namespace {

// a key's bytes in registers: 4 x 16 B per point
template <int NP>
struct KeyWords {
  uint4 q[4 * NP];
};
template <int NP>
__device__ __forceinline__ KeyWords<NP> load_key(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                  size_t i) {
  KeyWords<NP> w;
  const uint4* pa = reinterpret_cast<const uint4*>(a + i * 64);
#pragma unroll
  for (int j = 0; j < 4; j++) w.q[j] = pa[j];
  if (NP == 2) {
    const uint4* pb = reinterpret_cast<const uint4*>(b + i * 64);
#pragma unroll
    for (int j = 0; j < 4; j++) w.q[4 * (NP - 1) + j] = pb[j];
  }
  return w;
}
__device__ __forceinline__ bool same16(const uint4& x, const uint4& y) {
  return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) == 0u;
}
// w against 4 * NP consecutive 16-byte words at p
template <int NP>
__device__ __forceinline__ bool same_key(const KeyWords<NP>& w, const uint4* __restrict__ p) {
  bool eq = true;
#pragma unroll
  for (int j = 0; j < 4 * NP; j++) eq &= same16(w.q[j], p[j]);
  return eq;
}
template <int NP>
__device__ __forceinline__ bool same_words(const KeyWords<NP>& a, const KeyWords<NP>& b) {
  bool eq = true;
#pragma unroll
  for (int j = 0; j < 4 * NP; j++) eq &= same16(a.q[j], b.q[j]);
  return eq;
}
template <int NP>
__device__ __forceinline__ uint32_t home_hash(const KeyWords<NP>& w) {
  KeyHash h;
#pragma unroll
  for (int j = 0; j < 4 * NP; j++) {
    h.word(w.q[j].x);
    h.word(w.q[j].y);
    h.word(w.q[j].z);
    h.word(w.q[j].w);
  }
  return h.finish();
}

}  // namespace

// ------------------------------------------------------------------------------------------
// One lane per key: its bytes go into the index's own copy; a valid key then claims the first empty slot from
// its home slot on.  An occupied slot holds a key that differs (go on) or an equal one registered twice: the
// slot then keeps the lower index.  A slot never returns to empty and its occupant only ever changes to an
// equal key, so every lane of equal keys walks the same slots and stops at the same one.  Occupants are
// compared by the source points, which no lane writes.  The table is at most half full: the walk ends.
// ------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(kLookupBlock)
k_build_key_index(const uint8_t* __restrict__ P0, const uint8_t* __restrict__ P1,
                  const uint8_t* __restrict__ key_ok, size_t k, uint8_t* __restrict__ keys,
                  uint32_t* __restrict__ slots, size_t mask) {
  const size_t key = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= k) return;
  const KeyWords<NP> w = load_key<NP>(P0, P1, key);
  uint4* own = reinterpret_cast<uint4*>(keys + key * (size_t)(64 * NP));
#pragma unroll
  for (int j = 0; j < 4 * NP; j++) own[j] = w.q[j];
  if (key_ok[key] == 0) return;
  const uint32_t me = (uint32_t)key;
  size_t slot = home_hash<NP>(w) & mask;
#pragma unroll 1
  for (size_t probe = 0;; probe++) {
    const uint32_t old = atomicCAS(&slots[slot], kSlotEmpty, me);
    if (old == kSlotEmpty) return;
    if (old < k && same_words<NP>(w, load_key<NP>(P0, P1, old))) {
      atomicMin(&slots[slot], me);
      return;
    }
    if (probe == mask) return;  // unreachable: the table is at most half full, so an empty slot comes first
    slot = (slot + 1) & mask;
  }
}

// ------------------------------------------------------------------------------------------
// dsv_keyset_append: m further keys, indices first .. first + m - 1, into an index that already holds the keys
// below `first` and that lookups enqueued earlier may be walking.  One lane per new key (P0 / P1, key_ok: the m
// new keys' rows; keys / slots: the whole index): its bytes go into the index's own copy at row first + j,
// fenced; a valid key then claims the first empty slot from its home slot on, exactly as in the build.  An
// occupant below `first` was registered by an earlier call: it is compared by the index's own copy, which no
// lane of this launch writes (rows < first); an occupant from `first` on is a lane of this launch and is
// compared by the source points, which nobody writes.  An equal occupant keeps the lower index (atomicMin), so
// a key appended twice, or one already registered, keeps its first index.  As in the build:
// a slot never returns to empty, an occupant only ever changes to an equal key with a lower index, and the
// table is at most half full (cap >= 2 * capacity), so the walk ends.  A lookup that runs beside this launch
// carries the k of its own call (< first + 1) and reads every occupant >= k as an empty slot: it never follows
// an index into a row this launch is still writing.
// ------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(kLookupBlock)
k_append_key_index(const uint8_t* __restrict__ P0, const uint8_t* __restrict__ P1,
                   const uint8_t* __restrict__ key_ok, size_t first, size_t m, uint8_t* keys,
                   uint32_t* __restrict__ slots, size_t mask) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const KeyWords<NP> w = load_key<NP>(P0, P1, j);
  uint4* own = reinterpret_cast<uint4*>(keys + (first + j) * (size_t)(64 * NP));
#pragma unroll
  for (int q = 0; q < 4 * NP; q++) own[q] = w.q[q];
  __threadfence();
  if (key_ok[j] == 0) return;
  const uint32_t me = (uint32_t)(first + j);
  size_t slot = home_hash<NP>(w) & mask;
#pragma unroll 1
  for (size_t probe = 0;; probe++) {
    const uint32_t old = atomicCAS(&slots[slot], kSlotEmpty, me);
    if (old == kSlotEmpty) return;
    // the occupant's bytes: an earlier call's key from the index's copy, a lane of this launch from the source
    const bool older = old < first;
    const uint8_t* pa = older ? keys + (size_t)old * (size_t)(64 * NP) : P0 + (size_t)(old - first) * 64;
    const uint8_t* pb = older ? pa + 64 : P1 + (size_t)(old - first) * 64;
    const bool equal = old < first + m && same_words<NP>(w, load_key<NP>(pa, pb, 0));
    if (equal) {
      atomicMin(&slots[slot], me);
      return;
    }
    if (probe == mask) return;  // unreachable: the table is at most half full, so an empty slot comes first
    slot = (slot + 1) & mask;
  }
}

// ------------------------------------------------------------------------------------------
// One lane per item, grid-stride: the item's key bytes in registers, a walk from the home slot that compares
// against the index's copy of each occupant's bytes and ends at the first empty slot.  k: the set's key count
// when the call was enqueued.  An occupant >= k was appended since: it is read as an empty slot and ends the
// walk.  That is exact: every key below k whose walk passes this slot was placed while the slot was still
// empty, so it sits in front of it.
// ------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(kLookupBlock)
k_key_lookup(const uint8_t* __restrict__ key_a, const uint8_t* __restrict__ key_b, size_t n,
             const uint8_t* __restrict__ keys, const uint32_t* __restrict__ slots, size_t mask, size_t k,
             uint32_t* __restrict__ key_idx, uint32_t* __restrict__ misses) {
  __shared__ uint32_t block_misses;
  if (threadIdx.x == 0) block_misses = 0;
  __syncthreads();
  uint32_t missed = 0;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const KeyWords<NP> w = load_key<NP>(key_a, key_b, i);
    size_t slot = home_hash<NP>(w) & mask;
    uint32_t found = kSlotEmpty;
#pragma unroll 1
    for (size_t probe = 0;; probe++) {
      const uint32_t occ = slots[slot];
      if (occ >= k) break;  // empty (kSlotEmpty >= k), or a key newer than this call
      if (same_key<NP>(w, reinterpret_cast<const uint4*>(keys + (size_t)occ * (size_t)(64 * NP)))) {
        found = occ;
        break;
      }
      if (probe == mask) break;  // unreachable for the same reason: an empty slot ends the walk first
      slot = (slot + 1) & mask;
    }
    key_idx[i] = found;
    missed += found == kSlotEmpty ? 1u : 0u;
  }
  if (!misses) return;  // (uniform: every lane of the grid takes the same side)
  // per block: the waves' sums meet in LDS, one atomic per block that missed at all
#pragma unroll
  for (int off = warpSize / 2; off > 0; off >>= 1) missed += __shfl_down(missed, off);
  if ((threadIdx.x & (warpSize - 1)) == 0 && missed) atomicAdd(&block_misses, missed);
  __syncthreads();
  if (threadIdx.x == 0 && block_misses) atomicAdd(misses, block_misses);
}

// one word, written by a kernel of its own (launch_store_word)
__global__ void k_store_word(uint32_t* __restrict__ p, uint32_t v) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *p = v;
}
void launch_store_word(uint32_t* p, uint32_t v, hipStream_t s) {
  hipLaunchKernelGGL(k_store_word, dim3(1), dim3(64), 0, s, p, v);
}

hipError_t launch_clear_key_index(uint32_t* slots, size_t mask, hipStream_t s) {
  return hipMemsetAsync(slots, 0xff, (mask + 1) * 4, s);
}

void launch_append_key_index(const uint8_t* P0, const uint8_t* P1, const uint8_t* key_ok, int npoints, size_t first,
                             size_t m, uint8_t* keys, uint32_t* slots, size_t mask, hipStream_t s) {
  if (m == 0) return;
  const dim3 grid(grid_for(m, kLookupBlock)), block(kLookupBlock);
  if (first == 0) {  // nothing registered yet: the build, which compares by the source points alone
    if (npoints == 1)
      hipLaunchKernelGGL(k_build_key_index<1>, grid, block, 0, s, P0, P1, key_ok, m, keys, slots, mask);
    else
      hipLaunchKernelGGL(k_build_key_index<2>, grid, block, 0, s, P0, P1, key_ok, m, keys, slots, mask);
  } else if (npoints == 1) {
    hipLaunchKernelGGL(k_append_key_index<1>, grid, block, 0, s, P0, P1, key_ok, first, m, keys, slots, mask);
  } else {
    hipLaunchKernelGGL(k_append_key_index<2>, grid, block, 0, s, P0, P1, key_ok, first, m, keys, slots, mask);
  }
}

hipError_t launch_key_lookup(const uint8_t* key_a, const uint8_t* key_b, int npoints, size_t n,
                             const uint8_t* keys, const uint32_t* slots, size_t mask, size_t k,
                             uint32_t* key_idx, uint32_t* misses, hipStream_t s) {
  if (misses) launch_store_word(misses, 0, s);
  if (n == 0) return hipSuccess;
  const unsigned g = grid_for(n, kLookupBlock);
  const dim3 grid(g < kMaxLookupGrid ? g : kMaxLookupGrid), block(kLookupBlock);
  if (npoints == 1)
    hipLaunchKernelGGL(k_key_lookup<1>, grid, block, 0, s, key_a, key_b, n, keys, slots, mask, k, key_idx,
                       misses);
  else
    hipLaunchKernelGGL(k_key_lookup<2>, grid, block, 0, s, key_a, key_b, n, keys, slots, mask, k, key_idx,
                       misses);
  return hipSuccess;
}

}  // namespace dsv
