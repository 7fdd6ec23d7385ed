// k_keyed_lookup.hip — the indices of a registered key set over its own keys (keyed_lookup.h): the insertion of
// keys into an index, fresh or live (every constructor and dsv_keyset_append), one lane per key behind the table
// build, and the lookup that turns a batch's keys into the key_idx column of the keyed kernels, one lane per
// item.  Both are one kernel each over a key form — the affine bytes or the compressed records of the same keys.
// Bytes in, indices out: no field arithmetic, no table of keyed.h is read, a hit costs no square root.
#define DSV_INDEX_KERNELS
#include "keyed_lookup.h"

namespace dsv {
namespace {

// the lookup's tail, per block: the waves' sums meet in LDS, one atomic per block that missed at all
__device__ __forceinline__ void add_block_misses(uint32_t missed, uint32_t& block_misses,
                                                 uint32_t* __restrict__ misses) {
#pragma unroll
  for (int off = warpSize / 2; off > 0; off >>= 1) missed += __shfl_down(missed, off);
  if ((threadIdx.x & (warpSize - 1)) == 0 && missed) atomicAdd(&block_misses, missed);
  __syncthreads();
  if (threadIdx.x == 0 && block_misses) atomicAdd(misses, block_misses);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// m keys, indices first .. first + m - 1, into an index that already holds the keys below `first` (a fresh set:
// first = 0) and that lookups enqueued earlier may be walking.  One lane per new key (P0 / P1, key_ok: the m new
// keys' source points and verdicts; rows / slots: the whole index): its row goes into the index's own copy at
// first + j, fenced; a valid key then claims the first empty slot from its home slot on.  An occupied slot holds a
// key that differs (go on) or an equal one registered twice: the slot then keeps the lower index (atomicMin), so a
// key appended twice, or one already registered, keeps its first index.  An occupant below `first` was registered
// by an earlier call: it is compared by the index's own copy, which no lane of this launch writes (rows < first);
// an occupant from `first` on is a lane of this launch and is compared by the source points, which nobody writes
// (Form::occupant).  Why the walk is right:
//   - a slot never returns to empty, and its occupant only ever changes to an equal key with a lower index, so
//     every lane of equal keys walks the same slots and stops at the same one;
//   - the table is at most half full (cap >= 2 * capacity), so the walk ends at an empty slot;
//   - a lookup that runs beside this launch carries the k of its own call (< first + 1) and reads every occupant
//     >= k as an empty slot: it never follows an index into a row this launch is still writing.
// Two valid keys have equal records iff they have equal affine bytes, so both forms' indices
// hold the same keys at the same lowest indices.
// ------------------------------------------------------------------------------------------
template <class Form>
__global__ void __launch_bounds__(kLookupBlock)
k_index_append(const uint8_t* __restrict__ P0, const uint8_t* __restrict__ P1, const uint8_t* __restrict__ key_ok,
               size_t first, size_t m, uint8_t* rows, uint32_t* __restrict__ slots, size_t mask) {
  constexpr int W = Form::W;
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const Words<W> w = Form::source(P0, P1, j);
  uint4* own = reinterpret_cast<uint4*>(rows + (first + j) * (size_t)(16 * W));
#pragma unroll
  for (int q = 0; q < W; q++) own[q] = w.q[q];
  __threadfence();
  if (key_ok[j] == 0) return;
  const uint32_t me = (uint32_t)(first + j);
  size_t slot = home_hash<W>(w) & mask;
#pragma unroll 1
  for (size_t probe = 0;; probe++) {
    const uint32_t old = atomicCAS(&slots[slot], kSlotEmpty, me);
    if (old == kSlotEmpty) return;
    // (no slot holds an index >= first + m; were there one, the lane reads its own row instead, in bounds, and
    // goes on — the load stands in front of the test: behind it, AffineKey<2> takes 72 VGPRs instead of 66)
    const bool known = old < first + m;
    const Words<W> occ = Form::occupant(P0, P1, rows, known ? old : me, first);
    if (known && same_words<W>(w, occ)) {
      atomicMin(&slots[slot], me);
      return;
    }
    if (probe == mask) return;  // unreachable: the table is at most half full, so an empty slot comes first
    slot = (slot + 1) & mask;
  }
}

// ------------------------------------------------------------------------------------------
// One lane per item, grid-stride: the item's row in registers and walk_index (keyed_lookup.h) from its home slot.
// k: the set's key count when the call was enqueued.
// ------------------------------------------------------------------------------------------
template <class Form>
__global__ void __launch_bounds__(kLookupBlock)
k_index_lookup(const uint8_t* __restrict__ key_a, const uint8_t* __restrict__ key_b, size_t n,
               const uint8_t* __restrict__ rows, const uint32_t* __restrict__ slots, size_t mask, size_t k,
               uint32_t* __restrict__ key_idx, uint32_t* __restrict__ misses) {
  constexpr int W = Form::W;
  __shared__ uint32_t block_misses;
  if (threadIdx.x == 0) block_misses = 0;
  __syncthreads();
  uint32_t missed = 0;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const Words<W> w = Form::item(key_a, key_b, i);
    const uint32_t found = walk_index<W>(w, rows, slots, mask, k);
    key_idx[i] = found;
    missed += found == kSlotEmpty ? 1u : 0u;
  }
  if (!misses) return;  // (uniform: every lane of the grid takes the same side)
  add_block_misses(missed, block_misses, misses);
}

namespace {
// go(Form{}) for the form of `npoints`-point keys
template <class Go>
void with_key_form(KeyForm form, int npoints, Go go) {
  if (form == kKeyAffine) {
    if (npoints == 1) go(AffineKey<1>{}); else go(AffineKey<2>{});
  } else {
    if (npoints == 1) go(RecordKey<1>{}); else go(RecordKey<2>{});
  }
}
}  // namespace

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

void launch_index_append(KeyForm form, const uint8_t* P0, const uint8_t* P1, const uint8_t* key_ok, int npoints,
                         size_t first, size_t m, uint8_t* rows, uint32_t* slots, size_t mask, hipStream_t s) {
  if (m == 0) return;
  const dim3 grid(grid_for(m, kLookupBlock)), block(kLookupBlock);
  with_key_form(form, npoints, [&](auto f) {
    hipLaunchKernelGGL(k_index_append<decltype(f)>, grid, block, 0, s, P0, P1, key_ok, first, m, rows, slots, mask);
  });
}

hipError_t launch_index_lookup(KeyForm form, const uint8_t* key_a, const uint8_t* key_b, int npoints, size_t n,
                               const uint8_t* rows, const uint32_t* slots, size_t mask, size_t k, uint32_t* key_idx,
                               uint32_t* misses, hipStream_t s) {
  if (misses) launch_store_word(misses, 0, s);
  if (n == 0) return hipSuccess;
  const unsigned g = grid_for(n, kLookupBlock);
  const dim3 grid(g < kMaxLookupGrid ? g : kMaxLookupGrid), block(kLookupBlock);
  with_key_form(form, npoints, [&](auto f) {
    hipLaunchKernelGGL(k_index_lookup<decltype(f)>, grid, block, 0, s, key_a, key_b, n, rows, slots, mask, k, key_idx,
                       misses);
  });
  return hipSuccess;
}

}  // namespace dsv
