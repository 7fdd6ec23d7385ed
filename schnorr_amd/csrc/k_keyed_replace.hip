// k_keyed_replace.hip — keys of a registered set replaced in place (dsv_keyset_replace*, keyed_lookup.h; DESIGN.md
// §10.8): the commit that scatters the new keys' tables and rows from the call's scratch into the set, and the
// rebuild of an index from the set's own rows in the canonical layout.  Both run inside the replace's exclusive
// section, on a quiet device: nothing reads the set beside them.  Bytes in, bytes out: no field arithmetic.
#define DSV_INDEX_KERNELS
#include "keyed_lookup.h"

namespace dsv {
namespace {
constexpr int kReplaceBlock = 256;
constexpr unsigned kMaxReplaceGrid = 2048;  // 8 blocks per CU; the rest is grid-stride
constexpr int kCommitUnroll = 4;            // 16-byte loads in flight per lane

template <int W>
__device__ __forceinline__ void store_row(uint8_t* rows, size_t i, const Words<W>& w) {
  uint4* p = reinterpret_cast<uint4*>(rows + i * (size_t)(16 * W));
#pragma unroll
  for (int j = 0; j < W; j++) p[j] = w.q[j];
}
}  // namespace

// ------------------------------------------------------------------------------------------
// The tables of the m new keys, contiguous in the scratch (key j at j * T 16-byte words, T = NP tables), go to
// key indices[j] of the set: a grid-stride copy over all m * T words, kCommitUnroll loads in flight per lane.  The
// first m lanes of the grid then write the small rows of key j — its key_ok byte, its affine index row (the staged
// point bytes as they are) and its record index row (formed from them: RecordKey::source) — to indices[j] as well.
// indices are pairwise distinct and below the set's k (checked by the host), so no two lanes write one byte.
// ------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(kReplaceBlock)
k_replace_commit(const uint32_t* __restrict__ indices, size_t m, const uint4* __restrict__ src_tables,
                 const uint8_t* __restrict__ src_key_ok, const uint8_t* __restrict__ P0,
                 const uint8_t* __restrict__ P1, uint4* __restrict__ tables, uint8_t* __restrict__ key_ok,
                 uint8_t* __restrict__ affine_rows, uint8_t* __restrict__ record_rows) {
  constexpr size_t T = (size_t)NP * (kKeyPointBytes / 16);
  static_assert(kKeyPointBytes % 16 == 0, "a table is a whole number of 16-byte words");
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = (size_t)gridDim.x * blockDim.x;
  const size_t total = m * T;
#pragma unroll 1
  for (size_t base = lane; base < total; base += kCommitUnroll * lanes) {
    uint4 v[kCommitUnroll];
#pragma unroll
    for (int q = 0; q < kCommitUnroll; q++) {
      const size_t i = base + q * lanes;
      if (i < total) v[q] = src_tables[i];
    }
#pragma unroll
    for (int q = 0; q < kCommitUnroll; q++) {
      const size_t i = base + q * lanes;
      if (i < total) {
        const size_t j = i / T;
        tables[(size_t)indices[j] * T + (i - j * T)] = v[q];
      }
    }
  }
#pragma unroll 1
  for (size_t j = lane; j < m; j += lanes) {
    const size_t dst = indices[j];
    key_ok[dst] = src_key_ok[j];
    store_row<AffineKey<NP>::W>(affine_rows, dst, AffineKey<NP>::source(P0, P1, j));
    store_row<RecordKey<NP>::W>(record_rows, dst, RecordKey<NP>::source(P0, P1, j));
  }
}

// the affine index rows (key-major: PK | PK') as planar columns, one lane per 16 bytes
template <int NP>
__global__ void __launch_bounds__(kReplaceBlock)
k_rows_to_planar(const uint4* __restrict__ affine_rows, size_t k, uint4* __restrict__ P0, uint4* __restrict__ P1) {
  const size_t total = k * (size_t)(4 * NP);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t key = i / (4 * NP), part = i % (4 * NP);
    (part < 4 ? P0 : P1)[key * 4 + (part & 3)] = affine_rows[i];
  }
}

// ------------------------------------------------------------------------------------------
// Ordered insertion into a cleared slot array.  One lane per slot of `reps`; a lane whose slot holds a key index
// carries it from the key's home slot on: old = atomicMin(slot, carried).  An empty slot (kSlotEmpty is the
// largest value) takes the carried index and the lane is done; a slot that held a higher index takes it too and the
// lane carries the displaced index on; a slot that holds a lower index is passed.  The carried keys are pairwise
// different (reps holds one index per distinct valid key), so no row is compared: a row is read once, for its home.
// Why the result is the canonical layout whatever the order of the lanes:
//   - a slot's value only ever falls, and a lane puts index x into slot p only after every slot from x's home up to
//     p answered with a lower index (its own walk), or after x was displaced from a slot that now holds a lower
//     one; so at every moment each placed x has only lower indices between its home and its place;
//   - at the end every index is placed, and only one layout has that property: by induction over the indices, x
//     sits in the first slot from its home on that holds no lower index — where inserting 0, 1, 2, ... one after
//     the other puts it.
// At most (mask + 1) / 2 slots are ever filled, so a walk meets an empty slot within that many steps.
// ------------------------------------------------------------------------------------------
template <template <int> class Form, int NP>
__global__ void __launch_bounds__(kReplaceBlock)
k_index_reinsert(const uint8_t* __restrict__ affine_rows, const uint32_t* __restrict__ reps, uint32_t* slots,
                 size_t mask) {
  constexpr int W = Form<NP>::W;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t > mask) return;
  uint32_t carried = reps[t];
  if (carried == kSlotEmpty) return;
  const uint8_t* key = affine_rows + (size_t)carried * (size_t)(64 * NP);
  size_t slot = home_hash<W>(Form<NP>::source(key, key + 64, 0)) & mask;
#pragma unroll 1
  for (size_t probe = 0; probe <= mask; probe++) {
    const uint32_t old = atomicMin(&slots[slot], carried);
    if (old == kSlotEmpty) return;
    if (old > carried) carried = old;
    slot = (slot + 1) & mask;
  }
}

namespace {
unsigned replace_grid(size_t lanes) {
  const unsigned g = grid_for(lanes, kReplaceBlock);
  return g < kMaxReplaceGrid ? g : kMaxReplaceGrid;
}
}  // namespace

void launch_replace_commit(int npoints, const uint32_t* indices, size_t m, const uint32_t* src_tables,
                           const uint8_t* src_key_ok, const uint8_t* P0, const uint8_t* P1, uint32_t* tables,
                           uint8_t* key_ok, uint8_t* affine_rows, uint8_t* record_rows, hipStream_t s) {
  if (m == 0) return;
  const size_t words = m * (size_t)npoints * (kKeyPointBytes / 16);
  const dim3 grid(replace_grid((words + kCommitUnroll - 1) / kCommitUnroll)), block(kReplaceBlock);
  const uint4* src = reinterpret_cast<const uint4*>(src_tables);
  uint4* dst = reinterpret_cast<uint4*>(tables);
  if (npoints == 1)
    hipLaunchKernelGGL(k_replace_commit<1>, grid, block, 0, s, indices, m, src, src_key_ok, P0, P1, dst, key_ok,
                       affine_rows, record_rows);
  else
    hipLaunchKernelGGL(k_replace_commit<2>, grid, block, 0, s, indices, m, src, src_key_ok, P0, P1, dst, key_ok,
                       affine_rows, record_rows);
}

void launch_rows_to_planar(int npoints, const uint8_t* affine_rows, size_t k, uint8_t* P0, uint8_t* P1,
                           hipStream_t s) {
  if (k == 0) return;
  const dim3 grid(replace_grid(k * 4 * (size_t)npoints)), block(kReplaceBlock);
  const uint4* rows = reinterpret_cast<const uint4*>(affine_rows);
  uint4 *p0 = reinterpret_cast<uint4*>(P0), *p1 = reinterpret_cast<uint4*>(P1);
  if (npoints == 1)
    hipLaunchKernelGGL(k_rows_to_planar<1>, grid, block, 0, s, rows, k, p0, p1);
  else
    hipLaunchKernelGGL(k_rows_to_planar<2>, grid, block, 0, s, rows, k, p0, p1);
}

void launch_index_reinsert(KeyForm form, int npoints, const uint8_t* affine_rows, const uint32_t* reps,
                           uint32_t* slots, size_t mask, hipStream_t s) {
  const dim3 grid(grid_for(mask + 1, kReplaceBlock)), block(kReplaceBlock);
  if (form == kKeyAffine) {
    if (npoints == 1)
      hipLaunchKernelGGL((k_index_reinsert<AffineKey, 1>), grid, block, 0, s, affine_rows, reps, slots, mask);
    else
      hipLaunchKernelGGL((k_index_reinsert<AffineKey, 2>), grid, block, 0, s, affine_rows, reps, slots, mask);
  } else {
    if (npoints == 1)
      hipLaunchKernelGGL((k_index_reinsert<RecordKey, 1>), grid, block, 0, s, affine_rows, reps, slots, mask);
    else
      hipLaunchKernelGGL((k_index_reinsert<RecordKey, 2>), grid, block, 0, s, affine_rows, reps, slots, mask);
  }
}

}  // namespace dsv
