// k_keyed_open_wire.hip — the key cache for serialized records (keyed_open_wire.h): the wire index of a key set,
// one lane per new key behind the affine index's launch; the lookup that turns a batch's key RECORDS into the
// key_idx column of the keyed kernels, one lane per item; and the decompression of the key records of the items
// that missed, one lane per key point of a listed item.  The first two move bytes and never touch a field
// element: a hit costs no square root.
#include "keyed_open_wire.h"
#include "keyed_wire.h"
#include "common.h"
#include "decode29.h"

namespace dsv {
namespace {

// a key's record in registers: 2 x 16 B per point
template <int NP>
struct RecWords {
  uint4 q[2 * NP];
};
template <int NP>
__device__ __forceinline__ RecWords<NP> load_record(const uint8_t* __restrict__ rec) {
  RecWords<NP> w;
  const uint4* p = reinterpret_cast<const uint4*>(rec);
#pragma unroll
  for (int j = 0; j < 2 * NP; j++) w.q[j] = p[j];
  return w;
}
// the record of the affine point(s) at row i of a / b (u || v, 64 B each): v, bit 255 = the lowest bit of u
template <int NP>
__device__ __forceinline__ RecWords<NP> compress_key(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                     size_t i) {
  RecWords<NP> w;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    const uint4* pt = reinterpret_cast<const uint4*>((p ? b : a) + i * 64);
    const uint32_t sign = pt[0].x << 31;
    w.q[2 * p] = pt[2];
    w.q[2 * p + 1] = pt[3];
    w.q[2 * p + 1].w = (w.q[2 * p + 1].w & 0x7fffffffu) | sign;
  }
  return w;
}
__device__ __forceinline__ bool same16(const uint4& x, const uint4& y) {
  return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) == 0u;
}
template <int NP>
__device__ __forceinline__ bool same_record(const RecWords<NP>& a, const RecWords<NP>& b) {
  bool eq = true;
#pragma unroll
  for (int j = 0; j < 2 * NP; j++) eq &= same16(a.q[j], b.q[j]);
  return eq;
}
template <int NP>
__device__ __forceinline__ uint32_t home_hash(const RecWords<NP>& w) {
  KeyHash h;
#pragma unroll
  for (int j = 0; j < 2 * NP; j++) {
    h.word(w.q[j].x);
    h.word(w.q[j].y);
    h.word(w.q[j].z);
    h.word(w.q[j].w);
  }
  return h.finish();
}

}  // namespace

// ------------------------------------------------------------------------------------------
// k_append_key_index (k_keyed_lookup.hip) over records, for a fresh set (first = 0) as well: one lane per new key
// (P0 / P1, key_ok: the m new keys' rows; records / slots: the whole wire index).  The lane's record, formed from
// the affine source point by byte operations, goes to row first + j, fenced; a valid key then claims the first
// empty slot from its home slot on.  An occupant below `first` was registered by an earlier call: it is compared
// by the index's own copy, which no lane of this launch writes (rows < first); an occupant from `first` on is a
// lane of this launch and is compared by the source points, compressed on the fly, which nobody writes.  An equal
// occupant keeps the lower index (atomicMin).  As there: a slot never returns to empty,
// an occupant only ever changes to an equal key with a lower index, the table is at most half full, so the walk
// ends; rows < first are never written.  Two valid keys have equal records iff they have equal affine bytes
// (DESIGN.md §10.7), so this index holds the same keys at the same lowest indices as the affine one.
// ------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(kLookupBlock)
k_append_wire_index(const uint8_t* __restrict__ P0, const uint8_t* __restrict__ P1,
                    const uint8_t* __restrict__ key_ok, size_t first, size_t m, uint8_t* records,
                    uint32_t* __restrict__ slots, size_t mask) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  const RecWords<NP> w = compress_key<NP>(P0, P1, j);
  uint4* own = reinterpret_cast<uint4*>(records + (first + j) * (size_t)(32 * NP));
#pragma unroll
  for (int q = 0; q < 2 * NP; q++) own[q] = w.q[q];
  __threadfence();
  if (key_ok[j] == 0) return;
  const uint32_t me = (uint32_t)(first + j);
  size_t slot = home_hash<NP>(w) & mask;
#pragma unroll 1
  for (size_t probe = 0;; probe++) {
    const uint32_t old = atomicCAS(&slots[slot], kSlotEmpty, me);
    if (old == kSlotEmpty) return;
    bool equal = false;
    if (old < first)
      equal = same_record<NP>(w, load_record<NP>(records + (size_t)old * (size_t)(32 * NP)));
    else if (old < first + m)
      equal = same_record<NP>(w, compress_key<NP>(P0, P1, old - first));
    if (equal) {
      atomicMin(&slots[slot], me);
      return;
    }
    if (probe == mask) return;  // unreachable: the table is at most half full, so an empty slot comes first
    slot = (slot + 1) & mask;
  }
}

// ------------------------------------------------------------------------------------------
// k_key_lookup (k_keyed_lookup.hip) over 32 * NP-byte records: one lane per item, grid-stride; the item's record
// in registers, a walk from the home slot that compares against the index's copy of each occupant's record and
// ends at the first empty slot.  k: the set's key count when the call was enqueued; an occupant >= k was appended
// since, is read as an empty slot and ends the walk (exact for the reason given there: every key below k whose
// walk passes this slot was placed while the slot was still empty, so it sits in front of it).
// ------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(kLookupBlock)
k_key_lookup_wire(const uint8_t* __restrict__ pk, size_t n, const uint8_t* __restrict__ records,
                  const uint32_t* __restrict__ slots, size_t mask, size_t k, uint32_t* __restrict__ key_idx,
                  uint32_t* __restrict__ misses) {
  __shared__ uint32_t block_misses;
  if (threadIdx.x == 0) block_misses = 0;
  __syncthreads();
  uint32_t missed = 0;
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const RecWords<NP> w = load_record<NP>(pk + i * (size_t)(32 * NP));
    size_t slot = home_hash<NP>(w) & mask;
    uint32_t found = kSlotEmpty;
#pragma unroll 1
    for (size_t probe = 0;; probe++) {
      const uint32_t occ = slots[slot];
      if (occ >= k) break;  // empty (kSlotEmpty >= k), or a key newer than this call
      if (same_record<NP>(w, load_record<NP>(records + (size_t)occ * (size_t)(32 * NP)))) {
        found = occ;
        break;
      }
      if (probe == mask) break;  // unreachable: an empty slot ends the walk first
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

// ------------------------------------------------------------------------------------------
// The key points of the items that missed.  Lane t takes point p = t % NP of item i = list[t / NP], so the two
// points of one item sit in adjacent lanes of one wave (the block is a multiple of 64 and NP divides 64); the
// launch is sized for n items and a lane past min(*count, n) * NP returns before it touches anything else, as does
// the pair of an entry >= n.  The decoding is k_decompress's (k_misc.hip), step for step, as in
// k_keyed_wire_decode: v < q required, u = n * (n d)^(-1/2) with n = v^2 - 1, d = 1 + d_curve v^2, accepted iff
// u^2 d == n, the root chosen by the sign bit, the same bytes for undecodable input.  The affine point goes to row
// i of P0 / P1, and the item's decode flag is AND-ed into valid[i] — the byte the listed verify kernels start
// from — by one lane of the pair (every listed i is listed once: no other lane touches that byte).
// ------------------------------------------------------------------------------------------
template <int NP>
__global__ void __launch_bounds__(kKeyedWireBlock, kWavesHash)
k_decompress_listed(const uint8_t* __restrict__ pk, size_t n, const u32* __restrict__ list,
                    const u32* __restrict__ count, uint8_t* __restrict__ P0, uint8_t* __restrict__ P1,
                    uint8_t* __restrict__ valid, TsTables ts) {
  size_t listed = *count;
  if (listed > n) listed = n;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= listed * NP) return;  // (both lanes of a pair or neither)
  const size_t i = list[t / NP];
  if (i >= n) return;            // (the pair reads the same entry)
  const int p = (int)(t % NP);
  u32 w[8];
  {
    const uint4* rec = reinterpret_cast<const uint4*>(pk + i * (size_t)(32 * NP));
    const uint4 a = rec[2 * p], b = rec[2 * p + 1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
  }
  const u32 sign = w[7] >> 31;
  w[7] &= 0x7fffffffu;
  bool good = words_lt(w, kQ32);
  const Fe v = fe_to_mont(fe_from_words_plain(w));
  const Fe v2 = fe_sqr(v);
  const Fe num = fe_sub2(v2, fe_one());                          // v^2 - 1
  const Fe den = fe_add(fe_mul(v2, fe_const(kD)), fe_one());     // 1 + d v^2  (never 0: -1/d is a non-square)
  Fe u = fe_mul(num, fe_inv_sqrt(fe_mul(num, den), ts));
  good &= fe_equal(fe_mul(fe_sqr(u), den), num);
  u32 uw[8];
  fe_to_words_plain(uw, fe_from_mont(u));
  if ((uw[0] & 1u) != sign) {                                    // take the other root
    u = fe_neg2(u);
    fe_to_words_plain(uw, fe_from_mont(u));
  }
  uint8_t* out = (NP == 2 && p) ? P1 : P0;
  store_words8(out, 2 * i, uw);
  store_words8(out, 2 * i + 1, w);
  int flag = good ? 1 : 0;
  if (NP == 2) flag &= __shfl_xor(flag, 1);  // the item's other point, in the neighbouring lane
  if (p == 0) valid[i] = (uint8_t)((valid[i] != 0 ? 1 : 0) & flag);
}

void launch_append_wire_index(const uint8_t* P0, const uint8_t* P1, const uint8_t* key_ok, int npoints, size_t first,
                              size_t m, uint8_t* records, uint32_t* slots, size_t mask, hipStream_t s) {
  if (m == 0) return;
  const dim3 grid(grid_for(m, kLookupBlock)), block(kLookupBlock);
  if (npoints == 1)
    hipLaunchKernelGGL(k_append_wire_index<1>, grid, block, 0, s, P0, P1, key_ok, first, m, records, slots, mask);
  else
    hipLaunchKernelGGL(k_append_wire_index<2>, grid, block, 0, s, P0, P1, key_ok, first, m, records, slots, mask);
}

hipError_t launch_key_lookup_wire(const uint8_t* pk, int npoints, size_t n, const uint8_t* records,
                                  const uint32_t* slots, size_t mask, size_t k, uint32_t* key_idx, uint32_t* misses,
                                  hipStream_t s) {
  if (misses) launch_store_word(misses, 0, s);
  if (n == 0) return hipSuccess;
  const unsigned g = grid_for(n, kLookupBlock);
  const dim3 grid(g < kMaxLookupGrid ? g : kMaxLookupGrid), block(kLookupBlock);
  if (npoints == 1)
    hipLaunchKernelGGL(k_key_lookup_wire<1>, grid, block, 0, s, pk, n, records, slots, mask, k, key_idx, misses);
  else
    hipLaunchKernelGGL(k_key_lookup_wire<2>, grid, block, 0, s, pk, n, records, slots, mask, k, key_idx, misses);
  return hipSuccess;
}

void launch_decompress_listed(int npoints, const uint8_t* pk, size_t n, const uint32_t* list, const uint32_t* count,
                              uint8_t* P0, uint8_t* P1, uint8_t* valid, const uint32_t* ts_cancel,
                              const uint8_t* ts_hash, hipStream_t s) {
  if (n == 0) return;
  const TsTables ts{ts_cancel, ts_hash};
  const dim3 grid(grid_for(n * (size_t)npoints, kKeyedWireBlock)), block(kKeyedWireBlock);
  if (npoints == 1)
    hipLaunchKernelGGL(k_decompress_listed<1>, grid, block, 0, s, pk, n, list, count, P0, P1, valid, ts);
  else
    hipLaunchKernelGGL(k_decompress_listed<2>, grid, block, 0, s, pk, n, list, count, P0, P1, valid, ts);
}

}  // namespace dsv
