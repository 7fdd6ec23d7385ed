// k_keyed_open_wire.hip — the key cache for serialized records (keyed_open_wire.h): the decompression of the key
// records of the items that missed the set's record index (k_keyed_lookup.hip), one lane per key point of a listed
// item.
#include "keyed_open_wire.h"
#include "keyed_wire.h"
#include "common.h"
#include "decode29.h"

namespace dsv {

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
