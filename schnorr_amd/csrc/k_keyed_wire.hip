// k_keyed_wire.hip — the decode pass of the keyed wire form (keyed_wire.h): `Signature::from_bytes` /
// `SignatureDouble::from_bytes` / `SignatureVarGen::from_bytes` (dusk-schnorr src/signatures.rs:117-122,
// :261-269, :398-403) for a batch whose keys are registered — the records' nonce points are decompressed,
// u is copied out, and one validity byte per item says whether every nonce point decoded.  It stands where
// the unkeyed wire path runs k_gather32 and one k_decompress per point (k_misc.hip), the second of them
// reading `valid` back to AND into it: here an item's flags meet in registers.
#include "keyed_wire.h"
#include "common.h"
#include "decode29.h"

namespace dsv {

// One lane per nonce point: lane t decodes point p = t % NS of item i = t / NS, so the two points of a
// double item sit in adjacent lanes of one wave (the block is a multiple of 64 and NS divides 64) and a
// small batch has the latency of one square root.  The decoding is k_decompress's, step for step:
// v < q required, u = n * (n d)^(-1/2) with n = v^2 - 1, d = 1 + d_curve v^2, accepted iff u^2 d == n, the
// root chosen by the sign bit, no further canonicity or subgroup test, the same bytes for undecodable input.
// u: the record's first 32 bytes as they lie, 32 / NS of them per lane (the keyed kernel checks u < r).
template <int SCHEME>
__global__ void __launch_bounds__(kKeyedWireBlock, kWavesHash)
k_keyed_wire_decode(const uint8_t* __restrict__ sig, size_t n, uint8_t* __restrict__ u_out,
                    uint8_t* __restrict__ R_uv, uint8_t* __restrict__ Rp_uv, uint8_t* __restrict__ valid,
                    TsTables ts) {
  constexpr int NS = SCHEME == 1 ? 2 : 1;
  constexpr size_t kRec = 32 + 32 * (size_t)NS;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * NS) return;  // (both lanes of a pair or neither: n * NS and the lane count are multiples of NS)
  const size_t i = t / NS;
  const int p = (int)(t % NS);
  const uint4* rec = reinterpret_cast<const uint4*>(sig + i * kRec);
  {
    uint4* o = reinterpret_cast<uint4*>(u_out + i * 32);
    if (NS == 1) {
      o[0] = rec[0];
      o[1] = rec[1];
    } else {
      o[p] = rec[p];
    }
  }
  u32 w[8];
  {
    const uint4 a = rec[2 + 2 * p], b = rec[3 + 2 * p];
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
  uint8_t* out = (NS == 2 && p) ? Rp_uv : R_uv;
  store_words8(out, 2 * i, uw);
  store_words8(out, 2 * i + 1, w);
  int flag = good ? 1 : 0;
  if (NS == 2) flag &= __shfl_xor(flag, 1);  // the item's other point, in the neighbouring lane
  if (p == 0) valid[i] = (uint8_t)flag;
}

void launch_keyed_wire_decode(int scheme, const uint8_t* sig, size_t n, uint8_t* u, uint8_t* R_uv, uint8_t* Rp_uv,
                              uint8_t* valid, const uint32_t* ts_cancel, const uint8_t* ts_hash, hipStream_t s) {
  if (n == 0) return;
  const TsTables ts{ts_cancel, ts_hash};
  const dim3 grid(grid_for(n * (size_t)keyed_sig_points(scheme), kKeyedWireBlock)), block(kKeyedWireBlock);
  if (scheme == 0)
    hipLaunchKernelGGL(k_keyed_wire_decode<0>, grid, block, 0, s, sig, n, u, R_uv, Rp_uv, valid, ts);
  else if (scheme == 1)
    hipLaunchKernelGGL(k_keyed_wire_decode<1>, grid, block, 0, s, sig, n, u, R_uv, Rp_uv, valid, ts);
  else
    hipLaunchKernelGGL(k_keyed_wire_decode<2>, grid, block, 0, s, sig, n, u, R_uv, Rp_uv, valid, ts);
}

}  // namespace dsv
