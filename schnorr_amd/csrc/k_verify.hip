// k_verify.hip — the dominant kernel: ok &= [ u*Gen + c*PK == R ] for Gen = G / G' given by its
// fixed-base table (`PublicKey::verify`, `PublicKeyDouble::verify`,
// /root/reference/src/keys/public.rs:121-130, :222-244), evaluated with half-size scalars
// (halfgcd.h): with (a, b), a = b*c (mod 8r), b odd,
//   u*G + c*PK == R   <=>   (b*u mod r)*G + a*PK - b*R == O.
// ONE per-lane window table over both variable bases — the 11 combinations da*PK + db*R of signed
// 2-bit digits in [-1, 2] (common.h: build_joint_table) — and one Straus chain of ~66 windows of two doublings
// and ONE addition each, whose length is the lane's own max(bitlen a, bitlen b) (lanes of a wave
// simply leave the loop at different times); then 16 mixed additions from the fixed-base table;
// the verdict is an identity test.  (r01 - r03a: one 4-bit table of 8 entries per base, two
// additions per four doublings: the same chain, but 116 multiplications of table building per
// chain instead of 67 + 12 squarings and 16 entries written per lane instead of 11: +2.1 % single,
// +2.5 % double, same-box A/B profiles/r03/ab_joint_windows.txt.)
//
// NCHAIN = 2 is PublicKeyDouble::verify in ONE launch: both equations share u and c, so (a, b), both
// recodings and b*u mod r are computed once and the chain runs twice — (G, PK, R) then (G', PK', R')
// — through the same code (a rolled loop over the two operand sets: the hot loop exists once in
// the instruction cache) and the same table slot.
#include "common.h"
#include "halfgcd.h"

namespace dsv {

template <int NCHAIN>
__global__ void __launch_bounds__(kVerifyBlock, kWavesVerify)
k_verify_fixed_half(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c, ChainOperands op0,
                    ChainOperands op1, const uint8_t* __restrict__ valid, bool accumulate, size_t n,
                    uint8_t* __restrict__ ok, u32* __restrict__ var_tables, const u32* __restrict__ gate) {
  if (gate_says_done(gate)) return;  // the batch fast accept decided these items (launch.h)
  __shared__ uint4 top_limbs[kJointLdsVectors];  // limb 8 of the lane-private window entries (common.h)
  const JointTable tbl = joint_table_of_lane(var_tables, top_limbs);
#pragma unroll 1
  for (size_t base = (size_t)blockIdx.x * kVerifyBlock; base < n;
       base += (size_t)gridDim.x * kVerifyBlock) {
    const size_t i = base + threadIdx.x;
    if (i >= n) continue;
    bool good = accumulate ? (ok[i] != 0) : (valid[i] != 0);
    // the per-item body, shared as text with k_verify_listed (k_keyed_open.hip); the points lie at the item's row
#define DSV_ITEM_ROW_SETUP
#define DSV_ITEM_ROW i
#include "verify_half_item_body.h"
#undef DSV_ITEM_ROW
#undef DSV_ITEM_ROW_SETUP
    ok[i] = good ? 1 : 0;
  }
}

void launch_verify_half(int nchain, bool accumulate, const uint8_t* u, const uint8_t* c,
                        ChainOperands op0, ChainOperands op1, const uint8_t* valid, size_t n,
                        uint8_t* ok, uint32_t* var_tables, hipStream_t s, const uint32_t* gate) {
  const dim3 grid(verify_grid(n)), block(kVerifyBlock);
  if (nchain == 2)
    hipLaunchKernelGGL(k_verify_fixed_half<2>, grid, block, 0, s, u, c, op0, op1, valid, accumulate, n,
                       ok, var_tables, gate);
  else
    hipLaunchKernelGGL(k_verify_fixed_half<1>, grid, block, 0, s, u, c, op0, op1, valid, accumulate, n,
                       ok, var_tables, gate);
}

}  // namespace dsv
