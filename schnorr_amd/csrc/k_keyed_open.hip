// k_keyed_open.hip — the miss branch of the open-set verify by key value (keyed_open.h): the list of the items
// whose key the lookup did not find, and the unkeyed equation of k_verify_fixed_half (k_verify.hip) over that
// list.
#include "common.h"
#include "halfgcd.h"
#include "keyed_open.h"

namespace dsv {

// ------------------------------------------------------------------------------------------
// One lane per item, grid-stride in whole waves (every lane of a wave makes the same number of trips, so the
// ballot sees all 64): a wave that holds misses reserves their places with ONE atomic, a lane's place is the
// reserved base plus the number of misses in the lanes below it.  At most n places are ever reserved.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMissBlock)
k_miss_list(const u32* __restrict__ key_idx, size_t n, u32* __restrict__ list, u32* __restrict__ count) {
  const u32 lane = threadIdx.x & (u32)(warpSize - 1);
#pragma unroll 1
  for (size_t base = (size_t)blockIdx.x * kMissBlock + (threadIdx.x - lane); base < n;
       base += (size_t)gridDim.x * kMissBlock) {
    const size_t i = base + lane;
    const bool miss = i < n && key_idx[i] == kSlotEmpty;
    const unsigned long long wave = __ballot(miss);
    if (wave == 0) continue;
    u32 first = 0;
    if (lane == (u32)__builtin_ctzll(wave)) first = atomicAdd(count, (u32)__popcll(wave));
    first = __shfl(first, __builtin_ctzll(wave));
    if (miss) list[first + (u32)__popcll(wave & ((1ull << lane) - 1ull))] = (u32)i;
  }
}

// ------------------------------------------------------------------------------------------
// The verdict of item i = list[base + lane]: valid[i] & [every chain's equation holds]; tbl: the lane's window table.  The
// body is k_verify_fixed_half's (k_verify.hip, where the method is described): one text, verify_half_item_body.h,
// included by both.
// ------------------------------------------------------------------------------------------
template <int NCHAIN>
DSV_DEV bool listed_item_ok(const uint8_t* u, const uint8_t* c, const ChainOperands& op0, const ChainOperands& op1,
                            const uint8_t* valid, size_t i, const JointTable& tbl,
                            const u32* list, size_t base) {
  bool good = valid[i] != 0;
  // The chain's points are addressed by the row read from the list AGAIN (as for the store of the verdict in
  // k_verify_listed): k_verify_fixed_half rebuilds its row from the workgroup's base and the lane, here it would
  // stay in a register — with the addresses made from it — across the first chain's window loop, and the
  // two-chain kernel spilled more than k_verify_fixed_half<2> (tests/test_keyset_open_abi.py).
#define DSV_ITEM_ROW_SETUP       \
  u32 lane = threadIdx.x;        \
  asm volatile("" : "+v"(lane)); \
  const size_t r = list[base + lane];
#define DSV_ITEM_ROW r
#include "verify_half_item_body.h"
#undef DSV_ITEM_ROW
#undef DSV_ITEM_ROW_SETUP
  return good;
}

// ------------------------------------------------------------------------------------------
// k_verify_fixed_half over list[0 .. min(*count, n)): lane j verifies item list[j] — every column at that row —
// and overwrites its verdict; the per-lane window tables are addressed by workgroup and lane as there.  The
// launch is sized for n items: a workgroup past the end of the list returns before it touches anything else.
// ------------------------------------------------------------------------------------------
template <int NCHAIN>
__global__ void __launch_bounds__(kVerifyBlock, kWavesVerify)
k_verify_listed(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c, ChainOperands op0, ChainOperands op1,
                const uint8_t* __restrict__ valid, size_t n, uint8_t* __restrict__ ok,
                u32* __restrict__ var_tables, const u32* __restrict__ list, const u32* __restrict__ count) {
  size_t listed = *count;
  if (listed > n) listed = n;
  if ((size_t)blockIdx.x * kVerifyBlock >= listed) return;
  __shared__ uint4 top_limbs[kJointLdsVectors];  // limb 8 of the lane-private window entries (common.h)
  const JointTable tbl = joint_table_of_lane(var_tables, top_limbs);
#pragma unroll 1
  for (size_t base = (size_t)blockIdx.x * kVerifyBlock; base < listed;
       base += (size_t)gridDim.x * kVerifyBlock) {
    const size_t j = base + threadIdx.x;
    const u32 i = j < listed ? list[j] : kSlotEmpty;  // the list is only ever dereferenced where k_miss_list wrote it
    if (i >= n) continue;                             // (n <= DSV_MAX_BATCH = 2^28: kSlotEmpty is no row)
    const bool good = listed_item_ok<NCHAIN>(u, c, op0, op1, valid, i, tbl, list, base);
    // The row is read from the list AGAIN for the store, through a lane number the compiler cannot see through,
    // so that it does not stay in a register across the window loop: the kernel this one mirrors rebuilds its
    // row from the workgroup's base and the lane, this one has only the list — and with the row kept live it
    // spilled more registers than k_verify_fixed_half (tests/test_keyset_open_abi.py).  Four bytes, an L2 hit.
    u32 lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    ok[list[base + lane]] = good ? 1 : 0;
  }
}

hipError_t launch_miss_list(const uint32_t* key_idx, size_t n, uint32_t* list, uint32_t* count, hipStream_t s) {
  launch_store_word(count, 0, s);
  if (n == 0) return hipSuccess;
  const unsigned g = grid_for(n, kMissBlock);
  hipLaunchKernelGGL(k_miss_list, dim3(g < kMaxMissGrid ? g : kMaxMissGrid), dim3(kMissBlock), 0, s, key_idx, n,
                     list, count);
  return hipSuccess;
}

void launch_verify_listed(int nchain, const uint8_t* u, const uint8_t* c, ChainOperands op0, ChainOperands op1,
                          const uint8_t* valid, size_t n, uint8_t* ok, uint32_t* var_tables, const uint32_t* list,
                          const uint32_t* count, hipStream_t s) {
  const dim3 grid(verify_grid(n)), block(kVerifyBlock);
  if (nchain == 2)
    hipLaunchKernelGGL(k_verify_listed<2>, grid, block, 0, s, u, c, op0, op1, valid, n, ok, var_tables, list,
                       count);
  else
    hipLaunchKernelGGL(k_verify_listed<1>, grid, block, 0, s, u, c, op0, op1, valid, n, ok, var_tables, list,
                       count);
}

}  // namespace dsv
