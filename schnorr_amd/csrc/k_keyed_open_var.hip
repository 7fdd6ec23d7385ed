// k_keyed_open_var.hip — the var-generator miss branch of the open-set verify by key value (keyed_open.h;
// dsv_verify_vargen_keyed_open*): the unkeyed three-base equation of k_verify_var (k_vargen.hip) over the list
// that k_miss_list (k_keyed_open.hip) wrote.
#include "common.h"
#include "decode29.h"
#include "inv29.h"
#include "lattice3.h"
#include "quad29.h"
#include "keyed_open.h"

namespace dsv {

// ------------------------------------------------------------------------------------------
// k_verify_var over list[0 .. min(*count, n)): lane j verifies item list[j] — every column at that row — and
// overwrites its verdict; the three per-lane window tables (Gen, PK, R) are addressed by workgroup and lane as
// there.  The launch is sized for n items: a workgroup past the end of the list returns before it touches
// anything else.  The per-item body is k_verify_var's (k_vargen.hip, where the method is described): one text,
// verify_var_item_body.h, included by both.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kVerifyBlock, kWavesVerify)
k_verify_var_listed(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c,
                    const uint8_t* __restrict__ PK_uv, const uint8_t* __restrict__ Gen_uv,
                    const uint8_t* __restrict__ R_uv, const uint8_t* __restrict__ valid, size_t n,
                    uint8_t* __restrict__ ok, u32* __restrict__ var_tables, const u32* __restrict__ list,
                    const u32* __restrict__ count) {
  size_t listed = *count;
  if (listed > n) listed = n;
  if ((size_t)blockIdx.x * kVerifyBlock >= listed) return;
  u32* tg = var_tables + ((size_t)blockIdx.x * kVerifyBlock + threadIdx.x) * (3 * kVarLaneWords);
  u32* tp = tg + kVarLaneWords;
  u32* tr = tp + kVarLaneWords;
#pragma unroll 1
  for (size_t base = (size_t)blockIdx.x * kVerifyBlock; base < listed;
       base += (size_t)gridDim.x * kVerifyBlock) {
    const size_t j = base + threadIdx.x;
    const u32 row = j < listed ? list[j] : kSlotEmpty;  // the list is only ever dereferenced where k_miss_list wrote it
    if (row >= n) continue;                             // (n <= DSV_MAX_BATCH = 2^28: kSlotEmpty is no row)
    const size_t i = row;
    bool good = valid[i] != 0;
    // the per-item body, shared as text with k_verify_var (k_vargen.hip)
#include "verify_var_item_body.h"
    // The row is read from the list AGAIN for the store, through a lane number the compiler cannot see through,
    // so that it does not stay in a register across the window loop (as in k_verify_listed): the kernel this
    // one mirrors rebuilds its row from the workgroup's base and the lane, this one has only the list.  Four
    // bytes, an L2 hit; the same entry that passed the row < n test above (the list is not written meanwhile).
    u32 lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    ok[list[base + lane]] = good ? 1 : 0;
  }
}

void launch_verify_var_listed(const uint8_t* u, const uint8_t* c, const uint8_t* PK_uv, const uint8_t* Gen_uv,
                              const uint8_t* R_uv, const uint8_t* valid, size_t n, uint8_t* ok,
                              uint32_t* var_tables, const uint32_t* list, const uint32_t* count, hipStream_t s) {
  hipLaunchKernelGGL(k_verify_var_listed, dim3(verify_grid(n)), dim3(kVerifyBlock), 0, s, u, c, PK_uv, Gen_uv,
                     R_uv, valid, n, ok, var_tables, list, count);
}

}  // namespace dsv
