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
// anything else.  The per-item body is k_verify_var's (k_vargen.hip, where the method is described), statement
// for statement, and it is a COPY on purpose, as k_verify_listed's is of k_verify_fixed_half's: k_vargen.hip is
// not to change for this kernel.  A change to either body belongs in both.
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
    u32 yx[8], yy[8], yz[8];
    int sx, sy, sz, top;
    {
      u32 us[8], cs[8], mx[8], my[8], mz[8];
      bool nx, ny, nz;
      load_words8(us, u, i);
      load_words8(cs, c, i);
      good &= words_lt(us, kR32);
      if (!words_lt(us, kR32)) us[7] &= 0x0fffffffu;  // keep the scalars in range; verdict is 0 anyway
      lattice3_scalars(mx, my, mz, nx, ny, nz, us, cs);
      recode_signed4(yx, mx);
      recode_signed4(yy, my);
      recode_signed4(yz, mz);
      u32 nzd[8];
#pragma unroll
      for (int k = 0; k < 8; k++)
        nzd[k] = (yx[k] ^ 0x88888888u) | (yy[k] ^ 0x88888888u) | (yz[k] ^ 0x88888888u);
      top = top_digit4(nzd);
      sx = nx ? -1 : 1;
      sy = ny ? -1 : 1;
      sz = nz ? 1 : -1;  // the chain adds (-z) * R
    }
    {
      Fe gu, gv;
      good &= load_fq(gu, Gen_uv, 2 * i);
      good &= load_fq(gv, Gen_uv, 2 * i + 1);
      build_var_table(tg, gu, gv);
    }
    {
      Fe pku, pkv;
      good &= load_fq(pku, PK_uv, 2 * i);
      good &= load_fq(pkv, PK_uv, 2 * i + 1);
      build_var_table(tp, pku, pkv);
    }
    {
      Fe ru, rv;
      good &= load_fq(ru, R_uv, 2 * i);
      good &= load_fq(rv, R_uv, 2 * i + 1);
      build_var_table(tr, ru, rv);
    }
    Ext acc = ext_from_niels(load_var_entry(tg, sx * sdigit4(yx, top)));
    acc = ext_add_niels(acc, load_var_entry(tp, sy * sdigit4(yy, top)));
    acc = ext_add_niels(acc, load_var_entry(tr, sz * sdigit4(yz, top)));
    {
      const int k0 = top > 0 ? top - 1 : 0;
      RawNiels ea = load_var_entry_raw(tg, sx * sdigit4(yx, k0));
#pragma unroll 1
      for (int k = top - 1; k >= 0; k--) {
        acc = ext_mul16(acc);
        const RawNiels eb = load_var_entry_raw(tp, sy * sdigit4(yy, k));
        acc = ext_add_niels(acc, finish_var_entry(ea));
        const RawNiels ec = load_var_entry_raw(tr, sz * sdigit4(yz, k));
        acc = ext_add_niels(acc, finish_var_entry(eb));
        const int kn = k > 0 ? k - 1 : 0;  // last round: reloads its own entry, unused
        ea = load_var_entry_raw(tg, sx * sdigit4(yx, kn));
        acc = ext_add_niels(acc, finish_var_entry(ec));
      }
    }
    // T == O  <=>  u == 0 and v == z
    good &= (bool)((int)fe_is_zero_canon(fe_canon(acc.u)) & (int)fe_equal(acc.v, acc.z));
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
