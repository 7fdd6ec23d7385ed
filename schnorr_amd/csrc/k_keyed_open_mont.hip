// k_keyed_open_mont.hip — the key cache for typed objects (keyed_open_mont.h): one front kernel that normalises
// the nonce points and the key points of a batch of the reference's in-memory objects, converts the two scalars
// and looks the normalised key up in the set's affine index — k_normalize_uvz (k_misc.hip) over all the item's
// points with k_index_lookup<AffineKey> (k_keyed_lookup.hip) at the point where the key's bytes exist, in
// registers, instead of a second launch that reads them back.
#define DSV_INDEX_KERNELS
#include "keyed_open_mont.h"
#include "common.h"
#include "inv29.h"
#include "normalize_items.h"

namespace dsv {

// ------------------------------------------------------------------------------------------
// k_normalize_uvz<NPS + NPK>'s lanes, per_lane, prefix layout and grid (k_misc.hip: Montgomery's trick over the
// NP points of an item and the per_lane items of a lane, one Euclidean inversion per lane, the scalar conversion
// inside), with the points told apart: a.in[0 .. NPS) are the nonce points, written to a.out[0 .. NPS) as there;
// a.in[NPS .. NP) are the key points, whose canonical affine bytes stay in registers as one index row in
// AffineKey<NPK>'s layout (u || v of PK, then of PK' / Gen).  On the way down the key points come first (the
// products are unwound in reverse), so the row is complete before the item's nonce points are; it is then looked
// up if every key limb group was usable (< q, z != 0), and stored — into row i of a.out[NPS ..), the miss branch's
// own key columns — only if the item misses.  valid[i] is k_normalize_uvz's: every limb group of every point < q,
// every z != 0.  An item with unusable key limbs is a miss with valid[i] = 0 (its row is stored like every miss's:
// the listed kernels read it, valid[i] decides).  The misses of a wave meet in one atomic; no lane leaves before
// the wave's sum (the block may be a single wave: the host pipeline asks for that).
// ------------------------------------------------------------------------------------------
template <int NPS, int NPK>
__global__ void __launch_bounds__(256)
k_normalize_lookup(NormalizeArgs a, size_t n, size_t lanes, int per_lane, uint8_t* __restrict__ valid,
                   u32* __restrict__ prefix, const uint8_t* __restrict__ rows, const uint32_t* __restrict__ slots,
                   size_t mask, size_t nkeys, uint32_t* __restrict__ key_idx, uint32_t* __restrict__ misses) {
  constexpr int NP = NPS + NPK;
  constexpr int W = 4 * NPK;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t missed = 0;
  if (t < lanes) {
    Fe acc = fe_one();
    u32 okmask = 0, keymask = 0;
#pragma unroll 1
    for (int k = 0; k < per_lane; k++) {
      const size_t i = (size_t)k * lanes + t;
      if (i >= n) break;
      bool ok = true, key_ok = true;
      auto up = [&](int p, bool& flag) {
        const Fe z = load_z_for_product(a.in[p], i, flag);
        store_fe_words(prefix + ((size_t)(k * NP + p) * lanes + t) * NL, acc);
        acc = fe_mul(acc, z);
      };
      up(0, ok);
      if (NPS > 1) up(1, ok);
      up(NPS, key_ok);
      if (NPK > 1) up(NPS + 1, key_ok);
      okmask |= (ok ? 1u : 0u) << k;
      keymask |= (key_ok ? 1u : 0u) << k;
      scalars_from_mont_item(a.u_mont, a.m_mont, i, a.u_out, a.m_out);
    }
    Fe inv = fe_invert_euclid(acc);  // the lane's one dependent chain (inv29.h)
#pragma unroll 1
    for (int k = per_lane - 1; k >= 0; k--) {
      const size_t i = (size_t)k * lanes + t;
      if (i >= n) continue;
      bool ok = (okmask >> k) & 1, key_ok = (keymask >> k) & 1;
      // point p's quotients: o[0] = u / z, o[1] = v / z, canonical words
      auto down = [&](int p, bool& flag, u32 (&ou)[8], u32 (&ov)[8]) {
        bool dummy = true;
        const Fe z = load_z_for_product(a.in[p], i, dummy);
        const Fe pre = load_fe_words(prefix + ((size_t)(k * NP + p) * lanes + t) * NL);
        const Fe zinv = fe_mul(inv, pre);  // 1/z in Montgomery form
        inv = fe_mul(inv, z);
        // plain coordinate x Montgomery 1/z = plain quotient: no conversion in either direction
        u32 w[8];
        load_words8(w, a.in[p], 3 * i);
        flag &= words_lt(w, kQ32);
        fe_to_words_plain(ou, fe_canon(fe_mul(fe_from_words_plain(w), zinv)));
        load_words8(w, a.in[p], 3 * i + 1);
        flag &= words_lt(w, kQ32);
        fe_to_words_plain(ov, fe_canon(fe_mul(fe_from_words_plain(w), zinv)));
      };
      Words<W> row;
      auto down_key = [&](int j) {  // key point j -> words 4 j .. 4 j + 3 of the row
        u32 ou[8], ov[8];
        down(NPS + j, key_ok, ou, ov);
        row.q[4 * j] = make_uint4(ou[0], ou[1], ou[2], ou[3]);
        row.q[4 * j + 1] = make_uint4(ou[4], ou[5], ou[6], ou[7]);
        row.q[4 * j + 2] = make_uint4(ov[0], ov[1], ov[2], ov[3]);
        row.q[4 * j + 3] = make_uint4(ov[4], ov[5], ov[6], ov[7]);
      };
      auto down_nonce = [&](int p) {
        u32 ou[8], ov[8];
        down(p, ok, ou, ov);
        store_words8(a.out[p], 2 * i, ou);
        store_words8(a.out[p], 2 * i + 1, ov);
      };
      if (NPK > 1) down_key(1);
      down_key(0);
      // (a set without an index has nkeys = 0 and no rows or slots: nothing is read)
      const uint32_t found = key_ok && nkeys ? walk_index<W>(row, rows, slots, mask, nkeys) : kSlotEmpty;
      key_idx[i] = found;
      if (found == kSlotEmpty) {
        missed++;
        uint4* oa = reinterpret_cast<uint4*>(a.out[NPS] + i * 64);
#pragma unroll
        for (int j = 0; j < 4; j++) oa[j] = row.q[j];
        if (NPK > 1) {
          uint4* ob = reinterpret_cast<uint4*>(a.out[NPS + NPK - 1] + i * 64);
#pragma unroll
          for (int j = 0; j < 4; j++) ob[j] = row.q[4 * (NPK - 1) + j];
        }
      }
      if (NPS > 1) down_nonce(1);
      down_nonce(0);
      valid[i] = (ok & key_ok) ? 1 : 0;
    }
  }
  if (!misses) return;  // (uniform: every lane of the grid takes the same side)
#pragma unroll
  for (int off = warpSize / 2; off > 0; off >>= 1) missed += __shfl_down(missed, off);
  if ((threadIdx.x & (warpSize - 1)) == 0 && missed) atomicAdd(misses, missed);
}

// the two-launch front's gate (keyed_open_mont.h): what `key_ok` decides inside k_normalize_lookup, from the limbs
__global__ void __launch_bounds__(256)
k_unusable_keys_miss(const uint8_t* __restrict__ key_a, const uint8_t* __restrict__ key_b, size_t n,
                     uint32_t* __restrict__ key_idx, uint32_t* __restrict__ count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || key_idx[i] == kSlotEmpty) return;
  bool usable = true;
  for (int p = 0; p < 2; p++) {
    const uint8_t* in = p ? key_b : key_a;
    if (!in) continue;
    u32 w[8];
    for (int c = 0; c < 3; c++) {
      load_words8(w, in, 3 * i + c);
      usable &= words_lt(w, kQ32);
    }
    usable &= (w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0;  // (the last group read: z)
  }
  if (usable) return;
  key_idx[i] = kSlotEmpty;
  if (count) atomicAdd(count, 1u);
}
void launch_unusable_keys_miss(const uint8_t* key_a, const uint8_t* key_b, int npk, size_t n, uint32_t* key_idx,
                               uint32_t* count, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_unusable_keys_miss, dim3(grid_for(n)), dim3(256), 0, s, key_a, npk == 2 ? key_b : nullptr, n,
                     key_idx, count);
}

void launch_normalize_lookup(const NormalizeArgs& a, int nps, int npk, size_t n, uint8_t* valid, uint32_t* prefix,
                             const uint8_t* rows, const uint32_t* slots, size_t mask, size_t k, uint32_t* key_idx,
                             uint32_t* misses, hipStream_t s, int want_per_lane, int block_threads) {
  if (n == 0) return;
  int per_lane;
  const size_t lanes = normalize_lanes(n, per_lane, want_per_lane);
  const unsigned bt = block_threads > 0 ? (unsigned)block_threads : 256u;
  const dim3 grid(grid_for(lanes, bt)), block(bt);
#define DSV_NL(NPS, NPK)                                                                                        \
  hipLaunchKernelGGL((k_normalize_lookup<NPS, NPK>), grid, block, 0, s, a, n, lanes, per_lane, valid, prefix, rows, \
                     slots, mask, k, key_idx, misses)
  if (nps == 2) DSV_NL(2, 2);
  else if (npk == 2) DSV_NL(1, 2);
  else DSV_NL(1, 1);
#undef DSV_NL
}

}  // namespace dsv
