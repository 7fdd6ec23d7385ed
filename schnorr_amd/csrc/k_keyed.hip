// k_keyed.hip — registered key sets (keyed.h): construction of the per-key fixed-base tables and the
// keyed verify kernel, `PublicKey::verify` / `PublicKeyDouble::verify` / `PublicKeyVarGen::verify`
// (dusk-schnorr src/keys/public.rs:121-130, :222-244, :401-415) with the key given by its index.
// u and c enter as the integers they are (never reduced mod r, no cofactor clearing): the verdict is the
// reference's for identity and small-order keys and nonce points too.
#define DSV_KEYED_KERNELS 1
#include "keyed.h"
#include "inv29.h"

namespace dsv {

// -u^2 + v^2 == 1 + d u^2 v^2, as 2 v^2 == 2 u^2 + 2 + (2d) u^2 v^2 (u, v: fe_mul outputs)
DSV_DEV bool key_on_curve(const Fe& u, const Fe& v) {
  const Fe uu = fe_sqr(u), vv = fe_sqr(v);
  const Fe rhs = fe_mul(fe_mul(uu, vv), fe_const(kD2));
  const Fe a = fe_carry(fe_dbl(vv));
  const Fe b0 = fe_carry(fe_add(fe_dbl(uu), fe_dbl(fe_one())));
  const Fe b = fe_carry(fe_add(b0, rhs));
  return fe_equal(a, b);
}

DSV_DEV void store_key_entry(u32* e, const Fe& vpu, const Fe& vmu, const Fe& t2d, const Fe& nt2d) {
#pragma unroll
  for (int i = 0; i < NL; i++) {
    e[i] = vpu.l[i];
    e[NL + i] = vmu.l[i];
    e[2 * NL + i] = t2d.l[i];
    e[3 * NL + i] = nt2d.l[i];
  }
}

// ------------------------------------------------------------------------------------------
// One lane per (key, point, window w): B = 2^(8w) * P by 8w doublings, then d * B for d = 1 .. 128 by
// running additions, all 128 normalised with ONE inversion (Montgomery's trick).  On the way up the
// entry slots themselves hold the projective (U, V, Z) of d * B and the running product Z_1 .. Z_d
// (27 + 9 of an entry's 36 words); on the way down entry d is read back, its 1/Z_d taken from the
// product in slot d - 1, and the slot overwritten with the finished affine niels entry.
// An invalid key (coordinate >= q, off the curve) still gets a table of whatever its arithmetic yields
// (z = 0 inverts to 0; no branch depends on it); key_ok keeps every verdict under it at 0.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kKeyBuildBlock)
k_build_key_tables(const uint8_t* __restrict__ P0, const uint8_t* __restrict__ P1,
                   const uint8_t* __restrict__ valid_in, int npoints, size_t k, u32* __restrict__ tables,
                   uint8_t* __restrict__ key_ok) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= k * (size_t)npoints * kKeyWindows) return;
  const int w = (int)(lane % kKeyWindows);
  const size_t kp = lane / kKeyWindows;  // key * npoints + point
  const int p = (int)(kp % (size_t)npoints);
  const size_t key = kp / (size_t)npoints;
  Fe pu, pv;
  (void)load_fq(pu, p ? P1 : P0, 2 * key);
  (void)load_fq(pv, p ? P1 : P0, 2 * key + 1);
  if (w == 0 && p == 0) {
    bool good = valid_in ? valid_in[key] != 0 : true;
    for (int pt = 0; pt < npoints; pt++) {
      Fe a, b;
      good &= load_fq(a, pt ? P1 : P0, 2 * key);
      good &= load_fq(b, pt ? P1 : P0, 2 * key + 1);
      good &= key_on_curve(a, b);
    }
    key_ok[key] = good ? 1 : 0;
  }
  u32* win = tables + kp * kKeyPointWords + (size_t)w * kKeyEntries * kEntryWords;

  // B = 2^(8w) * P
  Ext B = ext_from_affine(pu, pv);
  if (w > 0) {
    Fe u = pu, v = pv, z = fe_one();
#pragma unroll 1
    for (int j = 0; j < kKeyBits * w - 1; j++) ext_double_uvz(u, v, z);
    Ext q;
    q.u = u;
    q.v = v;
    q.z = z;
    B = ext_double(q);
  }
  const Niels nB = ext_to_niels(B);

  // up: d * B projective, running products of the z's
  Ext cur = B;
  Fe prod = cur.z;
#pragma unroll 1
  for (int d = 1; d < kKeyEntries; d++) {
    if (d > 1) {
      cur = ext_add_niels(cur, nB);
      prod = fe_mul(prod, cur.z);
    }
    u32* e = win + (size_t)d * kEntryWords;
    store_fe_words(e, cur.u);
    store_fe_words(e + NL, cur.v);
    store_fe_words(e + 2 * NL, cur.z);
    store_fe_words(e + 3 * NL, prod);
  }

  // down: inv = 1 / (Z_1 .. Z_d) at the top of each step
  Fe inv = fe_invert_euclid(prod);
#pragma unroll 1
  for (int d = kKeyEntries - 1; d >= 1; d--) {
    u32* e = win + (size_t)d * kEntryWords;
    const Fe U = load_fe_words(e), V = load_fe_words(e + NL), Z = load_fe_words(e + 2 * NL);
    const Fe below = d > 1 ? load_fe_words(e - kEntryWords + 3 * NL) : fe_one();
    const Fe zi = fe_mul(inv, below);
    inv = fe_mul(inv, Z);
    const Fe u = fe_mul(U, zi), v = fe_mul(V, zi);
    const Fe t2d = fe_mul(fe_mul(u, v), fe_const(kD2));
    store_key_entry(e, fe_canon(fe_add(v, u)), fe_canon(fe_sub2(v, u)), fe_canon(t2d), fe_canon(fe_neg2(t2d)));
  }
  // entry 0: the identity (v+u = v-u = 1, 2d*uv = 0)
  store_key_entry(win, fe_canon(fe_one()), fe_canon(fe_one()), fe_zero(), fe_zero());
}

// ------------------------------------------------------------------------------------------
// One lane per item, grid-stride (keyed.h: keyed_item_ok).
// ------------------------------------------------------------------------------------------
template <int SCHEME>
__global__ void __launch_bounds__(kKeyedBlock)
k_verify_keyed(const uint8_t* __restrict__ u, const uint8_t* __restrict__ c, const uint8_t* __restrict__ valid,
               const uint8_t* __restrict__ R_uv, const uint8_t* __restrict__ Rp_uv,
               const u32* __restrict__ key_idx, size_t n, const u32* __restrict__ tables,
               const uint8_t* __restrict__ key_ok, size_t k, const u32* __restrict__ gtab0,
               const u32* __restrict__ gtab1, uint8_t* __restrict__ ok) {
#pragma unroll 1
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    ok[i] = keyed_item_ok<SCHEME>(u, c, valid, R_uv, Rp_uv, key_idx, i, tables, key_ok, k, gtab0, gtab1) ? 1 : 0;
}

// affine (u, v) of an entry: u = ((v+u) - (v-u)) / 2, v = ((v+u) + (v-u)) / 2, canonical LE
DSV_DEV void halve_words(u32 (&w)[8]) {  // w < q: w / 2 mod q
  const bool odd = w[0] & 1u;
  u32 carry = 0;
  u32 t[9];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const u64 s = (u64)w[i] + (odd ? kQ32[i] : 0u) + carry;
    t[i] = (u32)s;
    carry = (u32)(s >> 32);
  }
  t[8] = carry;
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = __funnelshift_r(t[i], t[i + 1], 1);
}
__global__ void k_key_entry(const u32* __restrict__ entry, int negate, uint8_t* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const Fe a = load_fe_words(entry + (negate ? NL : 0)), b = load_fe_words(entry + (negate ? 0 : NL));
  u32 wu[8], wv[8];
  fe_to_words_plain(wu, fe_from_mont(fe_sub2(a, b)));
  fe_to_words_plain(wv, fe_from_mont(fe_add(a, b)));
  halve_words(wu);
  halve_words(wv);
  store_words8(out, 0, wu);
  store_words8(out, 1, wv);
}

void launch_build_key_tables(const uint8_t* P0, const uint8_t* P1, const uint8_t* valid_in, int npoints,
                             size_t k, uint32_t* tables, uint8_t* key_ok, hipStream_t s) {
  const size_t lanes = k * (size_t)npoints * kKeyWindows;
  if (lanes == 0) return;
  hipLaunchKernelGGL(k_build_key_tables, dim3(grid_for(lanes, kKeyBuildBlock)), dim3(kKeyBuildBlock), 0, s, P0,
                     P1, valid_in, npoints, k, tables, key_ok);
}
void launch_verify_keyed(int scheme, const uint8_t* u, const uint8_t* c, const uint8_t* valid,
                         const uint8_t* R_uv, const uint8_t* Rp_uv, const uint32_t* key_idx, size_t n,
                         const uint32_t* tables, const uint8_t* key_ok, size_t k, const uint32_t* gtab0,
                         const uint32_t* gtab1, uint8_t* ok, hipStream_t s) {
  if (n == 0) return;
  const unsigned g = grid_for(n, kKeyedBlock);
  const dim3 grid(g < kMaxKeyedGrid ? g : kMaxKeyedGrid), block(kKeyedBlock);
  if (scheme == 0)
    hipLaunchKernelGGL(k_verify_keyed<0>, grid, block, 0, s, u, c, valid, R_uv, Rp_uv, key_idx, n, tables, key_ok,
                       k, gtab0, gtab1, ok);
  else if (scheme == 1)
    hipLaunchKernelGGL(k_verify_keyed<1>, grid, block, 0, s, u, c, valid, R_uv, Rp_uv, key_idx, n, tables, key_ok,
                       k, gtab0, gtab1, ok);
  else
    hipLaunchKernelGGL(k_verify_keyed<2>, grid, block, 0, s, u, c, valid, R_uv, Rp_uv, key_idx, n, tables, key_ok,
                       k, gtab0, gtab1, ok);
}
void launch_key_entry(const uint32_t* entry, int negate, uint8_t* out64, hipStream_t s) {
  hipLaunchKernelGGL(k_key_entry, dim3(1), dim3(64), 0, s, entry, negate, out64);
}

}  // namespace dsv
