// limb_probe.hip — TEST INFRA: the device field, group-law, Hades and inversion functions of
// schnorr_amd/csrc/*.h run on raw limb records from the host (tests/test_gpu_limbs.py).
//
// Built by schnorr_amd/build.py: build_probe() with the engine's own flags into
// schnorr_amd/libdsv_probe.so, loaded beside libdsv.so (never linked into it, no dsv_init).  It compiles
// the same headers into kernels of its own: it pins the source and this compiler's code for these
// functions, not the instruction stream of k_verify / k_quad / k_hash.
//
// Records are u32 words exactly as the device holds them: a field element is 9 limbs, no
// canonicalisation on load or store.  One kernel per family; every lane of every launched wave runs
// (lanes past the last item redo the last item and skip the store), because the quad ops broadcast
// through DPP and the Hades ops use the matrix cores across the whole wave.
#define DSV_HOST_TABLES 1  // the probe uploads its own Hades round constants
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "fe29.h"
#include "jubjub29.h"
#include "quad29.h"
#include "hades29.h"
#include "decode29.h"
#include "inv29.h"

namespace dsv {
namespace probe {

enum Family { kFe, kPt, kQuad, kHades, kInv };

struct Op {
  const char* name;
  Family fam;
  int sub;        // op within the family
  int in_words;   // per item
  int out_words;  // per item
  int lanes;      // lanes per item
};

enum FeOp { FE_MUL, FE_SQR, FE_ADD, FE_DBL, FE_CARRY, FE_SUB2, FE_SUB2_RAW, FE_SUB4, FE_SUB4W, FE_SUB8, FE_NEG2,
            FE_RIPPLE, FE_COND_SUB1, FE_COND_SUB2, FE_COND_SUB4, FE_COND_SUB8, FE_CANON, FE_FROM_MONT, FE_TO_MONT,
            FE_EQUAL, FE_IS_ZERO_CANON, FE_FROM_WORDS, FE_TO_WORDS };
enum PtOp { PT_DOUBLE, PT_DOUBLE_AFFINE, PT_DOUBLE_UVZ, PT_ADD_NIELS, PT_ADD_ANIELS, PT_ADD_ANIELS_T, PT_ADD_SUB_ANIELS_T,
            PT_ADD_ANIELS_IS_IDENTITY, PT_FROM_NIELS, PT_TO_NIELS, PT_TO_NIELS_T, PT_EQ_AFFINE };
enum QuadOp { Q_DOUBLE_T, Q_DOUBLE, Q_ADD_NIELS, Q_ADD_ANIELS, Q_MUL16, Q_OCTET };
enum HadesOp { H_SBOX, H_MDS5, H_MDS_ROW1, H_MDS_MASK01, H_MDS_MASK11, H_FULL, H_FULL_W1, H_FIRST0, H_FIRST1,
               H_PARTIAL, H_PERMUTE, H_TRUNCATE };
enum InvOp { I_EUCLID, I_FERMAT };

constexpr int F = NL;         // words of a field element
constexpr int EXT = 5 * NL;   // Ext: u, v, z, t1, t2
constexpr int NIE = 4 * NL;   // Niels: vpu, vmu, z, t2d
constexpr int ANI = 3 * NL;   // ANiels: vpu, vmu, t2d
constexpr int QX = 4 * NL;    // QExt: u, v, z, t

const Op kOps[] = {
    {"mul", kFe, FE_MUL, 2 * F, F, 1}, {"sqr", kFe, FE_SQR, F, F, 1}, {"add", kFe, FE_ADD, 2 * F, F, 1},
    {"dbl", kFe, FE_DBL, F, F, 1}, {"carry", kFe, FE_CARRY, F, F, 1}, {"sub2", kFe, FE_SUB2, 2 * F, F, 1},
    {"sub2_raw", kFe, FE_SUB2_RAW, 2 * F, F, 1}, {"sub4", kFe, FE_SUB4, 2 * F, F, 1},
    {"sub4w", kFe, FE_SUB4W, 2 * F, F, 1}, {"sub8", kFe, FE_SUB8, 2 * F, F, 1}, {"neg2", kFe, FE_NEG2, F, F, 1},
    {"ripple", kFe, FE_RIPPLE, F, F, 1}, {"cond_sub_x1", kFe, FE_COND_SUB1, F, F, 1},
    {"cond_sub_x2", kFe, FE_COND_SUB2, F, F, 1}, {"cond_sub_x4", kFe, FE_COND_SUB4, F, F, 1},
    {"cond_sub_x8", kFe, FE_COND_SUB8, F, F, 1}, {"canon", kFe, FE_CANON, F, F, 1},
    {"from_mont", kFe, FE_FROM_MONT, F, F, 1}, {"to_mont", kFe, FE_TO_MONT, F, F, 1},
    {"equal", kFe, FE_EQUAL, 2 * F, 1, 1}, {"is_zero_canon", kFe, FE_IS_ZERO_CANON, F, 1, 1},
    {"from_words_plain", kFe, FE_FROM_WORDS, 8, F, 1}, {"to_words_plain", kFe, FE_TO_WORDS, F, 8, 1},
    {"ext_double", kPt, PT_DOUBLE, EXT, EXT, 1}, {"ext_double_affine", kPt, PT_DOUBLE_AFFINE, 2 * F, EXT, 1},
    {"ext_double_uvz", kPt, PT_DOUBLE_UVZ, 3 * F, 3 * F, 1}, {"ext_add_niels", kPt, PT_ADD_NIELS, EXT + NIE, EXT, 1},
    {"ext_add_aniels", kPt, PT_ADD_ANIELS, EXT + ANI, EXT, 1},
    {"ext_add_aniels_t", kPt, PT_ADD_ANIELS_T, EXT + F + ANI, EXT, 1},
    {"ext_add_sub_aniels_t", kPt, PT_ADD_SUB_ANIELS_T, EXT + F + ANI, 2 * EXT, 1},
    {"ext_add_aniels_is_identity", kPt, PT_ADD_ANIELS_IS_IDENTITY, EXT + ANI, 1, 1},
    {"ext_from_niels", kPt, PT_FROM_NIELS, NIE, EXT, 1}, {"ext_to_niels", kPt, PT_TO_NIELS, EXT, NIE, 1},
    {"ext_to_niels_t", kPt, PT_TO_NIELS_T, EXT + F, NIE, 1}, {"ext_eq_affine", kPt, PT_EQ_AFFINE, EXT + 2 * F, 1, 1},
    {"qext_double_t", kQuad, Q_DOUBLE_T, QX, 4 * QX, 4}, {"qext_double", kQuad, Q_DOUBLE, QX, 4 * QX, 4},
    {"qext_add_niels", kQuad, Q_ADD_NIELS, QX + NIE, 4 * QX, 4},
    {"qext_add_aniels", kQuad, Q_ADD_ANIELS, QX + ANI, 4 * QX, 4}, {"qext_mul16", kQuad, Q_MUL16, QX, 4 * QX, 4},
    {"qext_octet_combine", kQuad, Q_OCTET, 2 * QX, 4 * QX, 8},
    {"hades_sbox", kHades, H_SBOX, F, F, 1}, {"hades_mds", kHades, H_MDS5, 5 * F, 5 * F, 1},
    {"hades_mds_row1", kHades, H_MDS_ROW1, 5 * F, F, 1}, {"hades_mds_mask01", kHades, H_MDS_MASK01, 5 * F, 5 * F, 1},
    {"hades_mds_mask11", kHades, H_MDS_MASK11, 5 * F, 5 * F, 1},
    {"hades_full_round", kHades, H_FULL, 5 * F + 1, 5 * F, 1},
    {"hades_full_round_word1", kHades, H_FULL_W1, 5 * F + 1, F, 1},
    {"hades_first_round_const", kHades, H_FIRST0, 5 * F, 5 * F, 1},
    {"hades_first_round_const_pad", kHades, H_FIRST1, 5 * F, 5 * F, 1},
    {"hades_partial_rounds", kHades, H_PARTIAL, 5 * F, 5 * F, 1}, {"hades_permute", kHades, H_PERMUTE, 5 * F, 5 * F, 1},
    {"poseidon_truncate", kHades, H_TRUNCATE, F, 8, 1},
    {"fe_invert_euclid", kInv, I_EUCLID, F, F, 1}, {"fe_invert", kInv, I_FERMAT, F, F, 1},
};
constexpr int kNumOps = sizeof(kOps) / sizeof(kOps[0]);
constexpr int kBlock = 256;

DSV_DEV Fe ld(const u32* p) {
  Fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.l[i] = p[i];
  return r;
}
DSV_DEV void st(u32* p, const Fe& a) {
#pragma unroll
  for (int i = 0; i < NL; i++) p[i] = a.l[i];
}
DSV_DEV Ext ld_ext(const u32* p) {
  Ext e;
  e.u = ld(p);
  e.v = ld(p + F);
  e.z = ld(p + 2 * F);
  e.t1 = ld(p + 3 * F);
  e.t2 = ld(p + 4 * F);
  return e;
}
DSV_DEV void st_ext(u32* p, const Ext& e) {
  st(p, e.u);
  st(p + F, e.v);
  st(p + 2 * F, e.z);
  st(p + 3 * F, e.t1);
  st(p + 4 * F, e.t2);
}
DSV_DEV Niels ld_niels(const u32* p) {
  Niels n;
  n.vpu = ld(p);
  n.vmu = ld(p + F);
  n.z = ld(p + 2 * F);
  n.t2d = ld(p + 3 * F);
  return n;
}
DSV_DEV ANiels ld_aniels(const u32* p) {
  ANiels n;
  n.vpu = ld(p);
  n.vmu = ld(p + F);
  n.t2d = ld(p + 2 * F);
  return n;
}
DSV_DEV QExt ld_q(const u32* p) {
  QExt e;
  e.u = ld(p);
  e.v = ld(p + F);
  e.z = ld(p + 2 * F);
  e.t = ld(p + 3 * F);
  return e;
}
DSV_DEV void st_q(u32* p, const QExt& e) {
  st(p, e.u);
  st(p + F, e.v);
  st(p + 2 * F, e.z);
  st(p + 3 * F, e.t);
}

// item of this lane (clamped: every lane runs) and whether it stores
struct Slot {
  size_t i;
  bool live;
};
DSV_DEV Slot slot(size_t n, int lanes) {
  const size_t raw = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / lanes;
  Slot s;
  s.live = raw < n;
  s.i = s.live ? raw : n - 1;
  return s;
}

__global__ void __launch_bounds__(kBlock) k_probe_fe(int op, const u32* __restrict__ in, int iw, u32* __restrict__ out,
                                                     int ow, size_t n) {
  const Slot s = slot(n, 1);
  const u32* p = in + s.i * iw;
  u32* o = out + s.i * ow;
  const Fe a = ld(p);
  const Fe b = ld(p + (iw >= 2 * F ? F : 0));
  Fe r = fe_zero();
  u32 flag = 0;
  u32 w[8];
  switch (op) {
    case FE_MUL: r = fe_mul(a, b); break;
    case FE_SQR: r = fe_sqr(a); break;
    case FE_ADD: r = fe_add(a, b); break;
    case FE_DBL: r = fe_dbl(a); break;
    case FE_CARRY: r = fe_carry(a); break;
    case FE_SUB2: r = fe_sub2(a, b); break;
    case FE_SUB2_RAW: r = fe_sub2_raw(a, b); break;
    case FE_SUB4: r = fe_sub4(a, b); break;
    case FE_SUB4W: r = fe_sub4w(a, b); break;
    case FE_SUB8: r = fe_sub8(a, b); break;
    case FE_NEG2: r = fe_neg2(a); break;
    case FE_RIPPLE: r = fe_ripple(a); break;
    case FE_COND_SUB1: r = fe_cond_sub(a, kQx1); break;
    case FE_COND_SUB2: r = fe_cond_sub(a, kQx2); break;
    case FE_COND_SUB4: r = fe_cond_sub(a, kQx4); break;
    case FE_COND_SUB8: r = fe_cond_sub(a, kQx8); break;
    case FE_CANON: r = fe_canon(a); break;
    case FE_FROM_MONT: r = fe_from_mont(a); break;
    case FE_TO_MONT: r = fe_to_mont(a); break;
    case FE_EQUAL: flag = fe_equal(a, b) ? 1u : 0u; break;
    case FE_IS_ZERO_CANON: flag = fe_is_zero_canon(a) ? 1u : 0u; break;
    case FE_FROM_WORDS:
#pragma unroll
      for (int k = 0; k < 8; k++) w[k] = p[k];
      r = fe_from_words_plain(w);
      break;
    case FE_TO_WORDS: fe_to_words_plain(w, a); break;
    default: break;
  }
  if (!s.live) return;
  if (op == FE_EQUAL || op == FE_IS_ZERO_CANON) {
    o[0] = flag;
  } else if (op == FE_TO_WORDS) {
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = w[k];
  } else {
    st(o, r);
  }
}

__global__ void __launch_bounds__(kBlock) k_probe_pt(int op, const u32* __restrict__ in, int iw, u32* __restrict__ out,
                                                     int ow, size_t n) {
  const Slot s = slot(n, 1);
  const u32* p = in + s.i * iw;
  u32* o = out + s.i * ow;
  switch (op) {
    case PT_DOUBLE: {
      const Ext r = ext_double(ld_ext(p));
      if (s.live) st_ext(o, r);
      break;
    }
    case PT_DOUBLE_AFFINE: {
      const Ext r = ext_double_affine(ld(p), ld(p + F));
      if (s.live) st_ext(o, r);
      break;
    }
    case PT_DOUBLE_UVZ: {
      Fe u = ld(p), v = ld(p + F), z = ld(p + 2 * F);
      ext_double_uvz(u, v, z);
      if (s.live) {
        st(o, u);
        st(o + F, v);
        st(o + 2 * F, z);
      }
      break;
    }
    case PT_ADD_NIELS: {
      const Ext r = ext_add_niels(ld_ext(p), ld_niels(p + EXT));
      if (s.live) st_ext(o, r);
      break;
    }
    case PT_ADD_ANIELS: {
      const Ext r = ext_add_aniels(ld_ext(p), ld_aniels(p + EXT));
      if (s.live) st_ext(o, r);
      break;
    }
    case PT_ADD_ANIELS_T: {
      const Ext r = ext_add_aniels_t(ld_ext(p), ld(p + EXT), ld_aniels(p + EXT + F));
      if (s.live) st_ext(o, r);
      break;
    }
    case PT_ADD_SUB_ANIELS_T: {
      Ext sum, diff;
      ext_add_sub_aniels_t(sum, diff, ld_ext(p), ld(p + EXT), ld_aniels(p + EXT + F));
      if (s.live) {
        st_ext(o, sum);
        st_ext(o + EXT, diff);
      }
      break;
    }
    case PT_ADD_ANIELS_IS_IDENTITY: {
      const bool r = ext_add_aniels_is_identity(ld_ext(p), ld_aniels(p + EXT));
      if (s.live) o[0] = r ? 1u : 0u;
      break;
    }
    case PT_FROM_NIELS: {
      const Ext r = ext_from_niels(ld_niels(p));
      if (s.live) st_ext(o, r);
      break;
    }
    case PT_TO_NIELS:
    case PT_TO_NIELS_T: {
      const Niels r = op == PT_TO_NIELS ? ext_to_niels(ld_ext(p)) : ext_to_niels_t(ld_ext(p), ld(p + EXT));
      if (s.live) {
        st(o, r.vpu);
        st(o + F, r.vmu);
        st(o + 2 * F, r.z);
        st(o + 3 * F, r.t2d);
      }
      break;
    }
    case PT_EQ_AFFINE: {
      const bool r = ext_eq_affine(ld_ext(p), ld(p + EXT), ld(p + EXT + F));
      if (s.live) o[0] = r ? 1u : 0u;
      break;
    }
    default: break;
  }
}

// four lanes per item (eight for the octet combine), the record replicated in every lane; every lane
// writes its own copy of the result (the octet combine: the lanes of quad 0)
__global__ void __launch_bounds__(kBlock) k_probe_quad(int op, const u32* __restrict__ in, int iw, u32* __restrict__ out,
                                                       int ow, size_t n) {
  const int lanes = op == Q_OCTET ? 8 : 4;
  const Slot s = slot(n, lanes);
  const int q = threadIdx.x & 3;
  const bool upper = (threadIdx.x & 4) != 0;
  const u32* p = in + s.i * iw;
  QExt acc = ld_q(p + ((op == Q_OCTET && upper) ? QX : 0));
  switch (op) {
    case Q_DOUBLE_T: qext_double<true>(acc, q); break;
    case Q_DOUBLE: qext_double<false>(acc, q); break;
    case Q_ADD_NIELS: qext_add_niels(acc, q, ld_niels(p + QX)); break;
    case Q_ADD_ANIELS: qext_add_aniels(acc, q, ld_aniels(p + QX)); break;
    case Q_MUL16: {
#pragma unroll 1
      for (int j = 0; j < 3; j++) qext_double<false>(acc, q);
      qext_double<true>(acc, q);
      break;
    }
    case Q_OCTET: qext_add_niels(acc, q, qext_upper_niels(acc)); break;
    default: break;
  }
  if (s.live && !(op == Q_OCTET && upper)) st_q(out + s.i * ow + q * QX, acc);
}

// one lane per item, whole waves: the linear layers run on the matrix cores
__global__ void __launch_bounds__(kBlock) k_probe_hades(int op, const u32* __restrict__ in, int iw, u32* __restrict__ out,
                                                        int ow, size_t n) {
  hades_mfma_load_table();
  const Slot sl = slot(n, 1);
  const u32* p = in + sl.i * iw;
  u32* o = out + sl.i * ow;
  Fe s[5];
#pragma unroll
  for (int k = 0; k < 5; k++) s[k] = ld(p + (iw >= 5 * F ? k * F : 0));
  u32 w[8];
  switch (op) {
    case H_SBOX: s[0] = hades_sbox(s[0]); break;
    case H_MDS5: hades_mds_mfma(s, 0, 5); break;
    case H_MDS_ROW1: hades_mds_mfma(s, 1, 1); break;
    case H_MDS_MASK01: hades_mds_mfma(s, 0, 5, 0x01u); break;
    case H_MDS_MASK11: hades_mds_mfma(s, 0, 5, 0x11u); break;
    case H_FULL:
    case H_FULL_W1: {
      const u32 r = p[5 * F] % (DSV_HADES_FULL + DSV_HADES_PARTIAL);
      hades_full_round(s, c_hades_rc + 5 * r, op == H_FULL_W1);
      break;
    }
    case H_FIRST0: hades_first_round_const<false>(s, c_hades_rc); break;
    case H_FIRST1: hades_first_round_const<true>(s, c_hades_rc); break;
    case H_PARTIAL: hades_partial_rounds(s); break;
    case H_PERMUTE: hades_permute<0>(s, false); break;
    case H_TRUNCATE: poseidon_truncate(w, s[0]); break;
    default: break;
  }
  if (!sl.live) return;
  if (op == H_TRUNCATE) {
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = w[k];
  } else if (op == H_SBOX) {
    st(o, s[0]);
  } else if (op == H_MDS_ROW1) {
    st(o, s[4]);
  } else if (op == H_FULL_W1) {
    st(o, s[1]);
  } else {
#pragma unroll
    for (int k = 0; k < 5; k++) st(o + k * F, s[k]);
  }
}

__global__ void __launch_bounds__(kBlock) k_probe_inv(int op, const u32* __restrict__ in, int iw, u32* __restrict__ out,
                                                      int ow, size_t n) {
  const Slot s = slot(n, 1);
  const Fe a = ld(in + s.i * iw);
  const Fe r = op == I_EUCLID ? fe_invert_euclid(a) : fe_invert(a);
  if (s.live) st(out + s.i * ow, r);
}

hipError_t upload_constants() {
  static bool done = false;
  if (done) return hipSuccess;
  hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_hades_rc), DSV_HADES_RC_HOST, sizeof(DSV_HADES_RC_HOST));
  if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(c_hades_k0), DSV_HADES_K0_HOST, sizeof(DSV_HADES_K0_HOST));
  done = e == hipSuccess;
  return e;
}

}  // namespace probe
}  // namespace dsv

using dsv::probe::kOps;
using dsv::probe::kNumOps;

// number of ops; for 0 <= idx < count, the op's name, words per item in and out and items per wave
extern "C" int dsv_probe_ops(int idx, const char** name, int* in_words, int* out_words, int* items_per_wave) {
  if (idx >= 0 && idx < kNumOps) {
    if (name) *name = kOps[idx].name;
    if (in_words) *in_words = kOps[idx].in_words;
    if (out_words) *out_words = kOps[idx].out_words;
    if (items_per_wave) *items_per_wave = 64 / kOps[idx].lanes;
  }
  return kNumOps;
}

// runs op on n items of host memory `in` (n * in_words words) into `out` (n * out_words words):
// 0 on success, -1 for an unknown op, -(1000 + hipError_t) on a HIP error
extern "C" int dsv_probe_run(int op, const uint32_t* in, size_t n, uint32_t* out) {
  using namespace dsv::probe;
  if (op < 0 || op >= kNumOps) return -1;
  if (n == 0) return 0;
  const Op& d = kOps[op];
  const size_t in_bytes = n * d.in_words * sizeof(uint32_t), out_bytes = n * d.out_words * sizeof(uint32_t);
  const size_t threads = n * d.lanes;
  const size_t grid = (threads + kBlock - 1) / kBlock;  // whole blocks of whole waves, all lanes run
  uint32_t *din = nullptr, *dout = nullptr;
  hipError_t e = hipSuccess;
#define DSV_PROBE_TRY(x) \
  if (e == hipSuccess) e = (x)
  if (d.fam == kHades) DSV_PROBE_TRY(upload_constants());
  // (16 zero words of slack: the fe kernel loads whole field elements also from 8-word records)
  DSV_PROBE_TRY(hipMalloc(&din, in_bytes + 16 * sizeof(uint32_t)));
  DSV_PROBE_TRY(hipMalloc(&dout, out_bytes));
  DSV_PROBE_TRY(hipMemset(din, 0, in_bytes + 16 * sizeof(uint32_t)));
  DSV_PROBE_TRY(hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice));
  DSV_PROBE_TRY(hipMemset(dout, 0, out_bytes));
  if (e == hipSuccess) {
    const dim3 g((unsigned)grid), b(kBlock);
    switch (d.fam) {
      case kFe: hipLaunchKernelGGL(k_probe_fe, g, b, 0, 0, d.sub, din, d.in_words, dout, d.out_words, n); break;
      case kPt: hipLaunchKernelGGL(k_probe_pt, g, b, 0, 0, d.sub, din, d.in_words, dout, d.out_words, n); break;
      case kQuad: hipLaunchKernelGGL(k_probe_quad, g, b, 0, 0, d.sub, din, d.in_words, dout, d.out_words, n); break;
      case kHades: hipLaunchKernelGGL(k_probe_hades, g, b, 0, 0, d.sub, din, d.in_words, dout, d.out_words, n); break;
      case kInv: hipLaunchKernelGGL(k_probe_inv, g, b, 0, 0, d.sub, din, d.in_words, dout, d.out_words, n); break;
    }
    e = hipGetLastError();
  }
  DSV_PROBE_TRY(hipDeviceSynchronize());
  DSV_PROBE_TRY(hipMemcpy(out, dout, out_bytes, hipMemcpyDeviceToHost));
#undef DSV_PROBE_TRY
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return e == hipSuccess ? 0 : -(1000 + (int)e);
}
