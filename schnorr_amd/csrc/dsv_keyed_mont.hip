// dsv_keyed_mont.hip — the keyed typed-object form (include/dsv.h: dsv_keyset_create_mont_cols,
// dsv_verify_keyed_mont_*; keyed_mont.h): keys registered from `PublicKey*` objects where they lie, `Signature*`
// objects verified where they lie by key index.  Device form: normalise the nonce points and the two scalars,
// challenge hash, keyed kernel — three launches on the caller's stream.  Host form: the normalisation once per
// chunk of the shared host pipeline (dsv_pipeline.h), hash and keyed kernel per sub-batch, under the key-set
// registry's shared lock for the whole call.  Submit: dsv_host.hip's job driver around the host form.
#include "dsv_pipeline.h"
#include "keyed_mont.h"

namespace dsvh {

KeyedCols carve_keyed_mont(Stager& x, int scheme, size_t n) {
  const int np = keyed_sig_points(scheme);
  KeyedCols w;
  w.u = x.take(n * 32);
  w.m = x.take(n * 32);
  w.R = x.take(n * 64);
  w.Rp = np == 2 ? x.take(n * 64) : nullptr;
  w.valid = x.take(n);
  w.prefix = reinterpret_cast<u32*>(x.take(normalize_prefix_bytes(n, np)));
  return w;
}

void normalize_keyed_mont(int scheme, const uint8_t* u, const uint8_t* R, const uint8_t* Rp, const uint8_t* m,
                          size_t n, const KeyedCols& w, hipStream_t stream, int per_lane, int block) {
  const int np = keyed_sig_points(scheme);
  NormalizeArgs a = {};
  a.in[0] = R;
  a.out[0] = w.R;
  if (np == 2) {
    a.in[1] = Rp;
    a.out[1] = w.Rp;
  }
  a.u_mont = u;
  a.m_mont = m;
  a.u_out = w.u;
  a.m_out = w.m;
  launch_normalize_uvz(a, np, n, w.valid, w.prefix, stream, per_lane, block);
}

int check_keyed_mont_cols(const dsv_keyset* ks, const dsv_column* cols, size_t n, const uint8_t* ok) {
  if (int r = check_n(n)) return r;
  if (!ks) return fail(DSV_ERR_INVALID_ARGUMENT, "null key set");
  if (n == 0) return DSV_OK;
  if (!cols || !ok) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
  const int nc = keyed_mont_columns(ks->scheme);
  for (int c = 0; c < nc; c++) {
    const size_t width = keyed_mont_width(ks->scheme, c);
    if (!cols[c].base) return fail(DSV_ERR_INVALID_ARGUMENT, "column %d: null pointer", c);
    if (cols[c].stride < width)
      return fail(DSV_ERR_INVALID_ARGUMENT, "column %d: stride %zu < %zu", c, cols[c].stride, width);
    if (width == 4 && (((uintptr_t)cols[c].base | cols[c].stride) & 3))
      return fail(DSV_ERR_INVALID_ARGUMENT, "column %d: key indices must be 4-byte aligned", c);
  }
  return DSV_OK;
}

namespace {

size_t keyed_mont_ws_bytes(int scheme, size_t n) { return keyed_mont_cols_bytes(scheme, n) + keyed_ws_bytes(n); }

}  // namespace

// host objects: per chunk ONE normalisation launch (the preprocessing of the unkeyed *_mont_cols path, over
// the nonce points alone), per sub-batch the challenge hash and the keyed kernel with the normalisation's
// validity bytes as valid_in; the keyed workspace (c, valid) is the lane's verify workspace, never smaller
int verify_keyed_mont_cols_locked(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok) {
  if (int r = check_keyed_mont_cols(ks, cols, n, ok)) return r;
  const int scheme = ks->scheme;
  Context* cp = nullptr;
  if (int r = check_set(ks, scheme, n, cp)) return r;
  if (n == 0) return DSV_OK;
  const int np = keyed_sig_points(scheme), nc = keyed_mont_columns(scheme);
  HostIn ins[kMaxHostIn];
  for (int c = 0; c < nc; c++)
    ins[c] = HostIn{static_cast<const uint8_t*>(cols[c].base), keyed_mont_width(scheme, c), cols[c].stride};
  // scratch of the chunk's normalisation per item: u, m, the affine points, valid, the prefix products
  const size_t prep_item_bytes = 64 + (size_t)np * 64 + 1 + (size_t)np * kLimbs * 4;
  return run_pipelined(
      *cp, ins, (size_t)nc, ok, n, prep_item_bytes, 0,
      [=](const void* const* d, size_t c, Stager& x, hipStream_t st, Staged& g) {
        const KeyedCols w = carve_keyed_mont(x, scheme, c);
        normalize_keyed_mont(scheme, (const uint8_t*)d[0], (const uint8_t*)d[1],
                             np == 2 ? (const uint8_t*)d[2] : nullptr, (const uint8_t*)d[np + 2], c, w, st,
                             cp->norm_per_lane, cp->norm_block);  // ONE launch
        HIP_TRY(hipGetLastError());
        // staged as u, R, R' (null unless double), key_idx (as transferred), m
        g.p[0] = w.u, g.p[1] = w.R, g.p[2] = w.Rp, g.p[3] = (const uint8_t*)d[np + 1], g.p[4] = w.m;
        g.bytes[0] = g.bytes[4] = 32, g.bytes[1] = g.bytes[2] = 64, g.bytes[3] = 4;
        g.valid = w.valid;
        return (int)DSV_OK;
      },
      [=](const Staged& g, size_t off, size_t cnt, void* dok, void* ws, Stager&, hipStream_t st) {
        const Items in = make_items(scheme, g.p[0] + off * 32, {g.p[1] + off * 64, g.p[2] ? g.p[2] + off * 64 : nullptr},
                                    g.p[4] + off * 32);
        enqueue_keyed(*cp, ks, in, reinterpret_cast<const uint32_t*>(g.p[3] + off * 4), cnt,
                      static_cast<uint8_t*>(dok), ws, st, g.valid + off);
        HIP_TRY(hipGetLastError());
        return (int)DSV_OK;
      });
}

// the typed-object key form: m `PublicKey*` objects gathered out of their columns, normalised in front of the
// table build
KeysetForm keyset_form_mont_cols(int scheme, const dsv_column* cols, size_t m) {
  const int np = keyset_points(scheme);
  // behind the points: the objects' limbs (np x m x 96 B), the normalisation's verdicts and its prefix products
  const size_t off_valid = align_up((size_t)np * m * 96, 256), off_prefix = off_valid + align_up(m, 256);
  return {[=] {
            if (!cols) return fail(DSV_ERR_INVALID_ARGUMENT, "null pointer");
            for (int p = 0; p < np; p++) {
              if (!cols[p].base) return fail(DSV_ERR_INVALID_ARGUMENT, "column %d: null pointer", p);
              if (cols[p].stride < 96)
                return fail(DSV_ERR_INVALID_ARGUMENT, "column %d: stride %zu < 96", p, cols[p].stride);
            }
            return (int)DSV_OK;
          },
          off_prefix + align_up(normalize_prefix_bytes(m, np), 256),
          // dense: the key points gathered out of the objects (outlives the transfer: the form lives until the
          // call has synchronised its stream)
          [=, dense = std::vector<uint8_t>()](Context&, uint8_t* P, uint8_t* own, hipStream_t s,
                                              uint8_t*& valid) mutable {
            dense.resize((size_t)np * m * 96);
            NormalizeArgs a = {};
            for (int p = 0; p < np; p++) {
              copy_strided_plain(dense.data() + (size_t)p * m * 96, static_cast<const uint8_t*>(cols[p].base),
                                 cols[p].stride, 96, m);
              a.in[p] = own + (size_t)p * m * 96;
              a.out[p] = P + (size_t)p * m * 64;
            }
            HIP_TRY(hipMemcpyAsync(own, dense.data(), dense.size(), hipMemcpyHostToDevice, s));
            valid = own + off_valid;
            launch_normalize_uvz(a, np, m, valid, reinterpret_cast<u32*>(own + off_prefix), s);
            HIP_TRY(hipGetLastError());
            return (int)DSV_OK;
          }};
}

}  // namespace dsvh

using namespace dsvh;

extern "C" {

int dsv_keyset_create_mont_cols(int scheme, const dsv_column* cols, size_t k, dsv_keyset** out) {
  return create_keyset(scheme, k, k, false, out, keyset_form_mont_cols(scheme, cols, k));
}
int dsv_keyset_append_mont_cols(dsv_keyset* ks, const dsv_column* cols, size_t m, uint32_t* first_index) {
  return append_keyset(ks, m, first_index, [=](int scheme) { return keyset_form_mont_cols(scheme, cols, m); });
}

size_t dsv_keyed_mont_workspace_bytes(int scheme, size_t n) {
  return scheme_ok(scheme) ? keyed_mont_ws_bytes(scheme, n) : 0;
}

int dsv_verify_keyed_mont_dev(const dsv_keyset* ks, const void* u, const void* R_uvz, const void* Rp_uvz,
                              const void* key_idx, const void* m, size_t n, void* ok, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return run_keyed_dev(
      ks, -1, [=](int scheme) { return !u || !R_uvz || (keyed_sig_points(scheme) == 2 && !Rp_uvz) || !m; },
      [=](int scheme) { return keyed_mont_cols_bytes(scheme, n); }, key_idx, n, ok, workspace, workspace_bytes, stream,
      [=](const Context&, int scheme, Stager& x, hipStream_t s, Items& in, const uint8_t*& valid_in) {
        const KeyedCols w = carve_keyed_mont(x, scheme, n);
        normalize_keyed_mont(scheme, (const uint8_t*)u, (const uint8_t*)R_uvz, (const uint8_t*)Rp_uvz,
                             (const uint8_t*)m, n, w, s);
        in = w.items(scheme);
        valid_in = w.valid;
        return (int)DSV_OK;
      });
}

int dsv_verify_keyed_mont_cols(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok) {
  std::shared_lock<std::shared_mutex> rl(keyset_mutex());
  return verify_keyed_mont_cols_locked(ks, cols, n, ok);
}

int dsv_verify_keyed_mont_cols_submit(const dsv_keyset* ks, const dsv_column* cols, size_t n, uint8_t* ok,
                                      dsv_job** job) {
  if (!job) return fail(DSV_ERR_INVALID_ARGUMENT, "null job pointer");
  *job = nullptr;
  int ncols = 0;
  {
    std::shared_lock<std::shared_mutex> rl(keyset_mutex());
    if (int r = check_keyed_mont_cols(ks, cols, n, ok)) return r;
    ncols = keyed_mont_columns(ks->scheme);
  }
  return submit_cols_job(ks, 0, cols, n ? ncols : 0, n, ok, job);
}

}  // extern "C"
