// api_poly.hip -- batch inversion and four-point interpolation (multi_inv.hip, inv_items.cuh); polynomial products, division, zpoly,
// lagrange_interp and evaluation (poly_arith.hip, poly_eval.hip, poly_items.cuh) on the host side.
#include "ctx.hpp"
using namespace shk;

namespace {
constexpr uint64_t IV_MAX_ITEMS = 1ull << 52;  // keeps every byte count of a call far from 2^64

int multi_inv_run(sh_ctx* c, const fp* in, fp* out, uint64_t n) {
  void* s = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_INV, (size_t)shk_multi_inv_scratch(n) * sizeof(fp), &s));
  HIP_TRY(c, shk_multi_inv(in, out, n, static_cast<fp*>(s), c->stream));
  return SH_OK;
}
int multi_interp_4_run(sh_ctx* c, const fp* xs, const fp* ys, fp* coeffs, uint64_t rows) {
  void* s = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_INV, (size_t)shk_multi_interp_4_scratch(rows) * sizeof(fp), &s));
  HIP_TRY(c, shk_multi_interp_4(xs, ys, coeffs, rows, static_cast<fp*>(s), c->stream));
  return SH_OK;
}

// ---- polynomial products, division, zpoly, lagrange_interp (poly_arith.hip, poly_items.cuh) ------------------------------------------
constexpr uint64_t PA_MAX_PRODUCT = 1ull << 25;   // result coefficients of sh_poly_mul
constexpr uint64_t PA_MAX_DIVIDEND = 1ull << 24;  // dividend coefficients of sh_poly_divmod
constexpr uint64_t PA_MAX_POINTS = 1ull << 20;    // points of sh_zpoly / sh_lagrange_interp

// the back end of poly_items.cuh's drivers on the device: batched NTT plans over 7^((p - 1) / n) from the plan cache (shared with every
// other entry point), the poly_arith.hip kernels, scratch from the context's workspaces, all on the ctx stream
struct DevOps {
  sh_ctx* c;
  int ntt(const fp* src, fp* dst, uint64_t batch, uint64_t n, uint64_t n_in, bool inverse) {
    const fp w = h_root_of_order_pow2(ilog2(n));
    NttPlan* pl = nullptr;
    SH_TRY(get_plan(c, inverse ? h_pow(w, n - 1) : w, n, inverse, &pl));
    return run_ntt(c, pl, src, dst, (uint32_t)batch, n_in);
  }
  int copy(const PaCopy& k, const fp* src, fp* dst) { HIP_TRY(c, shk_pa_copy(k, src, dst, c->stream)); return SH_OK; }
  int pointwise(const fp* a, const fp* b, fp* out, uint64_t n) { HIP_TRY(c, shk_pointwise_mul(a, b, out, n, c->stream)); return SH_OK; }
  int tree(const fp* hz, fp* oz, const fp* hn, fp* on, uint32_t log2d, uint64_t nodes) {
    HIP_TRY(c, shk_pa_tree(hz, oz, hn, on, log2d, nodes, c->stream));
    return SH_OK;
  }
  int mid(const fp* hd, fp* hr, uint32_t log2d, uint64_t children) { HIP_TRY(c, shk_pa_mid(hd, hr, log2d, children, c->stream)); return SH_OK; }
  int newton(const fp* F, fp* G, uint64_t n) { HIP_TRY(c, shk_pa_newton(F, G, n, c->stream)); return SH_OK; }
  int inv1(const fp* src, fp* dst) { HIP_TRY(c, shk_pa_inv1(src, dst, c->stream)); return SH_OK; }
  int deriv_rev(const fp* top, fp* out, uint64_t N, uint64_t n) { HIP_TRY(c, shk_pa_deriv_rev(top, out, N, n, c->stream)); return SH_OK; }
  int multi_inv(const fp* in, fp* out, uint64_t n) { return multi_inv_run(c, in, out, n); }
  int weights(const fp* ys, const fp* inv, fp* out, uint64_t n, uint64_t N) {
    HIP_TRY(c, shk_pa_weights(ys, inv, out, n, N, c->stream));
    return SH_OK;
  }
  int sub(const fp* a, const fp* b, fp* out, uint64_t n) { HIP_TRY(c, shk_pa_sub(a, b, out, n, c->stream)); return SH_OK; }
  int eval_pow_table(const fp* xs, uint64_t m, uint32_t lgS, fp* tbl) { HIP_TRY(c, shk_pe_pow_table(xs, m, lgS, tbl, c->stream)); return SH_OK; }
  int eval_direct(const PeDirect& s, const fp* coefs, const fp* tbl, fp* dst) { HIP_TRY(c, shk_pe_direct(s, coefs, tbl, dst, c->stream)); return SH_OK; }
  int eval_sum(const PeDirect& s, const fp* part, fp* out) { HIP_TRY(c, shk_pe_sum(s, part, out, c->stream)); return SH_OK; }
  int eval_chunks(const fp* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, fp* dst) {
    HIP_TRY(c, shk_pe_chunks(coefs, n, batch, N, C, dst, c->stream));
    return SH_OK;
  }
  int bcast_mul(fp* a, const fp* b, uint64_t rows, uint64_t len) { HIP_TRY(c, shk_pe_bcast_mul(a, b, rows, len, c->stream)); return SH_OK; }
  int eval_combine(const fp* leaves, const fp* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, fp* out) {
    HIP_TRY(c, shk_pe_combine(leaves, xs, m, N, C, batch, out, c->stream));
    return SH_OK;
  }
  int buf(int slot, uint64_t elems, fp** out) { return ws(sh_ctx::WS_PA_TREE + slot, elems, out); }
  int ws(int slot, uint64_t elems, fp** out) {
    void* p = nullptr;
    SH_TRY(ws_get(c, slot, (size_t)elems * sizeof(fp), &p));
    *out = static_cast<fp*>(p);
    return SH_OK;
  }
};

// the leading coefficient of a device divisor, read before anything is launched
int pa_lc_nonzero(sh_ctx* c, const void* d_b, uint64_t nb, bool* nonzero) {
  fp lc;
  HIP_TRY(c, hipMemcpyAsync(&lc, static_cast<const fp*>(d_b) + (nb - 1), sizeof(fp), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *nonzero = !fp_eq_canon(fp_canon(lc), fp_zero());
  return SH_OK;
}

// sh_poly_eval's limits and checks (include/starkhip.h), then the path: STARKHIP_EVAL_PATH, else poly_items.cuh's cost rule
constexpr uint64_t PE_MAX_COEFS = 1ull << 25, PE_MAX_TOTAL = 1ull << 26, PE_MAX_POINTS = 1ull << 20;
int pe_check(sh_ctx* c, const void* coefs, uint64_t n, uint32_t batch, const void* xs, uint64_t m, const void* out) {
  if (!c || batch == 0 || (n && !coefs) || (m && (!xs || !out))) return SH_ERR_INVALID;
  if (n > PE_MAX_COEFS || (uint64_t)batch * n > PE_MAX_TOTAL || m > PE_MAX_POINTS) return SH_ERR_UNSUPPORTED;
  const uint64_t out_bytes = 32ull * batch * m;
  if (any_overlap(out, out_bytes, coefs, 32ull * batch * n) || any_overlap(out, out_bytes, xs, 32 * m)) return SH_ERR_INVALID;
  return SH_OK;
}
bool pe_direct(uint64_t n, uint64_t m, uint32_t batch) {
  const int forced = shk_knobs().eval_path;
  return forced ? forced == 1 : pe_direct_preferred(n, m, batch);
}
}  // namespace

extern "C" {

int sh_dev_multi_inv(sh_ctx* c, const void* d_in, void* d_out, uint64_t n) {
  if (!c || !d_in || !d_out || n > IV_MAX_ITEMS || partial_overlap(d_in, 32 * n, d_out, 32 * n)) return SH_ERR_INVALID;
  if (n == 0) return SH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return multi_inv_run(c, static_cast<const fp*>(d_in), static_cast<fp*>(d_out), n);
}

int sh_multi_inv(sh_ctx* c, const uint8_t* in, uint64_t n, uint8_t* out) {
  if (!c || !in || !out || n > IV_MAX_ITEMS) return SH_ERR_INVALID;
  if (n == 0) return SH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  fp* x = nullptr;
  SH_TRY(upload_padded(c, in, n, n, 1, sh_ctx::WS_X, &x));
  SH_TRY(multi_inv_run(c, x, x, n));
  return download_wire(c, x, out, n);
}

int sh_dev_multi_interp_4(sh_ctx* c, const void* d_xs, const void* d_ys, uint64_t rows, void* d_coeffs) {
  if (!c || !d_xs || !d_ys || !d_coeffs || rows > IV_MAX_ITEMS) return SH_ERR_INVALID;
  const uint64_t bytes = 128 * rows;
  if (partial_overlap(d_xs, bytes, d_coeffs, bytes) || partial_overlap(d_ys, bytes, d_coeffs, bytes)) return SH_ERR_INVALID;
  if (rows == 0) return SH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return multi_interp_4_run(c, static_cast<const fp*>(d_xs), static_cast<const fp*>(d_ys), static_cast<fp*>(d_coeffs), rows);
}

int sh_multi_interp_4(sh_ctx* c, const uint8_t* xs, const uint8_t* ys, uint64_t rows, uint8_t* coeffs) {
  if (!c || !xs || !ys || !coeffs || rows > IV_MAX_ITEMS) return SH_ERR_INVALID;
  if (rows == 0) return SH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  fp *x = nullptr, *y = nullptr;
  SH_TRY(upload_padded(c, xs, 4 * rows, 4 * rows, 1, sh_ctx::WS_X, &x));
  SH_TRY(upload_padded(c, ys, 4 * rows, 4 * rows, 1, sh_ctx::WS_Y, &y));
  SH_TRY(multi_interp_4_run(c, x, y, x, rows));
  return download_wire(c, x, coeffs, 4 * rows);
}

int sh_dev_poly_mul(sh_ctx* c, const void* d_a, uint64_t n_a, const void* d_b, uint64_t n_b, void* d_out) {
  if (!c || n_a > PA_MAX_PRODUCT || n_b > PA_MAX_PRODUCT) return SH_ERR_INVALID;
  if (n_a == 0 || n_b == 0) return SH_OK;
  const uint64_t nc = n_a + n_b - 1;
  if (nc > PA_MAX_PRODUCT || !d_a || !d_b || !d_out || any_overlap(d_out, 32 * nc, d_a, 32 * n_a) ||
      any_overlap(d_out, 32 * nc, d_b, 32 * n_b))
    return SH_ERR_INVALID;
  SH_TRY(enter(c));
  DevOps o{c};
  fp *t1, *t2;
  SH_TRY(o.buf(PA_BUF_1, pa_pow2_at_least(nc), &t1));
  SH_TRY(o.buf(PA_BUF_2, pa_pow2_at_least(nc), &t2));
  return pa_mul(o, static_cast<const fp*>(d_a), n_a, static_cast<const fp*>(d_b), n_b, static_cast<fp*>(d_out), t1, t2);
}

int sh_poly_mul(sh_ctx* c, const uint8_t* a, uint64_t n_a, const uint8_t* b, uint64_t n_b, uint8_t* out) {
  if (!c || n_a > PA_MAX_PRODUCT || n_b > PA_MAX_PRODUCT) return SH_ERR_INVALID;
  if (n_a == 0 || n_b == 0) return SH_OK;
  const uint64_t nc = n_a + n_b - 1;
  if (nc > PA_MAX_PRODUCT || !a || !b || !out) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  DevOps o{c};
  fp *x, *y, *d_out, *t1, *t2;
  SH_TRY(upload_padded(c, a, n_a, n_a, 1, sh_ctx::WS_X, &x));
  SH_TRY(upload_padded(c, b, n_b, n_b, 1, sh_ctx::WS_Y, &y));
  SH_TRY(o.buf(PA_BUF_4, nc, &d_out));
  SH_TRY(o.buf(PA_BUF_1, pa_pow2_at_least(nc), &t1));
  SH_TRY(o.buf(PA_BUF_2, pa_pow2_at_least(nc), &t2));
  SH_TRY(pa_mul(o, x, n_a, y, n_b, d_out, t1, t2));
  return download_wire(c, d_out, out, nc);
}

int sh_dev_poly_divmod(sh_ctx* c, const void* d_a, uint64_t n_a, const void* d_b, uint64_t n_b, void* d_q, void* d_r) {
  if (!c || n_b == 0 || n_a > PA_MAX_DIVIDEND || n_b > PA_MAX_DIVIDEND || !d_b) return SH_ERR_INVALID;
  const uint64_t nq = n_a >= n_b ? n_a - n_b + 1 : 0, nr = n_a < n_b - 1 ? n_a : n_b - 1;
  if ((n_a && !d_a) || (nq && !d_q) || (nr && !d_r)) return SH_ERR_INVALID;
  const void* in[2] = {d_a, d_b};
  const uint64_t in_n[2] = {n_a, n_b};
  for (int k = 0; k < 2; ++k)
    if (any_overlap(d_q, 32 * nq, in[k], 32 * in_n[k]) || any_overlap(d_r, 32 * nr, in[k], 32 * in_n[k])) return SH_ERR_INVALID;
  if (any_overlap(d_q, 32 * nq, d_r, 32 * nr)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  bool ok = false;
  SH_TRY(pa_lc_nonzero(c, d_b, n_b, &ok));
  if (!ok) return SH_ERR_INVALID;
  if (n_a == 0) return SH_OK;
  DevOps o{c};
  return pa_divmod(o, static_cast<const fp*>(d_a), n_a, static_cast<const fp*>(d_b), n_b, static_cast<fp*>(d_q), static_cast<fp*>(d_r));
}

int sh_poly_divmod(sh_ctx* c, const uint8_t* a, uint64_t n_a, const uint8_t* b, uint64_t n_b, uint8_t* q, uint8_t* r) {
  if (!c || n_b == 0 || n_a > PA_MAX_DIVIDEND || n_b > PA_MAX_DIVIDEND || !b) return SH_ERR_INVALID;
  const uint64_t nq = n_a >= n_b ? n_a - n_b + 1 : 0, nr = n_a < n_b - 1 ? n_a : n_b - 1;
  if ((n_a && !a) || (nq && !q) || (nr && !r)) return SH_ERR_INVALID;
  if (fp_eq_canon(h_from_wire(b + 32 * (n_b - 1)), fp_zero())) return SH_ERR_INVALID;
  if (n_a == 0) return SH_OK;
  SH_TRY(enter(c));
  DevOps o{c};
  fp *x, *y, *oq, *orr;
  SH_TRY(upload_padded(c, a, n_a, n_a, 1, sh_ctx::WS_X, &x));
  SH_TRY(upload_padded(c, b, n_b, n_b, 1, sh_ctx::WS_Y, &y));
  SH_TRY(o.ws(sh_ctx::WS_MISC, nq + nr, &oq));
  orr = oq + nq;
  SH_TRY(pa_divmod(o, x, n_a, y, n_b, oq, orr));
  if (nq) SH_TRY(download_wire(c, oq, q, nq));
  if (nr) SH_TRY(download_wire(c, orr, r, nr));
  return SH_OK;
}

int sh_dev_zpoly(sh_ctx* c, const void* d_xs, uint64_t n, void* d_out) {
  if (!c || n > PA_MAX_POINTS || !d_out || (n && !d_xs) || any_overlap(d_out, 32 * (n + 1), d_xs, 32 * n)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  DevOps o{c};
  return pa_zpoly(o, static_cast<const fp*>(d_xs), n, static_cast<fp*>(d_out));
}

int sh_zpoly(sh_ctx* c, const uint8_t* xs, uint64_t n, uint8_t* out) {
  if (!c || n > PA_MAX_POINTS || !out || (n && !xs)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  DevOps o{c};
  fp *x = nullptr, *d_out;
  if (n) SH_TRY(upload_padded(c, xs, n, n, 1, sh_ctx::WS_X, &x));
  SH_TRY(o.ws(sh_ctx::WS_MISC, n + 1, &d_out));
  SH_TRY(pa_zpoly(o, x, n, d_out));
  return download_wire(c, d_out, out, n + 1);
}

int sh_dev_lagrange_interp(sh_ctx* c, const void* d_xs, const void* d_ys, uint64_t n, void* d_out) {
  if (!c || n > PA_MAX_POINTS) return SH_ERR_INVALID;
  if (n == 0) return SH_OK;
  if (!d_xs || !d_ys || !d_out || any_overlap(d_out, 32 * n, d_xs, 32 * n) || any_overlap(d_out, 32 * n, d_ys, 32 * n))
    return SH_ERR_INVALID;
  SH_TRY(enter(c));
  DevOps o{c};
  return pa_lagrange(o, static_cast<const fp*>(d_xs), static_cast<const fp*>(d_ys), n, static_cast<fp*>(d_out));
}

int sh_lagrange_interp(sh_ctx* c, const uint8_t* xs, const uint8_t* ys, uint64_t n, uint8_t* out) {
  if (!c || n > PA_MAX_POINTS) return SH_ERR_INVALID;
  if (n == 0) return SH_OK;
  if (!xs || !ys || !out) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  DevOps o{c};
  fp *x, *y, *d_out;
  SH_TRY(upload_padded(c, xs, n, n, 1, sh_ctx::WS_X, &x));
  SH_TRY(upload_padded(c, ys, n, n, 1, sh_ctx::WS_Y, &y));
  SH_TRY(o.ws(sh_ctx::WS_MISC, n, &d_out));
  SH_TRY(pa_lagrange(o, x, y, n, d_out));
  return download_wire(c, d_out, out, n);
}

int sh_dev_poly_eval(sh_ctx* c, const void* d_coefs, uint64_t n, uint32_t batch, const void* d_xs, uint64_t m, void* d_out) {
  SH_TRY(pe_check(c, d_coefs, n, batch, d_xs, m, d_out));
  if (m == 0) return SH_OK;
  SH_TRY(enter(c));
  DevOps o{c};
  return pa_eval(o, static_cast<const fp*>(d_coefs), n, batch, static_cast<const fp*>(d_xs), m, static_cast<fp*>(d_out),
                 pe_direct(n, m, batch));
}

int sh_poly_eval(sh_ctx* c, const uint8_t* coefs, uint64_t n, uint32_t batch, const uint8_t* xs, uint64_t m, uint8_t* out) {
  SH_TRY(pe_check(c, coefs, n, batch, xs, m, out));
  if (m == 0) return SH_OK;
  SH_TRY(enter(c));
  DevOps o{c};
  fp *x = nullptr, *d_xs, *d_out;
  if (n) SH_TRY(upload_padded(c, coefs, n, n, batch, sh_ctx::WS_X, &x));
  SH_TRY(upload_padded(c, xs, m, m, 1, sh_ctx::WS_Y, &d_xs));
  SH_TRY(o.ws(sh_ctx::WS_MISC, (uint64_t)batch * m, &d_out));
  SH_TRY(pa_eval(o, x, n, batch, d_xs, m, d_out, pe_direct(n, m, batch)));
  return download_wire(c, d_out, out, (uint64_t)batch * m);
}
}  // extern "C"
