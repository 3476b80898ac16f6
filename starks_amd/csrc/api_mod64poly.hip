// api_mod64poly.hip -- polynomial products, division, zpoly, lagrange_interp, batch inversion, four-point interpolation and evaluation
// at arbitrary points (sh_mod64_poly_eval) over any prime modulus below 2^64 on packed 64-bit words, on the host side: the drivers of
// poly_items.cuh over the packed-word transform (api_ntt64.hip: mod64_table, mod64_run) and the kernels of mod64poly.hip and
// mod64eval.hip.  Every check runs here before the first launch; every error
// text opens with the entry's name.
#include "ctx.hpp"
#include "mod64eval_items.cuh"
#include "mod64poly_items.cuh"
#include "modpoly_items.cuh"  // mp_max_transform: the one statement of the largest transform
using namespace shk;

namespace {
constexpr uint64_t M6P_MAX_ITEMS = 1ull << 52;    // keeps every byte count of a call far from 2^64
constexpr uint64_t M6P_MAX_PRODUCT = 1ull << 25;  // the sh_mod_* entries' limits (api_modpoly.hip)
constexpr uint64_t M6P_MAX_DIVIDEND = 1ull << 24;
constexpr uint64_t M6P_MAX_POINTS = 1ull << 20;
constexpr int M6P_MAX_ROOT_LOG = N64_MAX_LOG_N;  // 28

int fail(sh_ctx* c, const char* who, const std::string& what, int code) {
  c->err = std::string(who) + ": " + what;
  return code;
}
int check_modulus(sh_ctx* c, const char* who, uint64_t modulus, f64_mod* M) {
  if (!f64_mod_init(modulus, M)) return fail(c, who, "the modulus must be odd and at least 3", SH_ERR_INVALID);
  return SH_OK;
}

// everything a call derives from (modulus, root, root_log) on the host, and the back end of poly_items.cuh's drivers over it
struct Mod64Ops {
  sh_ctx* c;
  f64_mod M;
  uint64_t root_mont;  // the caller's root of order 2^root_log, Montgomery form
  int root_log;
  Mod64Call call[2][M6P_MAX_ROOT_LOG + 1];  // [inverse][log2 n], filled on first use
  bool have[2][M6P_MAX_ROOT_LOG + 1];

  // modulus, root below p, root of order exactly 2^root_log: the one order check of the call
  int init(sh_ctx* ctx, const char* who, uint64_t modulus, uint64_t root, uint32_t rl) {
    c = ctx;
    memset(have, 0, sizeof have);
    SH_TRY(check_modulus(c, who, modulus, &M));
    if (rl > (uint32_t)M6P_MAX_ROOT_LOG) return fail(c, who, "root_log is limited to 28", SH_ERR_UNSUPPORTED);
    if (root >= modulus) return fail(c, who, "root is not below the modulus", SH_ERR_ROOT_ORDER);
    if (!n64_check_root(root, 1ull << rl, M)) return fail(c, who, "root does not have order 2^root_log in this field", SH_ERR_ROOT_ORDER);
    root_log = (int)rl;
    root_mont = f64_to_mont(root, M);
    return SH_OK;
  }
  // the largest transform of the call against the root's order
  int fits(const char* who, uint64_t need) const {
    if (need <= (1ull << root_log)) return SH_OK;
    return fail(c, who,
                "the call needs a transform of size " + std::to_string(need) + " and the root given has order " +
                    std::to_string(1ull << root_log),
                SH_ERR_ROOT_ORDER);
  }
  const Mod64Call& get(int k, bool inverse) {
    Mod64Call& mc = call[inverse][k];
    if (!have[inverse][k]) {
      mc.M = M;
      mc.log_n = k;
      uint64_t w = root_mont;  // root^(2^(root_log - k)): order 2^k
      for (int i = k; i < root_log; ++i) w = f64_mul(w, w, M);
      mc.root_mont = inverse ? f64_pow(w, (1ull << k) - 1, M) : w;
      mc.scale = inverse ? n64_inv_n(k, M) : 1;
      have[inverse][k] = true;
    }
    return mc;
  }

  int ntt(const uint64_t* src, uint64_t* dst, uint64_t batch, uint64_t n, uint64_t n_in, bool inverse) {
    const int k = ilog2(n);
    if (k > root_log) return fail(c, "packed-word polynomial arithmetic", "transform above the root's order", SH_ERR_ROOT_ORDER);
    const Mod64Call& mc = get(k, inverse);
    const uint64_t* tab = nullptr;
    SH_TRY(mod64_table(c, mc, &tab));
    const uint64_t ni = n_in ? n_in : n, per = (1ull << N64_MAX_LOG_N) >> k;  // a level above batch n = 2^28 runs as several calls
    for (uint64_t b0 = 0; b0 < batch; b0 += per) {
      const uint64_t nb = batch - b0 < per ? batch - b0 : per;
      SH_TRY(mod64_run(c, mc, tab, src + b0 * ni, ni, dst + b0 * n, (uint32_t)nb));
    }
    return SH_OK;
  }
  int copy(const PaCopy& k, const uint64_t* src, uint64_t* dst) { HIP_TRY(c, shk_m6p_copy(k, src, dst, M, c->stream)); return SH_OK; }
  int pointwise(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    HIP_TRY(c, shk_n64_pointwise(a, b, out, n, M, c->stream));
    return SH_OK;
  }
  int tree(const uint64_t* hz, uint64_t* oz, const uint64_t* hn, uint64_t* on, uint32_t log2d, uint64_t nodes) {
    HIP_TRY(c, shk_m6p_tree(hz, oz, hn, on, log2d, nodes, M, c->stream));
    return SH_OK;
  }
  int mid(const uint64_t* hd, uint64_t* hr, uint32_t log2d, uint64_t children) {
    HIP_TRY(c, shk_m6p_mid(hd, hr, log2d, children, M, c->stream));
    return SH_OK;
  }
  int newton(const uint64_t* F, uint64_t* G, uint64_t n) { HIP_TRY(c, shk_m6p_newton(F, G, n, M, c->stream)); return SH_OK; }
  int inv1(const uint64_t* src, uint64_t* dst) { HIP_TRY(c, shk_m6p_inv1(src, dst, M, c->stream)); return SH_OK; }
  int deriv_rev(const uint64_t* top, uint64_t* out, uint64_t N, uint64_t n) {
    HIP_TRY(c, shk_m6p_deriv_rev(top, out, N, n, M, c->stream));
    return SH_OK;
  }
  int multi_inv(const uint64_t* in, uint64_t* out, uint64_t n) {
    void* s = nullptr;
    SH_TRY(ws_get(c, sh_ctx::WS_INV, (size_t)shk_m6p_multi_inv_scratch(n) * 8, &s));
    HIP_TRY(c, shk_m6p_multi_inv(in, out, n, static_cast<uint64_t*>(s), M, c->stream));
    return SH_OK;
  }
  int multi_interp_4(const uint64_t* xs, const uint64_t* ys, uint64_t* coeffs, uint64_t rows) {
    void* s = nullptr;
    SH_TRY(ws_get(c, sh_ctx::WS_INV, (size_t)shk_m6p_multi_interp_4_scratch(rows) * 8, &s));
    HIP_TRY(c, shk_m6p_multi_interp_4(xs, ys, coeffs, rows, static_cast<uint64_t*>(s), M, c->stream));
    return SH_OK;
  }
  int weights(const uint64_t* ys, const uint64_t* inv, uint64_t* out, uint64_t n, uint64_t N) {
    HIP_TRY(c, shk_m6p_weights(ys, inv, out, n, N, M, c->stream));
    return SH_OK;
  }
  int sub(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) { HIP_TRY(c, shk_m6p_sub(a, b, out, n, M, c->stream)); return SH_OK; }
  int eval_pow_table(const uint64_t* xs, uint64_t m, uint32_t lgS, uint64_t* tbl) {
    HIP_TRY(c, shk_m6e_pow_table(xs, m, lgS, tbl, M, c->stream));
    return SH_OK;
  }
  int eval_direct(const PeDirect& s, const uint64_t* coefs, const uint64_t* tbl, uint64_t* dst) {
    HIP_TRY(c, shk_m6e_direct(s, coefs, tbl, dst, M, c->stream));
    return SH_OK;
  }
  int eval_sum(const PeDirect& s, const uint64_t* part, uint64_t* out) { HIP_TRY(c, shk_m6e_sum(s, part, out, M, c->stream)); return SH_OK; }
  int eval_chunks(const uint64_t* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, uint64_t* dst) {
    HIP_TRY(c, shk_m6e_chunks(coefs, n, batch, N, C, dst, c->stream));
    return SH_OK;
  }
  int bcast_mul(uint64_t* a, const uint64_t* b, uint64_t rows, uint64_t len) {
    HIP_TRY(c, shk_m6e_bcast_mul(a, b, rows, len, M, c->stream));
    return SH_OK;
  }
  int eval_combine(const uint64_t* leaves, const uint64_t* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, uint64_t* out) {
    HIP_TRY(c, shk_m6e_combine(leaves, xs, m, N, C, batch, out, M, c->stream));
    return SH_OK;
  }
  int buf(int slot, uint64_t elems, uint64_t** out) { return ws(sh_ctx::WS_PA_TREE + slot, elems, out); }
  int ws(int slot, uint64_t elems, uint64_t** out) {
    void* p = nullptr;
    SH_TRY(ws_get(c, slot, (size_t)elems * 8, &p));
    *out = static_cast<uint64_t*>(p);
    return SH_OK;
  }
  // host-buffer forms: native words in and out, plain copies; nothing is reduced
  int upload(const uint64_t* in, uint64_t n, int slot, uint64_t** out) {
    SH_TRY(ws(slot, n, out));
    return h2d(c, *out, in, (size_t)n * 8);
  }
  int download(const uint64_t* d, uint64_t* out, uint64_t n) { return d2h(c, out, d, (size_t)n * 8); }
};

// the divisor's leading word, reduced: zero mod p ?  (a nonzero multiple of p included)
bool lc_is_zero(uint64_t lc, const f64_mod& M) { return f64_canon(lc, M) == 0; }

// the size checks shared by the two forms of an entry
int mul_sizes(sh_ctx* c, const char* who, uint64_t n_a, uint64_t n_b) {
  if (n_a > M6P_MAX_PRODUCT || n_b > M6P_MAX_PRODUCT || (n_a && n_b && n_a + n_b - 1 > M6P_MAX_PRODUCT))
    return fail(c, who, "the product is limited to 2^25 coefficients", SH_ERR_INVALID);
  return SH_OK;
}
int divmod_sizes(sh_ctx* c, const char* who, uint64_t n_a, uint64_t n_b) {
  if (n_b == 0) return fail(c, who, "the divisor is empty", SH_ERR_INVALID);
  if (n_a > M6P_MAX_DIVIDEND || n_b > M6P_MAX_DIVIDEND)
    return fail(c, who, "dividend and divisor are limited to 2^24 coefficients", SH_ERR_INVALID);
  return SH_OK;
}
int point_sizes(sh_ctx* c, const char* who, uint64_t n) {
  if (n > M6P_MAX_POINTS) return fail(c, who, "the points are limited to 2^20", SH_ERR_INVALID);
  return SH_OK;
}
const uint64_t* cw(const void* p) { return static_cast<const uint64_t*>(p); }
uint64_t* w(void* p) { return static_cast<uint64_t*>(p); }

// sh_mod64_poly_eval's limits and checks (sh_mod_poly_eval's: api_modpoly.hip), the modulus and the root, then the path:
// STARKHIP_EVAL_PATH, else the direct path when the tree's transform exceeds the root's order, else mod64eval_items.cuh's cost rule.
// A forced tree that does not fit is refused here, before any launch.
constexpr uint64_t M6E_MAX_COEFS = 1ull << 25, M6E_MAX_TOTAL = 1ull << 26;
int eval_check(sh_ctx* c, const char* who, Mod64Ops* o, uint64_t modulus, uint64_t root, uint32_t root_log, const void* coefs, uint64_t n,
               uint32_t batch, const void* xs, uint64_t m, const void* out, bool* direct) {
  if (batch == 0) return fail(c, who, "batch is zero", SH_ERR_INVALID);
  if ((n && !coefs) || (m && (!xs || !out))) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (n > M6E_MAX_COEFS) return fail(c, who, "a polynomial is limited to 2^25 coefficients", SH_ERR_UNSUPPORTED);
  if ((uint64_t)batch * n > M6E_MAX_TOTAL) return fail(c, who, "the polynomials are limited to 2^26 coefficients in all", SH_ERR_UNSUPPORTED);
  if (m > M6P_MAX_POINTS) return fail(c, who, "the points are limited to 2^20", SH_ERR_UNSUPPORTED);
  const uint64_t out_bytes = 8ull * batch * m;
  if (any_overlap(out, out_bytes, coefs, 8ull * batch * n) || any_overlap(out, out_bytes, xs, 8 * m))
    return fail(c, who, "the output overlaps an input", SH_ERR_INVALID);
  SH_TRY(o->init(c, who, modulus, root, root_log));
  const int forced = shk_knobs().eval_path;
  *direct = forced ? forced == 1 : m6e_direct_preferred(n, m, batch, root_log);
  if (!*direct) SH_TRY(o->fits(who, mp_max_transform(MP_OP_EVAL, n, m)));
  return SH_OK;
}
}  // namespace

extern "C" {

int sh_dev_mod64_multi_inv(sh_ctx* c, uint64_t modulus, const void* d_in, void* d_out, uint64_t n) {
  static const char who[] = "sh_dev_mod64_multi_inv";
  if (!c) return SH_ERR_INVALID;
  if (!d_in || !d_out) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (n > M6P_MAX_ITEMS) return fail(c, who, "too many values", SH_ERR_INVALID);
  if (partial_overlap(d_in, 8 * n, d_out, 8 * n)) return fail(c, who, "the buffers overlap in part", SH_ERR_INVALID);
  Mod64Ops o;
  o.c = c;
  SH_TRY(check_modulus(c, who, modulus, &o.M));
  if (n == 0) return SH_OK;
  SH_TRY(enter(c));
  return o.multi_inv(cw(d_in), w(d_out), n);
}

int sh_mod64_multi_inv(sh_ctx* c, uint64_t modulus, const uint64_t* in, uint64_t n, uint64_t* out) {
  static const char who[] = "sh_mod64_multi_inv";
  if (!c) return SH_ERR_INVALID;
  if (!in || !out) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (n > M6P_MAX_ITEMS) return fail(c, who, "too many values", SH_ERR_INVALID);
  Mod64Ops o;
  o.c = c;
  SH_TRY(check_modulus(c, who, modulus, &o.M));
  if (n == 0) return SH_OK;
  SH_TRY(enter(c));
  uint64_t* x = nullptr;
  SH_TRY(o.upload(in, n, sh_ctx::WS_X, &x));
  SH_TRY(o.multi_inv(x, x, n));
  return o.download(x, out, n);
}

int sh_dev_mod64_multi_interp_4(sh_ctx* c, uint64_t modulus, const void* d_xs, const void* d_ys, uint64_t rows, void* d_coeffs) {
  static const char who[] = "sh_dev_mod64_multi_interp_4";
  if (!c) return SH_ERR_INVALID;
  if (!d_xs || !d_ys || !d_coeffs) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (rows > M6P_MAX_ITEMS) return fail(c, who, "too many rows", SH_ERR_INVALID);
  const uint64_t bytes = 32 * rows;
  if (partial_overlap(d_xs, bytes, d_coeffs, bytes) || partial_overlap(d_ys, bytes, d_coeffs, bytes))
    return fail(c, who, "the buffers overlap in part", SH_ERR_INVALID);
  Mod64Ops o;
  o.c = c;
  SH_TRY(check_modulus(c, who, modulus, &o.M));
  if (rows == 0) return SH_OK;
  SH_TRY(enter(c));
  return o.multi_interp_4(cw(d_xs), cw(d_ys), w(d_coeffs), rows);
}

int sh_mod64_multi_interp_4(sh_ctx* c, uint64_t modulus, const uint64_t* xs, const uint64_t* ys, uint64_t rows, uint64_t* coeffs) {
  static const char who[] = "sh_mod64_multi_interp_4";
  if (!c) return SH_ERR_INVALID;
  if (!xs || !ys || !coeffs) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (rows > M6P_MAX_ITEMS) return fail(c, who, "too many rows", SH_ERR_INVALID);
  Mod64Ops o;
  o.c = c;
  SH_TRY(check_modulus(c, who, modulus, &o.M));
  if (rows == 0) return SH_OK;
  SH_TRY(enter(c));
  uint64_t *x = nullptr, *y = nullptr;
  SH_TRY(o.upload(xs, 4 * rows, sh_ctx::WS_X, &x));
  SH_TRY(o.upload(ys, 4 * rows, sh_ctx::WS_Y, &y));
  SH_TRY(o.multi_interp_4(x, y, x, rows));
  return o.download(x, coeffs, 4 * rows);
}

int sh_dev_mod64_poly_mul(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const void* d_a, uint64_t n_a, const void* d_b,
                          uint64_t n_b, void* d_out) {
  static const char who[] = "sh_dev_mod64_poly_mul";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(mul_sizes(c, who, n_a, n_b));
  const uint64_t nc = n_a && n_b ? n_a + n_b - 1 : 0;
  if (nc && (!d_a || !d_b || !d_out)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (any_overlap(d_out, 8 * nc, d_a, 8 * n_a) || any_overlap(d_out, 8 * nc, d_b, 8 * n_b))
    return fail(c, who, "the output overlaps an input", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_MUL, n_a, n_b)));
  if (nc == 0) return SH_OK;
  SH_TRY(enter(c));
  uint64_t *t1, *t2;
  SH_TRY(o.buf(PA_BUF_1, pa_pow2_at_least(nc), &t1));
  SH_TRY(o.buf(PA_BUF_2, pa_pow2_at_least(nc), &t2));
  return pa_mul(o, cw(d_a), n_a, cw(d_b), n_b, w(d_out), t1, t2);
}

int sh_mod64_poly_mul(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const uint64_t* a, uint64_t n_a, const uint64_t* b,
                      uint64_t n_b, uint64_t* out) {
  static const char who[] = "sh_mod64_poly_mul";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(mul_sizes(c, who, n_a, n_b));
  const uint64_t nc = n_a && n_b ? n_a + n_b - 1 : 0;
  if (nc && (!a || !b || !out)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_MUL, n_a, n_b)));
  if (nc == 0) return SH_OK;
  SH_TRY(enter(c));
  uint64_t *x, *y, *d_out, *t1, *t2;
  SH_TRY(o.upload(a, n_a, sh_ctx::WS_X, &x));
  SH_TRY(o.upload(b, n_b, sh_ctx::WS_Y, &y));
  SH_TRY(o.buf(PA_BUF_4, nc, &d_out));
  SH_TRY(o.buf(PA_BUF_1, pa_pow2_at_least(nc), &t1));
  SH_TRY(o.buf(PA_BUF_2, pa_pow2_at_least(nc), &t2));
  SH_TRY(pa_mul(o, cw(x), n_a, cw(y), n_b, d_out, t1, t2));
  return o.download(d_out, out, nc);
}

int sh_dev_mod64_poly_divmod(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const void* d_a, uint64_t n_a, const void* d_b,
                             uint64_t n_b, void* d_q, void* d_r) {
  static const char who[] = "sh_dev_mod64_poly_divmod";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(divmod_sizes(c, who, n_a, n_b));
  const uint64_t nq = n_a >= n_b ? n_a - n_b + 1 : 0, nr = n_a < n_b - 1 ? n_a : n_b - 1;
  if (!d_b || (n_a && !d_a) || (nq && !d_q) || (nr && !d_r)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  const void* in[2] = {d_a, d_b};
  const uint64_t in_n[2] = {n_a, n_b};
  for (int k = 0; k < 2; ++k)
    if (any_overlap(d_q, 8 * nq, in[k], 8 * in_n[k]) || any_overlap(d_r, 8 * nr, in[k], 8 * in_n[k]))
      return fail(c, who, "an output overlaps an input", SH_ERR_INVALID);
  if (any_overlap(d_q, 8 * nq, d_r, 8 * nr)) return fail(c, who, "the outputs overlap", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_DIVMOD, n_a, n_b)));
  SH_TRY(enter(c));
  uint64_t lc = 0;  // the one read-back: the divisor's leading word, 8 bytes, behind the work already queued on the stream
  HIP_TRY(c, hipMemcpyAsync(&lc, cw(d_b) + (n_b - 1), 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (lc_is_zero(lc, o.M)) return fail(c, who, "the divisor's leading coefficient is zero mod p", SH_ERR_INVALID);
  if (n_a == 0) return SH_OK;
  return pa_divmod(o, cw(d_a), n_a, cw(d_b), n_b, w(d_q), w(d_r));
}

int sh_mod64_poly_divmod(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const uint64_t* a, uint64_t n_a, const uint64_t* b,
                         uint64_t n_b, uint64_t* q, uint64_t* r) {
  static const char who[] = "sh_mod64_poly_divmod";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(divmod_sizes(c, who, n_a, n_b));
  const uint64_t nq = n_a >= n_b ? n_a - n_b + 1 : 0, nr = n_a < n_b - 1 ? n_a : n_b - 1;
  if (!b || (n_a && !a) || (nq && !q) || (nr && !r)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_DIVMOD, n_a, n_b)));
  if (lc_is_zero(b[n_b - 1], o.M)) return fail(c, who, "the divisor's leading coefficient is zero mod p", SH_ERR_INVALID);
  if (n_a == 0) return SH_OK;
  SH_TRY(enter(c));
  uint64_t *x, *y, *oq, *orr;
  SH_TRY(o.upload(a, n_a, sh_ctx::WS_X, &x));
  SH_TRY(o.upload(b, n_b, sh_ctx::WS_Y, &y));
  SH_TRY(o.ws(sh_ctx::WS_MISC, nq + nr, &oq));
  orr = oq + nq;
  SH_TRY(pa_divmod(o, cw(x), n_a, cw(y), n_b, oq, orr));
  if (nq) SH_TRY(o.download(oq, q, nq));
  if (nr) SH_TRY(o.download(orr, r, nr));
  return SH_OK;
}

int sh_dev_mod64_zpoly(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const void* d_xs, uint64_t n, void* d_out) {
  static const char who[] = "sh_dev_mod64_zpoly";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(point_sizes(c, who, n));
  if (!d_out || (n && !d_xs)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (any_overlap(d_out, 8 * (n + 1), d_xs, 8 * n)) return fail(c, who, "the output overlaps the input", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_ZPOLY, n, 0)));
  SH_TRY(enter(c));
  return pa_zpoly(o, cw(d_xs), n, w(d_out));
}

int sh_mod64_zpoly(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const uint64_t* xs, uint64_t n, uint64_t* out) {
  static const char who[] = "sh_mod64_zpoly";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(point_sizes(c, who, n));
  if (!out || (n && !xs)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_ZPOLY, n, 0)));
  SH_TRY(enter(c));
  uint64_t *x = nullptr, *d_out;
  if (n) SH_TRY(o.upload(xs, n, sh_ctx::WS_X, &x));
  SH_TRY(o.ws(sh_ctx::WS_MISC, n + 1, &d_out));
  SH_TRY(pa_zpoly(o, cw(x), n, d_out));
  return o.download(d_out, out, n + 1);
}

int sh_dev_mod64_lagrange_interp(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const void* d_xs, const void* d_ys,
                                 uint64_t n, void* d_out) {
  static const char who[] = "sh_dev_mod64_lagrange_interp";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(point_sizes(c, who, n));
  if (n && (!d_xs || !d_ys || !d_out)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  if (any_overlap(d_out, 8 * n, d_xs, 8 * n) || any_overlap(d_out, 8 * n, d_ys, 8 * n))
    return fail(c, who, "the output overlaps an input", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_LAGRANGE, n, 0)));
  if (n == 0) return SH_OK;
  SH_TRY(enter(c));
  return pa_lagrange(o, cw(d_xs), cw(d_ys), n, w(d_out));
}

int sh_mod64_lagrange_interp(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const uint64_t* xs, const uint64_t* ys,
                             uint64_t n, uint64_t* out) {
  static const char who[] = "sh_mod64_lagrange_interp";
  if (!c) return SH_ERR_INVALID;
  SH_TRY(point_sizes(c, who, n));
  if (n && (!xs || !ys || !out)) return fail(c, who, "null pointer", SH_ERR_INVALID);
  Mod64Ops o;
  SH_TRY(o.init(c, who, modulus, root, root_log));
  SH_TRY(o.fits(who, mp_max_transform(MP_OP_LAGRANGE, n, 0)));
  if (n == 0) return SH_OK;
  SH_TRY(enter(c));
  uint64_t *x, *y, *d_out;
  SH_TRY(o.upload(xs, n, sh_ctx::WS_X, &x));
  SH_TRY(o.upload(ys, n, sh_ctx::WS_Y, &y));
  SH_TRY(o.ws(sh_ctx::WS_MISC, n, &d_out));
  SH_TRY(pa_lagrange(o, cw(x), cw(y), n, d_out));
  return o.download(d_out, out, n);
}

int sh_dev_mod64_poly_eval(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const void* d_coefs, uint64_t n, uint32_t batch,
                           const void* d_xs, uint64_t m, void* d_out) {
  static const char who[] = "sh_dev_mod64_poly_eval";
  if (!c) return SH_ERR_INVALID;
  Mod64Ops o;
  bool direct = true;
  SH_TRY(eval_check(c, who, &o, modulus, root, root_log, d_coefs, n, batch, d_xs, m, d_out, &direct));
  if (m == 0) return SH_OK;
  SH_TRY(enter(c));
  return pa_eval(o, cw(d_coefs), n, batch, cw(d_xs), m, w(d_out), direct);
}

int sh_mod64_poly_eval(sh_ctx* c, uint64_t modulus, uint64_t root, uint32_t root_log, const uint64_t* coefs, uint64_t n, uint32_t batch,
                       const uint64_t* xs, uint64_t m, uint64_t* out) {
  static const char who[] = "sh_mod64_poly_eval";
  if (!c) return SH_ERR_INVALID;
  Mod64Ops o;
  bool direct = true;
  SH_TRY(eval_check(c, who, &o, modulus, root, root_log, coefs, n, batch, xs, m, out, &direct));
  if (m == 0) return SH_OK;
  SH_TRY(enter(c));
  uint64_t *x = nullptr, *d_xs, *d_out;
  if (n) SH_TRY(o.upload(coefs, (uint64_t)batch * n, sh_ctx::WS_X, &x));
  SH_TRY(o.upload(xs, m, sh_ctx::WS_Y, &d_xs));
  SH_TRY(o.ws(sh_ctx::WS_MISC, (uint64_t)batch * m, &d_out));
  SH_TRY(pa_eval(o, cw(x), n, batch, cw(d_xs), m, d_out, direct));
  return o.download(d_out, out, (uint64_t)batch * m);
}
}  // extern "C"
