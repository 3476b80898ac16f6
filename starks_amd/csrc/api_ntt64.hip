// api_ntt64.hip -- the transform over any odd modulus below 2^64 on packed 64-bit words (fp64m.cuh, ntt64_items.cuh), and the
// conversions between word form and limb form.
#include "ctx.hpp"
using namespace shk;

namespace {
const char* const LIMIT = ": n and batch * n are limited to 2^28";  // after the entry point's name
}

namespace shk {
int mod64_prepare(sh_ctx* c, uint64_t modulus, uint64_t root, uint64_t n, uint64_t batch, bool inverse, bool scaled, Mod64Call* mc,
                  const char* who) {
  if (!is_pow2(n) || batch == 0) return SH_ERR_INVALID;
  if (n > (1ull << N64_MAX_LOG_N) || batch > (1ull << N64_MAX_LOG_N) || batch * n > (1ull << N64_MAX_LOG_N)) {
    c->err = std::string(who) + LIMIT;
    return SH_ERR_UNSUPPORTED;
  }
  if (!f64_mod_init(modulus, &mc->M)) {
    c->err = std::string(who) + ": the modulus must be odd and at least 3";
    return SH_ERR_INVALID;
  }
  if (root >= modulus) {
    c->err = std::string(who) + ": root is not below the modulus";
    return SH_ERR_ROOT_ORDER;
  }
  if (!n64_check_root(root, n, mc->M)) {
    c->err = std::string(who) + ": root does not have order n in this ring";
    return SH_ERR_ROOT_ORDER;
  }
  mc->log_n = ilog2(n);
  mc->root_mont = f64_to_mont(root, mc->M);
  if (inverse) mc->root_mont = f64_pow(mc->root_mont, n - 1, mc->M);  // w^-1 = w^(n-1)
  mc->scale = scaled ? n64_inv_n(mc->log_n, mc->M) : 1;
  return SH_OK;
}

// the tables of (modulus, effective root, n) -- lo | hi | stw in one allocation: a plan like any other -- same map, same byte budget,
// same LRU pass, same statistics
int mod64_table(sh_ctx* c, const Mod64Call& mc, const uint64_t** out) {
  *out = nullptr;
  if (mc.log_n == 0) return SH_OK;
  std::string key("m64:");
  key.append(reinterpret_cast<const char*>(&mc.M.p), 8);
  key.append(reinterpret_cast<const char*>(&mc.root_mont), 8);
  key += std::to_string(mc.log_n);
  if (const NttPlan* hit = plan_find(c, key)) {
    *out = reinterpret_cast<const uint64_t*>(hit->owned[0]);
    return SH_OK;
  }
  PlanHolder holder;  // frees the tables on every exit before plan_commit
  holder.p->n = 1ull << mc.log_n;
  holder.p->log_n = mc.log_n;
  int radix[N64_MAX_PASSES];
  n64_plan(mc.log_n, shk_knobs().mod64_tile_log, radix);
  N64Tw t;
  n64_tw_args(mc.root_mont, mc.log_n, radix[0], mc.M, &t);
  void* d = nullptr;
  SH_TRY(plan_alloc(c, holder.p, (size_t)n64_table_bytes(t), &d));
  t.tab = reinterpret_cast<uint64_t*>(d);
  const hipError_t e = shk_n64_tw(t, mc.M, c->stream);
  if (e != hipSuccess) {
    c->err = std::string("packed-word transform tables: ") + hipGetErrorString(e);
    return SH_ERR_HIP;
  }
  plan_commit(c, key, &holder);
  *out = t.tab;
  return SH_OK;
}

// src [batch][n_in] -> dst [batch][n]; src may be dst when n_in == n
int mod64_run(sh_ctx* c, const Mod64Call& mc, const uint64_t* tab, const void* src, uint64_t n_in, void* dst, uint32_t batch) {
  int radix[N64_MAX_PASSES];
  const int tile_log = shk_knobs().mod64_tile_log, m = n64_plan(mc.log_n, tile_log, radix);
  N64Tw t = {};
  if (mc.log_n) n64_tw_args(mc.root_mont, mc.log_n, radix[0], mc.M, &t);  // the table offsets (the squarings are not used here)
  void* work = nullptr;
  if (m > 1) SH_TRY(ws_get(c, sh_ctx::WS_NTT, ((size_t)batch << mc.log_n) * sizeof(uint64_t), &work));
  for (int d = 0; d < m; ++d) {
    N64Pass a = n64_pass(mc.log_n, tile_log, radix, m, d, batch);
    a.lo = tab;
    a.hi = tab ? tab + t.n_lo : nullptr;
    a.stw = tab ? tab + t.n_lo + t.n_hi : nullptr;
    a.src = reinterpret_cast<const uint64_t*>(d == 0 ? src : work);
    a.dst = reinterpret_cast<uint64_t*>(d + 1 == m ? dst : work);
    if (d == 0) a.n_in = n_in;
    if (d + 1 == m) a.scale = mc.scale;
    HIP_TRY(c, shk_n64_pass(a, mc.M, c->stream));
  }
  return SH_OK;
}
}  // namespace shk

extern "C" {

int sh_dev_mod64_ntt(sh_ctx* c, uint64_t modulus, const void* d_in, uint64_t n_in, void* d_out, uint64_t n, uint32_t batch,
                     uint64_t root, int inverse) {
  if (!c || !d_in || !d_out) return SH_ERR_INVALID;
  Mod64Call mc;
  SH_TRY(mod64_prepare(c, modulus, root, n, batch, inverse != 0, inverse != 0, &mc));
  if (n_in > n) return SH_ERR_INVALID;
  if (d_in == d_out ? n_in != n : any_overlap(d_in, (uint64_t)batch * n_in * 8, d_out, (uint64_t)batch * n * 8)) {
    c->err = "sh_dev_mod64_ntt: d_in and d_out overlap (d_in == d_out is allowed when n_in == n)";
    return SH_ERR_INVALID;
  }
  SH_TRY(enter(c));
  const uint64_t* tab = nullptr;
  SH_TRY(mod64_table(c, mc, &tab));
  return mod64_run(c, mc, tab, d_in, n_in, d_out, batch);
}

int sh_mod64_ntt(sh_ctx* c, uint64_t modulus, const uint64_t* in, uint64_t n_in, uint64_t* out, uint64_t n, uint32_t batch,
                 uint64_t root, int inverse) {
  if (!c || !out || (n_in && !in)) return SH_ERR_INVALID;
  if (n_in > (1ull << N64_MAX_LOG_N)) {
    c->err = std::string("sh_mod64_ntt") + LIMIT;
    return SH_ERR_UNSUPPORTED;
  }
  Mod64Call mc;
  SH_TRY(mod64_prepare(c, modulus, root, n, batch, inverse != 0, inverse != 0, &mc));
  if (n_in > n) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  const uint64_t* tab = nullptr;
  SH_TRY(mod64_table(c, mc, &tab));
  void *w = nullptr, *x = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)batch * n_in * 8, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)batch * n * 8, &x));
  SH_TRY(h2d(c, w, in, (size_t)batch * n_in * 8));
  SH_TRY(mod64_run(c, mc, tab, w, n_in, x, batch));  // the zeros beyond n_in are never stored
  return d2h(c, out, x, (size_t)batch * n * 8);
}

int sh_mod64_mul_polys(sh_ctx* c, uint64_t modulus, const uint64_t* a, uint64_t n_a, const uint64_t* b, uint64_t n_b, uint64_t* out,
                       uint64_t n, uint64_t root) {
  if (!c || !out || (n_a && !a) || (n_b && !b)) return SH_ERR_INVALID;
  Mod64Call fwd, rev;
  SH_TRY(mod64_prepare(c, modulus, root, n, 1, false, false, &fwd));
  SH_TRY(mod64_prepare(c, modulus, root, n, 1, true, false, &rev));  // reversed roots, NO 1/n (fft.py:345)
  if (n_a > n || n_b > n) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  const uint64_t *tf = nullptr, *tr = nullptr;
  SH_TRY(mod64_table(c, fwd, &tf));
  SH_TRY(mod64_table(c, rev, &tr));
  void *w = nullptr, *x = nullptr, *y = nullptr, *z = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)(n_a > n_b ? n_a : n_b) * 8, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)n * 8, &x));
  SH_TRY(ws_get(c, sh_ctx::WS_Y, (size_t)n * 8, &y));
  SH_TRY(ws_get(c, sh_ctx::WS_MISC, (size_t)n * 8, &z));
  SH_TRY(h2d(c, w, a, (size_t)n_a * 8));
  SH_TRY(mod64_run(c, fwd, tf, w, n_a, x, 1));
  SH_TRY(h2d(c, w, b, (size_t)n_b * 8));
  SH_TRY(mod64_run(c, fwd, tf, w, n_b, y, 1));
  HIP_TRY(c, shk_n64_pointwise(reinterpret_cast<const uint64_t*>(x), reinterpret_cast<const uint64_t*>(y), reinterpret_cast<uint64_t*>(x),
                               n, fwd.M, c->stream));
  SH_TRY(mod64_run(c, rev, tr, x, n, z, 1));
  return d2h(c, out, z, (size_t)n * 8);
}

int sh_dev_mod64_from_limbs(sh_ctx* c, uint64_t modulus, const void* d_limbs, void* d_words, uint64_t count) {
  if (!c || (count && (!d_limbs || !d_words))) return SH_ERR_INVALID;
  f64_mod M;
  if (!f64_mod_init(modulus, &M)) {
    c->err = "sh_dev_mod64_from_limbs: the modulus must be odd and at least 3";
    return SH_ERR_INVALID;
  }
  if (any_overlap(d_limbs, count * 32, d_words, count * 8)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  HIP_TRY(c, shk_n64_from_limbs(d_limbs, reinterpret_cast<uint64_t*>(d_words), count, M, c->stream));
  return SH_OK;
}

int sh_dev_mod64_to_limbs(sh_ctx* c, const void* d_words, void* d_limbs, uint64_t count) {
  if (!c || (count && (!d_words || !d_limbs))) return SH_ERR_INVALID;
  if (any_overlap(d_words, count * 8, d_limbs, count * 32)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  HIP_TRY(c, shk_n64_to_limbs(reinterpret_cast<const uint64_t*>(d_words), d_limbs, count, c->stream));
  return SH_OK;
}
}  // extern "C"
