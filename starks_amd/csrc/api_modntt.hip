// api_modntt.hip -- the transform over any odd modulus below 2^256 (fft.py:256-345 with a run-time modulus; fpm.cuh, modntt_items.cuh).
#include "ctx.hpp"
using namespace shk;

namespace shk {
// (ctx.hpp has ModCall and the three declarations: the commit over another modulus, api_modfri.hip, transforms with them)
int mod_prepare(sh_ctx* c, const uint8_t modulus[32], const uint8_t root[32], uint64_t n, uint64_t batch, bool inverse, bool scaled,
                ModCall* mc, const char* who) {
  const std::string pre = std::string(who) + ": ";
  if (!is_pow2(n) || batch == 0) {
    c->err = pre + "n must be a power of two and batch at least 1";
    return SH_ERR_INVALID;
  }
  if (n > (1ull << MN_MAX_LOG_N) || batch > (1ull << MN_MAX_LOG_N) || batch * n > (1ull << MN_MAX_LOG_N)) {
    c->err = pre + "n and batch * n are limited to 2^26";
    return SH_ERR_UNSUPPORTED;
  }
  if (!fpm_mod_init(modulus, &mc->M)) {
    c->err = pre + "the modulus must be odd and at least 3";
    return SH_ERR_INVALID;
  }
  const fpm w = fpm_from_wire_bytes(root);
  if (!fpm_below_p(w, mc->M)) {
    c->err = pre + "root is not below the modulus";
    return SH_ERR_ROOT_ORDER;
  }
  if (!mn_check_root(w, n, mc->M)) {
    c->err = pre + "root does not have order n in this ring";
    return SH_ERR_ROOT_ORDER;
  }
  mc->log_n = ilog2(n);
  mc->root_mont = fpm_to_mont(w, mc->M);
  if (inverse) mc->root_mont = fpm_pow(mc->root_mont, n - 1, mc->M);  // w^-1 = w^(n-1)
  mc->scale = scaled ? mn_inv_n(mc->log_n, mc->M) : fpm_from_u32(1u);
  return SH_OK;
}

// the table of (modulus, effective root, n): a plan like any other -- same map, same byte budget, same LRU pass, same statistics
int mod_table(sh_ctx* c, const ModCall& mc, const fpm** out) {
  *out = nullptr;
  if (mc.log_n == 0) return SH_OK;
  std::string key("mod:");
  key.append(reinterpret_cast<const char*>(mc.M.p), 32);
  key.append(reinterpret_cast<const char*>(mc.root_mont.v), 32);
  key += std::to_string(mc.log_n);
  if (const NttPlan* hit = plan_find(c, key)) {
    *out = reinterpret_cast<const fpm*>(hit->owned[0]);
    return SH_OK;
  }
  PlanHolder holder;  // frees the table on every exit before plan_commit
  holder.p->n = 1ull << mc.log_n;
  holder.p->log_n = mc.log_n;
  MnTw t;
  mn_tw_args(mc.root_mont, mc.log_n, mc.M, &t);
  void* d = nullptr;
  SH_TRY(plan_alloc(c, holder.p, (size_t)t.count * sizeof(fpm), &d));
  t.tw = reinterpret_cast<fpm*>(d);
  const hipError_t e = shk_mn_tw(t, mc.M, c->stream);
  if (e != hipSuccess) {
    c->err = std::string("generic transform table: ") + hipGetErrorString(e);
    return SH_ERR_HIP;
  }
  plan_commit(c, key, &holder);
  *out = t.tw;
  return SH_OK;
}

// src [batch][n_in] (wire form when wire_in) -> dst [batch][n] (wire form when wire_out); src may be dst when n_in == n
int mod_run(sh_ctx* c, const ModCall& mc, const fpm* tw, const void* src, uint64_t n_in, void* dst, uint32_t batch, bool wire_in,
            bool wire_out) {
  int radix[MN_MAX_PASSES];
  const int tile_log = shk_knobs().modntt_tile_log, m = mn_plan(mc.log_n, tile_log, radix);
  void* work = nullptr;
  if (m > 1) SH_TRY(ws_get(c, sh_ctx::WS_NTT, ((size_t)batch << mc.log_n) * sizeof(fpm), &work));
  for (int d = 0; d < m; ++d) {
    MnPass a = mn_pass(mc.log_n, tile_log, radix, m, d, batch);
    a.tw = tw;
    a.src = d == 0 ? src : work;
    a.dst = d + 1 == m ? dst : work;
    if (d == 0) {
      a.n_in = n_in;
      a.wire_in = wire_in;
    }
    if (d + 1 == m) {
      a.scale = mc.scale;
      a.wire_out = wire_out;
    }
    HIP_TRY(c, shk_mn_pass(a, mc.M, c->stream));
  }
  return SH_OK;
}
}  // namespace shk

extern "C" {

int sh_dev_mod_ntt(sh_ctx* c, const uint8_t modulus[32], const void* d_in, void* d_out, uint64_t n, uint32_t batch,
                   const uint8_t root[32], int inverse) {
  if (!c || !modulus || !d_in || !d_out || !root) return SH_ERR_INVALID;
  ModCall mc;
  SH_TRY(mod_prepare(c, modulus, root, n, batch, inverse != 0, inverse != 0, &mc));
  SH_TRY(enter(c));
  const fpm* tw = nullptr;
  SH_TRY(mod_table(c, mc, &tw));
  return mod_run(c, mc, tw, d_in, n, d_out, batch, false, false);
}

int sh_mod_ntt(sh_ctx* c, const uint8_t modulus[32], const uint8_t* in, uint64_t n_in, uint8_t* out, uint64_t n, uint32_t batch,
               const uint8_t root[32], int inverse) {
  if (!c || !modulus || !out || !root || (n_in && !in)) return SH_ERR_INVALID;
  if (n_in > (1ull << MN_MAX_LOG_N)) {
    c->err = "sh_mod_ntt: n and batch * n are limited to 2^26";
    return SH_ERR_UNSUPPORTED;
  }
  ModCall mc;
  SH_TRY(mod_prepare(c, modulus, root, n, batch, inverse != 0, inverse != 0, &mc));
  if (n_in > n) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  const fpm* tw = nullptr;
  SH_TRY(mod_table(c, mc, &tw));
  void *w = nullptr, *x = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)batch * n_in * 32, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)batch * n * 32, &x));
  SH_TRY(h2d(c, w, in, (size_t)batch * n_in * 32));
  SH_TRY(mod_run(c, mc, tw, w, n_in, x, batch, true, true));  // fft.py:323-324: the zeros beyond n_in are never stored
  return d2h(c, out, x, (size_t)batch * n * 32);
}

int sh_mod_mul_polys(sh_ctx* c, const uint8_t modulus[32], const uint8_t* a, uint64_t n_a, const uint8_t* b, uint64_t n_b, uint8_t* out,
                     uint64_t n, const uint8_t root[32]) {
  if (!c || !modulus || !out || !root || (n_a && !a) || (n_b && !b)) return SH_ERR_INVALID;
  ModCall fwd, rev;
  SH_TRY(mod_prepare(c, modulus, root, n, 1, false, false, &fwd));
  SH_TRY(mod_prepare(c, modulus, root, n, 1, true, false, &rev));  // reversed roots, NO 1/n (fft.py:345)
  if (n_a > n || n_b > n) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  const fpm *tf = nullptr, *tr = nullptr;
  SH_TRY(mod_table(c, fwd, &tf));
  SH_TRY(mod_table(c, rev, &tr));
  void *w = nullptr, *x = nullptr, *y = nullptr, *z = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)(n_a > n_b ? n_a : n_b) * 32, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)n * 32, &x));
  SH_TRY(ws_get(c, sh_ctx::WS_Y, (size_t)n * 32, &y));
  SH_TRY(ws_get(c, sh_ctx::WS_MISC, (size_t)n * 32, &z));
  SH_TRY(h2d(c, w, a, (size_t)n_a * 32));
  SH_TRY(mod_run(c, fwd, tf, w, n_a, x, 1, true, false));
  SH_TRY(h2d(c, w, b, (size_t)n_b * 32));
  SH_TRY(mod_run(c, fwd, tf, w, n_b, y, 1, true, false));
  HIP_TRY(c, shk_mn_pointwise(reinterpret_cast<const fpm*>(x), reinterpret_cast<const fpm*>(y), reinterpret_cast<fpm*>(x), n, fwd.M,
                              c->stream));
  SH_TRY(mod_run(c, rev, tr, x, n, z, 1, false, true));
  return d2h(c, out, z, (size_t)n * 32);
}
}  // extern "C"
