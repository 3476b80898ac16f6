// api_ntt.hip -- the MiMC-field NTT on the host side: twiddle-table plans, the pass driver, and the transform, product,
// power-cycle and low-degree-extension entry points of include/starkhip.h.
#include "ctx.hpp"
using namespace shk;

namespace {
constexpr int DIRECT_TABLE_LOG = 18;  // power tables up to 2^18 entries (8 MiB, L2-resident) are stored in full; larger ones as two halves

// host table -> device, in stream order (no device-wide synchronisation: the host vector is pageable, so h2d has
// consumed it on return, and every reader of the table is a later launch on the same stream)
int upload_bytes(sh_ctx* c, NttPlan* pl, const void* host, size_t bytes, void** dev) {
  SH_TRY(plan_alloc(c, pl, bytes, dev));
  return h2d(c, *dev, host, bytes, true);
}
int upload_table(sh_ctx* c, NttPlan* pl, const std::vector<fp>& host, fp** dev) {
  void* d = nullptr;
  SH_TRY(upload_bytes(c, pl, host.data(), host.size() * sizeof(fp), &d));
  *dev = reinterpret_cast<fp*>(d);
  return SH_OK;
}

// table of factor * g^e, e < 2^log_order (factor may be null).  Up to 2^direct_log entries the table is stored in full
// (one load per lookup); larger ones as two halves lo[e & mask] * hi[e >> lb] (one more modmul per lookup).  Full tables
// above 2^18 entries are expanded on the device from the two halves.
int build_pow_table(sh_ctx* c, NttPlan* pl, const fp& g, int log_order, const fp* factor, PowTable* out,
                    int direct_log = DIRECT_TABLE_LOG) {
  const bool direct = log_order <= direct_log;
  const bool host_direct = direct && log_order <= DIRECT_TABLE_LOG;
  const int lb = host_direct ? log_order : (log_order + 1) / 2;
  std::vector<fp> lo((size_t)1 << lb);
  lo[0] = fp_one();
  for (size_t i = 1; i < lo.size(); ++i) lo[i] = fp_mul(lo[i - 1], g);
  const fp gs = fp_mul(lo.back(), g);  // g^(2^lb)
  if (host_direct && factor)
    for (auto& v : lo) v = fp_mul(v, *factor);
  if (host_direct) {
    SH_TRY(upload_table(c, pl, lo, &out->lo));
    out->lb = (uint32_t)lb;
    out->hi = nullptr;
    return SH_OK;
  }
  std::vector<fp> hi((size_t)1 << (log_order - lb));
  hi[0] = factor ? *factor : fp_one();
  for (size_t i = 1; i < hi.size(); ++i) hi[i] = fp_mul(hi[i - 1], gs);
  if (!direct) {
    SH_TRY(upload_table(c, pl, lo, &out->lo));
    SH_TRY(upload_table(c, pl, hi, &out->hi));
    out->lb = (uint32_t)lb;
    return SH_OK;
  }
  // expand on the device, in stream order: full[e] = lo[e & mask] * hi[e >> lb] (the two small halves stay with the plan)
  void* full = nullptr;
  fp *dlo = nullptr, *dhi = nullptr;
  SH_TRY(plan_alloc(c, pl, sizeof(fp) << log_order, &full));
  SH_TRY(upload_table(c, pl, lo, &dlo));
  SH_TRY(upload_table(c, pl, hi, &dhi));
  HIP_TRY(c, shk_powers(dlo, dhi, (uint32_t)lb, reinterpret_cast<fp*>(full), (uint64_t)1 << log_order, c->stream));
  out->lo = reinterpret_cast<fp*>(full);
  out->hi = nullptr;
  out->lb = (uint32_t)log_order;
  return SH_OK;
}

// the passes of a 2^log_n-point transform (knobs.hpp:shk_choose_radices; one decomposition per size)
void choose_radices(int log_n, std::vector<int>* out) {
  int r[4];
  const int m = shk_choose_radices(log_n, r);
  out->assign(r, r + m);
}

std::string plan_key(const fp& root, uint64_t n, bool scaled) {
  uint8_t b[32];
  h_to_wire(root, b);
  std::string k(reinterpret_cast<const char*>(b), 32);
  k += std::to_string(n);
  k += scaled ? "s" : "u";
  return k;
}

// root must have order exactly n (a power of two): for n > 1 that is root^(n/2) == -1
// (the reference finds n by walking the powers of the root, fft.py:319-321).
int check_root_order(const fp& root, uint64_t n) {
  if (n == 1) return fp_eq_canon(fp_canon(root), fp_one()) ? SH_OK : SH_ERR_ROOT_ORDER;
  const fp h = fp_canon(h_pow(root, n / 2));
  const fp m1 = fp_canon(fp_neg(fp_one()));
  return fp_eq_canon(h, m1) ? SH_OK : SH_ERR_ROOT_ORDER;
}

// Several vectors from page-locked host buffers: the vectors go through in up to 8 chunks, H2D on one copy stream, wire -> limb,
// transform, limb -> wire on the ctx stream, D2H on a second copy stream, chained by events -- the upload of chunk k + 1 and the
// download of chunk k - 1 run under the transform of chunk k (PCIe is full duplex), instead of upload, transform, download in a row.
int ntt_batch_pipelined(sh_ctx* c, NttPlan* pl, const uint8_t* in, uint8_t* out, uint64_t n, uint32_t batch) {
  const uint32_t nch = batch < 8 ? batch : 8;
  const uint32_t per = (batch + nch - 1) / nch;
  void *w_in = nullptr, *x = nullptr, *w_out = nullptr, *ntt_ws = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)batch * n * 32, &w_in));
  SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)batch * n * sizeof(fp), &x));
  SH_TRY(ws_get(c, sh_ctx::WS_Y, (size_t)batch * n * 32, &w_out));
  SH_TRY(ws_get(c, sh_ctx::WS_NTT, (size_t)per * n * sizeof(fp), &ntt_ws));  // sized once: run_ntt must not reallocate mid-pipeline
  if (!c->io_in) HIP_TRY(c, hipStreamCreateWithFlags(&c->io_in, hipStreamNonBlocking));
  if (!c->io_out) HIP_TRY(c, hipStreamCreateWithFlags(&c->io_out, hipStreamNonBlocking));
  struct Events {
    hipEvent_t e[17] = {};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } ev;
  for (uint32_t k = 0; k < 2 * nch + 1; ++k) HIP_TRY(c, hipEventCreateWithFlags(&ev.e[k], hipEventDisableTiming));
  // earlier work on the ctx stream may still use the workspaces: the uploads start behind it
  HIP_TRY(c, hipEventRecord(ev.e[2 * nch], c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->io_in, ev.e[2 * nch], 0));
  int rc = SH_OK;
  for (uint32_t k = 0; k < nch && rc == SH_OK; ++k) {
    const uint64_t v0 = (uint64_t)k * per, v1 = v0 + per < batch ? v0 + per : batch;
    if (v0 >= v1) break;
    const size_t off = (size_t)v0 * n * 32, len = (size_t)(v1 - v0) * n * 32;
    hipError_t e = hipMemcpyAsync(static_cast<uint8_t*>(w_in) + off, in + off, len, hipMemcpyHostToDevice, c->io_in);
    if (e == hipSuccess) e = hipEventRecord(ev.e[k], c->io_in);
    if (e != hipSuccess) rc = SH_ERR_HIP;
  }
  for (uint32_t k = 0; k < nch && rc == SH_OK; ++k) {
    const uint64_t v0 = (uint64_t)k * per, v1 = v0 + per < batch ? v0 + per : batch;
    if (v0 >= v1) break;
    const size_t off = (size_t)v0 * n * 32, len = (size_t)(v1 - v0) * n * 32;
    fp* xk = reinterpret_cast<fp*>(x) + v0 * n;
    hipError_t e = hipStreamWaitEvent(c->stream, ev.e[k], 0);
    if (e == hipSuccess) e = shk_wire_to_limb(static_cast<uint8_t*>(w_in) + off, xk, (v1 - v0) * n, c->stream);
    if (e != hipSuccess) { rc = SH_ERR_HIP; break; }
    rc = run_ntt(c, pl, xk, xk, (uint32_t)(v1 - v0));
    if (rc != SH_OK) break;
    e = shk_limb_to_wire(xk, static_cast<uint8_t*>(w_out) + off, (v1 - v0) * n, c->stream);
    if (e == hipSuccess) e = hipEventRecord(ev.e[nch + k], c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->io_out, ev.e[nch + k], 0);
    if (e == hipSuccess) e = hipMemcpyAsync(out + off, static_cast<uint8_t*>(w_out) + off, len, hipMemcpyDeviceToHost, c->io_out);
    if (e != hipSuccess) rc = SH_ERR_HIP;
  }
  // whatever happened, nothing of this call may still be in flight when the caller's buffers and the events go away
  (void)hipStreamSynchronize(c->io_in);
  (void)hipStreamSynchronize(c->stream);
  const hipError_t es = hipStreamSynchronize(c->io_out);
  if (rc == SH_OK && es != hipSuccess) rc = SH_ERR_HIP;
  if (rc == SH_ERR_HIP && c->err.empty()) c->err = "pipelined transform: HIP error";
  return rc;
}

// the two plans of a low-degree extension: the trace's inverse transform over G1 = G2^ext (stark.py:217-220), the domain's forward one
int lde_plans(sh_ctx* c, const uint8_t g2[32], uint64_t steps, uint32_t ext, NttPlan** inv1, NttPlan** fwd2) {
  SH_TRY(plan_for(c, g2, steps * ext, false, fwd2));
  uint8_t g1b[32];
  h_to_wire(h_pow((*fwd2)->root, ext), g1b);
  return plan_for(c, g1b, steps, true, inv1);
}
}  // namespace

namespace shk {
int get_plan(sh_ctx* c, const fp& root_eff, uint64_t n, bool scaled, NttPlan** out) {
  std::vector<int> radix;
  choose_radices(ilog2(n), &radix);
  if (radix.empty()) return SH_ERR_UNSUPPORTED;
  const std::string key = plan_key(root_eff, n, scaled);
  if ((*out = plan_find(c, key))) return SH_OK;
  PlanHolder holder;  // frees the partial plan on every exit before plan_commit
  NttPlan* pl = holder.p;
  pl->n = n;
  pl->log_n = ilog2(n);
  pl->scaled = scaled;
  pl->root = root_eff;
  pl->radix = radix;
  const size_t m = pl->radix.size();
  fp ninv = fp_one();
  if (scaled) ninv = h_pow(h_inv(fp_from_u32(2u)), (uint64_t)pl->log_n);  // n^-1 = (2^-1)^log_n
  int rc = build_pow_table(c, pl, root_eff, pl->log_n, nullptr, &pl->base);
  if (rc == SH_OK && pl->log_n >= 2) {
    std::map<int, const fp2*> wr_by_radix;
    int log_P = 0;
    for (size_t d = 0; d < m && rc == SH_OK; ++d) {
      const int r = pl->radix[d];
      if (!wr_by_radix.count(r)) {
        const fp wr = h_pow(root_eff, n >> r);
        std::vector<fp> t((size_t)1 << (r - 1));
        t[0] = fp_one();
        for (size_t i = 1; i < t.size(); ++i) t[i] = fp_mul(t[i - 1], wr);
        // the butterflies multiply by these through fp_mul2: every entry is followed by its image times 2^128
        fp two128 = fp_zero();
        two128.v[4] = 1;
        std::vector<fp> pairs(2 * t.size());
        for (size_t i = 0; i < t.size(); ++i) {
          pairs[2 * i] = t[i];
          pairs[2 * i + 1] = fp_canon(fp_mul(t[i], two128));
        }
        fp* dev = nullptr;
        rc = upload_table(c, pl, pairs, &dev);
        wr_by_radix[r] = reinterpret_cast<const fp2*>(dev);
      }
      pl->wR.push_back(wr_by_radix[r]);
      if (rc == SH_OK && d + 1 < m) {
        PowTable t;
        if (d == 0 && !scaled) {
          t = pl->base;  // P_1 = 1: the table of the root itself
        } else {
          const fp g = h_pow(root_eff, 1ull << log_P);
          rc = build_pow_table(c, pl, g, pl->log_n - log_P, (d == 0 && scaled) ? &ninv : nullptr, &t);
        }
        pl->tw.push_back(t);
        // the tile passes read their inter-pass twiddles g^(j2 k) as rows of adjacent columns: a [k][j2] copy of the
        // table, tw2[k * S + j2] -- one coalesced load per element instead of a scattered one (plus, above 2^18
        // entries, the second modmul of the two-half lookup).  n / P entries: 32 MiB for the first pass of 2^20 points;
        // above 2^23 entries (STARKHIP_TW2_MAX_LOG) the pass keeps the power-table lookup.
        fp* tw2 = nullptr;
        const int log_S = pl->log_n - log_P - r;
        if (rc == SH_OK && r + log_S <= shk_knobs().tw2_max_log) {
          // a failed allocation of the row table (up to 512 MiB) is not fatal: the pass keeps the power-table lookup
          void* dv = nullptr;
          if (plan_alloc(c, pl, sizeof(fp) << (r + log_S), &dv) == SH_OK) {
            tw2 = reinterpret_cast<fp*>(dv);
            HIP_TRY(c, shk_tw2(t.lo, t.hi, t.lb, tw2, (uint32_t)r, (uint32_t)log_S, c->stream));
          } else {
            (void)hipGetLastError();
            c->err.clear();
          }
        }
        pl->tw2.push_back(tw2);
      }
      log_P += r;
    }
  }
  if (rc == SH_OK && scaled && m == 1) {
    std::vector<fp> s(1, ninv);
    rc = upload_table(c, pl, s, &pl->scale);
  }
  if (rc != SH_OK) return rc;
  *out = plan_commit(c, key, &holder);
  return SH_OK;
}

// d_out = NTT(d_in) over plan->root; [batch][n] limb form; d_in may equal d_out.
// n_in != 0: d_in holds n_in <= n elements per vector ([batch][n_in]) and stands for its zero-padded extension
// (fft.py:323-324); d_in must then not alias d_out.  The first pass reads the short source and takes the rest as zeros.
int run_ntt(sh_ctx* c, NttPlan* pl, const fp* d_in, fp* d_out, uint32_t batch, uint64_t n_in) {
  const uint64_t n = pl->n;
  if (batch == 0) return SH_OK;
  if (n_in >= n) n_in = 0;
  if (n_in && pl->log_n <= 1) {  // the tiny transform has no short-source load
    HIP_TRY(c, shk_pad_copy(d_in, d_out, n_in, n, batch, c->stream));
    d_in = d_out;
    n_in = 0;
  }
  if (pl->log_n <= 1) {
    HIP_TRY(c, shk_launch_ntt_tiny(d_in, d_out, (uint32_t)n, batch, n == 2 ? pl->scale : nullptr, c->stream));
    return SH_OK;
  }
  const size_t m = pl->radix.size();
  const fp* src = d_in;
  fp* work = d_out;
  if (m > 1) {
    void* w = nullptr;
    SH_TRY(ws_get(c, sh_ctx::WS_NTT, (size_t)batch * n * sizeof(fp), &w));
    work = reinterpret_cast<fp*>(w);
  }
  int log_P = 0;
  for (size_t d = 0; d < m; ++d) {
    const int r = pl->radix[d];
    NttPassArgs a;
    memset(&a, 0, sizeof a);
    a.log_n = (uint32_t)pl->log_n;
    a.wR = pl->wR[d];
    a.src_n = d == 0 ? n_in : 0;
    const bool last = d + 1 == m;
    if (!last) {
      a.src = src;
      a.dst = work;
      a.log_S = (uint32_t)(pl->log_n - log_P - r);
      a.total = (uint64_t)batch << (pl->log_n - r);  // batch * P * S columns
      a.tw_lo = pl->tw[d].lo;
      a.tw_hi = pl->tw[d].hi;
      a.tw_lb = pl->tw[d].lb;
      a.tw_direct = pl->tw[d].hi == nullptr;
      a.tw2 = pl->tw2[d];
      src = work;
    } else {
      a.src = src;
      a.dst = d_out;
      a.log_P = (uint32_t)(pl->log_n - r);
      a.total = (uint64_t)batch << a.log_P;  // rows
      a.ndig = (uint32_t)(m - 1);
      for (size_t k = 0; k + 1 < m; ++k) a.dig_log[k] = (uint32_t)pl->radix[k];
      a.scale = (m == 1) ? pl->scale : nullptr;
    }
    a.pass_index = (uint32_t)d;
    HIP_TRY(c, shk_launch_ntt_pass(r, last, a, c->stream));
    log_P += r;
  }
  return SH_OK;
}

int plan_for(sh_ctx* c, const uint8_t root[32], uint64_t n, bool inverse, NttPlan** out) {
  if (!is_pow2(n) || n > (1ull << 32)) return n > (1ull << 32) ? SH_ERR_UNSUPPORTED : SH_ERR_INVALID;
  fp w = h_from_wire(root);
  SH_TRY(check_root_order(w, n));
  if (inverse) w = h_pow(w, n - 1);  // w^-1: the reversed root list rootz[:0:-1] of fft.py:327
  return get_plan(c, w, n, inverse, out);
}
}  // namespace shk

extern "C" {

int sh_dev_ntt(sh_ctx* c, const void* d_in, void* d_out, uint64_t n, uint32_t batch, const uint8_t root[32],
               int inverse) {
  if (!c || !d_in || !d_out || !root) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  NttPlan* pl = nullptr;
  SH_TRY(plan_for(c, root, n, inverse != 0, &pl));
  return run_ntt(c, pl, reinterpret_cast<const fp*>(d_in), reinterpret_cast<fp*>(d_out), batch);
}
int sh_dev_lde(sh_ctx* c, void* d_trace, void* d_out, uint64_t steps, uint32_t ext, uint32_t cols, const uint8_t g2[32]) {
  if (!c || !d_trace || !d_out || !g2 || cols == 0 || !is_pow2(steps) || !is_pow2(ext)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  NttPlan *inv1 = nullptr, *fwd2 = nullptr;
  SH_TRY(lde_plans(c, g2, steps, ext, &inv1, &fwd2));
  fp* t = reinterpret_cast<fp*>(d_trace);
  fp* x = reinterpret_cast<fp*>(d_out);
  SH_TRY(run_ntt(c, inv1, t, t, cols));                                  // stark.py:27-36
  return run_ntt(c, fwd2, t, x, cols, steps);                            // stark.py:253-256; fft_1d's zero padding implicit
}
int sh_ntt_batch(sh_ctx* c, const uint8_t* in, uint64_t n_in, uint8_t* out, uint64_t n, uint32_t batch,
                 const uint8_t root[32], int inverse) {
  if (!c || !out || !root || (n_in && !in) || batch == 0) return SH_ERR_INVALID;
  if (n_in > n) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  NttPlan* pl = nullptr;
  SH_TRY(plan_for(c, root, n, inverse != 0, &pl));
  if (batch >= 2 && n_in == n && n >= (1u << 12) && (size_t)batch * n * 32 >= ((size_t)4 << 20) && host_is_pinned(in) &&
      host_is_pinned(out))
    return ntt_batch_pipelined(c, pl, in, out, n, batch);
  fp* x = nullptr;
  uint64_t n_short = 0;
  SH_TRY(upload_short(c, in, n_in, n, batch, sh_ctx::WS_X, &x, &n_short));
  if (n_short) {
    void* y = nullptr;
    SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)batch * n * sizeof(fp), &y));
    SH_TRY(run_ntt(c, pl, x, reinterpret_cast<fp*>(y), batch, n_short));  // fft.py:323-324, zeros not materialised
    x = reinterpret_cast<fp*>(y);
  } else {
    SH_TRY(run_ntt(c, pl, x, x, batch));
  }
  return download_wire(c, x, out, (uint64_t)batch * n);
}
int sh_ntt(sh_ctx* c, const uint8_t* in, uint64_t n_in, uint8_t* out, uint64_t n, const uint8_t root[32], int inverse) {
  return sh_ntt_batch(c, in, n_in, out, n, 1, root, inverse);
}

int sh_mul_polys(sh_ctx* c, const uint8_t* a, uint64_t n_a, const uint8_t* b, uint64_t n_b, uint8_t* out, uint64_t n,
                 const uint8_t root[32]) {
  if (!c || !out || !root || (n_a && !a) || (n_b && !b) || n_a > n || n_b > n) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  NttPlan *fwd = nullptr, *rev = nullptr;
  SH_TRY(plan_for(c, root, n, false, &fwd));
  SH_TRY(get_plan(c, h_pow(fwd->root, n - 1), n, false, &rev));  // reversed roots, NO 1/n (fft.py:345)
  fp *x = nullptr, *y = nullptr;
  SH_TRY(upload_padded(c, a, n_a, n, 1, sh_ctx::WS_X, &x));
  SH_TRY(upload_padded(c, b, n_b, n, 1, sh_ctx::WS_Y, &y));
  SH_TRY(run_ntt(c, fwd, x, x, 1));
  SH_TRY(run_ntt(c, fwd, y, y, 1));
  HIP_TRY(c, shk_pointwise_mul(x, y, x, n, c->stream));
  SH_TRY(run_ntt(c, rev, x, x, 1));
  return download_wire(c, x, out, n);
}

int sh_power_cycle(sh_ctx* c, const uint8_t root[32], uint64_t n, uint8_t* out) {
  if (!c || !out || !root) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  NttPlan* pl = nullptr;
  SH_TRY(plan_for(c, root, n, false, &pl));
  void* x = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)n * sizeof(fp), &x));
  HIP_TRY(c, shk_powers(pl->base.lo, pl->base.hi, pl->base.lb, reinterpret_cast<fp*>(x), n, c->stream));
  return download_wire(c, reinterpret_cast<fp*>(x), out, n);
}

int sh_lde(sh_ctx* c, const uint8_t* trace, uint8_t* out, uint64_t steps, uint32_t ext, uint32_t cols,
           const uint8_t g2[32]) {
  if (!c || !trace || !out || !g2 || cols == 0 || !is_pow2(steps) || !is_pow2(ext)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  const uint64_t n = steps * ext;
  NttPlan *inv1 = nullptr, *fwd2 = nullptr;
  SH_TRY(lde_plans(c, g2, steps, ext, &inv1, &fwd2));
  fp* t = nullptr;
  SH_TRY(upload_padded(c, trace, steps, steps, cols, sh_ctx::WS_Y, &t));
  SH_TRY(run_ntt(c, inv1, t, t, cols));  // trace polynomial coefficients (stark.py:27-36)
  void* x = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_X, (size_t)cols * n * sizeof(fp), &x));
  SH_TRY(run_ntt(c, fwd2, t, reinterpret_cast<fp*>(x), cols, steps));  // stark.py:253-256
  return download_wire(c, reinterpret_cast<fp*>(x), out, (uint64_t)cols * n);
}

uint32_t sh_ntt_passes(uint64_t n, uint32_t batch) {
  if (!is_pow2(n) || n > (1ull << 32)) return 0;
  (void)batch;  // one decomposition per size
  int r[4];
  return (uint32_t)shk_choose_radices(ilog2(n), r);
}
}  // extern "C"
