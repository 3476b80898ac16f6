// api_stark.hip -- STARK.mk_proof (stark.py:233-279) and AIR.generate_witness on the host side, and their entry points.
#include "ctx.hpp"
using namespace shk;

namespace shk {
// Parse + upload the step polynomials' terms and their partial derivatives (skipped when equal to the previous call's).
int stark_terms(sh_ctx* c, uint32_t width, const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts) {
  if (!coefs || !exps || !counts) return SH_ERR_INVALID;
  uint64_t total = 0;
  for (uint32_t d = 0; d < width; ++d) total += counts[d];
  if (total == 0 || total > SHK_STARK_MAX_TERMS) return total ? SH_ERR_UNSUPPORTED : SH_ERR_INVALID;
  std::vector<uint8_t> key;
  key.push_back((uint8_t)width);
  key.insert(key.end(), reinterpret_cast<const uint8_t*>(counts), reinterpret_cast<const uint8_t*>(counts + width));
  key.insert(key.end(), coefs, coefs + 32 * total);
  key.insert(key.end(), exps, exps + (size_t)width * total);
  if (c->terms_dev && key == c->terms_key) return SH_OK;
  uint32_t degree = 0;
  for (uint64_t t = 0; t < total; ++t) {
    uint32_t sum = 0;
    for (uint32_t v = 0; v < width; ++v) sum += exps[t * width + v];
    if (sum > degree) degree = sum;  // MultivariatePolynomial.degree (multivariate_polynomial.py:111-117)
  }
  std::vector<uint8_t> img(TermLayout::total, 0);
  fp* cf = reinterpret_cast<fp*>(img.data() + TermLayout::coef);
  fp* dcf = reinterpret_cast<fp*>(img.data() + TermLayout::dcoef);
  uint8_t* ex = img.data() + TermLayout::exps;
  uint8_t* dex = img.data() + TermLayout::dexps;
  uint32_t* dbeg = reinterpret_cast<uint32_t*>(img.data() + TermLayout::dbegin);
  const fp one = fp_one();
  const size_t row = width + 1;
  for (uint64_t t = 0; t < total; ++t) {
    cf[t] = h_from_wire(coefs + 32 * t);
    memcpy(ex + t * row, exps + t * width, width);
    ex[t * row + width] = fp_eq_canon(cf[t], one) ? 1 : 0;
  }
  // d/dX_v of coef * prod X^e = (coef * e_v) * X_v^(e_v - 1) * prod_{u != v} X_u^e_u
  uint32_t begin[SHK_STARK_MAX_WIDTH + 1] = {0};
  for (uint32_t d = 0; d < width; ++d) begin[d + 1] = begin[d] + counts[d];
  uint32_t nd = 0;
  for (uint32_t d = 0; d < width; ++d) {
    for (uint32_t v = 0; v < width; ++v) {
      dbeg[d * width + v] = nd;
      for (uint32_t t = begin[d]; t < begin[d + 1]; ++t) {
        const uint32_t e = exps[(size_t)t * width + v];
        if (!e) continue;
        dcf[nd] = fp_canon(fp_mul(cf[t], fp_from_u32(e)));
        memcpy(dex + (size_t)nd * row, exps + (size_t)t * width, width);
        dex[(size_t)nd * row + v] = (uint8_t)(e - 1);
        dex[(size_t)nd * row + width] = fp_eq_canon(dcf[nd], one) ? 1 : 0;
        ++nd;
      }
    }
  }
  dbeg[width * width] = nd;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // earlier launches may still read the old terms
  if (!c->terms_dev) HIP_TRY(c, hipMalloc(&c->terms_dev, TermLayout::total));
  HIP_TRY(c, hipMemcpy(c->terms_dev, img.data(), TermLayout::total, hipMemcpyHostToDevice));
  memcpy(c->terms_begin, begin, sizeof begin);
  c->terms_degree = degree;
  c->terms_key.swap(key);
  return SH_OK;
}

uint64_t stark_header_len(uint64_t n, uint32_t width, uint32_t samples) {
  const uint64_t lg = (uint64_t)ilog2(n), k = 3ull * width;
  return 64 + (uint64_t)samples * 32 * (2 * (2 * k + (lg - 1)) + (lg + 1));
}

int stark_check_shape(uint64_t steps, uint32_t ext, uint32_t width, uint32_t degree, uint32_t samples) {
  if (!is_pow2(steps) || !is_pow2(ext) || steps < 2 || ext < 2 || width == 0 || samples == 0) return SH_ERR_INVALID;
  if (width > SHK_STARK_MAX_WIDTH) return SH_ERR_UNSUPPORTED;
  if (steps > (1ull << 24) || steps * ext >= (1ull << 24)) return SH_ERR_UNSUPPORTED;  // utils.py:69 (spot-check sampling)
  if ((uint64_t)degree * (steps - 1) + 1 >= steps * ext) return SH_ERR_UNSUPPORTED;   // C (X - x_last) must fit the domain
  return fri_validate(steps * ext, steps * degree, ext, 40);
}

// per-proof constraint flags: grown (and zeroed) on demand; flags already raised survive a growth
int bad_flags(sh_ctx* c, uint32_t batch) {
  if (batch <= c->bad_cap) return SH_OK;
  const uint32_t cap = (batch + 63u) & ~63u;
  uint32_t* nf = nullptr;
  HIP_TRY(c, hipMalloc(reinterpret_cast<void**>(&nf), (size_t)cap * 4));
  hipError_t e = hipMemsetAsync(nf, 0, (size_t)cap * 4, c->stream);
  if (e == hipSuccess && c->bad_flag)
    e = hipMemcpyAsync(nf, c->bad_flag, (size_t)c->bad_cap * 4, hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(nf);
    HIP_TRY(c, e);
  }
  if (c->bad_flag) (void)hipFree(c->bad_flag);
  c->bad_flag = nf;
  c->bad_cap = cap;
  return SH_OK;
}
}  // namespace shk

namespace {

int run_stark(sh_ctx* c, fp* d_wit, const fp* d_inputs, uint64_t steps, uint32_t ext, uint32_t width, uint32_t samples,
              uint32_t batch, uint8_t* d_proof) {
  const uint32_t degree = c->terms_degree;
  SH_TRY(stark_check_shape(steps, ext, width, degree, samples));
  if (!d_wit || !d_inputs || !d_proof || batch == 0) return SH_ERR_INVALID;
  if (batch > 65535) return SH_ERR_UNSUPPORTED;  // the leaf / spot-check kernels launch one grid row (blockIdx.y) per proof
  const uint64_t n = steps * ext, cols = (uint64_t)batch * width;
  if (cols > 0xffffffffull) return SH_ERR_UNSUPPORTED;
  const fp g2 = h_root_of_order_pow2(ilog2(n));           // stark.py:205
  uint8_t g2b[32], g1b[32];
  h_to_wire(g2, g2b);
  h_to_wire(h_pow(g2, ext), g1b);                          // G1 = G2^ext (stark.py:208)
  NttPlan *fwd_n, *inv_s, *fwd_s;
  SH_TRY(plan_for(c, g2b, n, false, &fwd_n));
  SH_TRY(plan_for(c, g1b, steps, true, &inv_s));
  SH_TRY(plan_for(c, g1b, steps, false, &fwd_s));
  const fp g1 = h_pow(g2, ext);
  const fp x_last = h_pow(g2, (steps - 1) * ext);          // stark.py:212
  const fp inv_last_m1 = h_inv(fp_sub(x_last, fp_one()));
  const fp cpow = h_pow(h_pow(g2, steps), n - 1);          // `powers[i]` after the loop: (G2^steps)^(precision-1) (stark.py:150-158)

  void *pe, *dw, *bw, *qv, *small, *mt;
  SH_TRY(ws_get(c, sh_ctx::WS_ST_P, cols * n * sizeof(fp), &pe));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_D, cols * n * sizeof(fp), &dw));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_B, cols * n * sizeof(fp), &bw));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_Q, cols * steps * sizeof(fp), &qv));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_MTREE, (size_t)batch * 2 * n * 32, &mt));
  const size_t iab_bytes = cols * 3 * sizeof(fp), scal_bytes = cols * 3 * sizeof(fp2);  // scalars as (s, s 2^128) pairs
  SH_TRY(ws_get(c, sh_ctx::WS_ST_SMALL, iab_bytes + scal_bytes + (size_t)batch * samples * 4, &small));
  fp* iab = reinterpret_cast<fp*>(small);
  fp* scal = reinterpret_cast<fp*>(reinterpret_cast<uint8_t*>(small) + iab_bytes);
  uint32_t* ys = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(small) + iab_bytes + scal_bytes);
  SH_TRY(bad_flags(c, batch));
  // cached per (steps, ext): 1 / (omega^j - 1) for the ext-th roots of unity omega^j = x^steps, and the domain tables
  // 1 / ((x_i - 1)(x_i - x_last)), x_i, (x_i - x_last) / (x_i^steps - 1)   (3 n elements, shared by every proof)
  fp* inv_omega = nullptr;
  {
    const auto key = std::make_pair(steps, ext);
    auto it = c->inv_omega.find(key);
    if (it == c->inv_omega.end()) {
      std::vector<fp> host(ext, fp_zero());
      const fp omega = h_pow(g2, steps);
      fp w = omega;
      for (uint32_t j = 1; j < ext; ++j) {
        host[j] = h_inv(fp_sub(w, fp_one()));
        w = fp_mul(w, omega);
      }
      void* t = nullptr;
      HIP_TRY(c, hipMalloc(&t, ext * sizeof(fp)));
      const hipError_t e = hipMemcpy(t, host.data(), ext * sizeof(fp), hipMemcpyHostToDevice);
      if (e != hipSuccess) {
        (void)hipFree(t);
        HIP_TRY(c, e);
      }
      c->inv_omega[key] = t;
      inv_omega = reinterpret_cast<fp*>(t);
    } else {
      inv_omega = reinterpret_cast<fp*>(it->second);
    }
  }
  fp* inv_z2 = nullptr;
  {
    const auto key = std::make_pair(steps, ext);
    auto it = c->inv_z2.find(key);
    if (it == c->inv_z2.end()) {
      void* t = nullptr;
      HIP_TRY(c, hipMalloc(&t, 3 * n * sizeof(fp)));
      inv_z2 = reinterpret_cast<fp*>(t);
      const hipError_t e = shk_stark_domain_tables(inv_z2, n, ext, fwd_n->base.lo, fwd_n->base.hi, fwd_n->base.lb, x_last, inv_omega,
                                                   c->stream);
      if (e != hipSuccess) {  // never cache a table whose fill did not launch
        (void)hipFree(t);
        HIP_TRY(c, e);
      }
      c->inv_z2[key] = t;
    } else {
      inv_z2 = reinterpret_cast<fp*>(it->second);
    }
  }
  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->terms_dev);
  StarkArgs a;
  memset(&a, 0, sizeof a);
  a.p_evals = reinterpret_cast<fp*>(pe);
  a.d_work = reinterpret_cast<fp*>(dw);
  a.b_work = reinterpret_cast<fp*>(bw);
  a.q_evals = reinterpret_cast<fp*>(qv);
  a.wit = d_wit;
  a.iab = iab;
  a.n = n;
  a.steps = steps;
  a.ext = ext;
  a.width = width;
  a.batch = batch;
  a.tw_lo = fwd_n->base.lo;
  a.tw_hi = fwd_n->base.hi;
  a.tw_lb = fwd_n->base.lb;
  a.inv_z2 = inv_z2;
  a.xpow = inv_z2 + n;
  a.fz = inv_z2 + 2 * n;
  a.inv_omega = inv_omega;
  a.x_last = x_last;
  a.g1 = g1;
  a.inv_steps = h_pow(h_inv(fp_from_u32(2u)), (uint64_t)ilog2(steps));
  a.inv_1_m_last = fp_neg(inv_last_m1);
  a.bad = c->bad_flag;
  a.term_coef = reinterpret_cast<const fp*>(tb + TermLayout::coef);
  a.term_exps = tb + TermLayout::exps;
  memcpy(a.term_begin, c->terms_begin, sizeof a.term_begin);
  a.dterm_coef = reinterpret_cast<const fp*>(tb + TermLayout::dcoef);
  a.dterm_exps = tb + TermLayout::dexps;
  a.dterm_begin = reinterpret_cast<const uint32_t*>(tb + TermLayout::dbegin);
  fp* P = reinterpret_cast<fp*>(pe);
  fp* Q = reinterpret_cast<fp*>(qv);

  // boundary interpolants need witness[dim][-1] before the trace becomes coefficients (stark.py:91-96)
  HIP_TRY(c, shk_stark_interp(d_wit, d_inputs, steps, (uint32_t)cols, inv_last_m1, iab, c->stream));
  // trace polynomials and their evaluations: the low-degree extension (stark.py:27-36, 253-256)
  // (coefficients go to the Q buffer: the witness stays what it is -- the trace polynomials' values on the trace points,
  // which the trace-point kernel reads contiguously)
  SH_TRY(run_ntt(c, inv_s, d_wit, Q, (uint32_t)cols));
  SH_TRY(run_ntt(c, fwd_n, Q, P, (uint32_t)cols, steps));  // the zero padding of fft_1d is implicit (fft.py:323-324)
  // Q = X P'(X) on the trace points, for the quotients' values there
  HIP_TRY(c, shk_stark_qprep(Q, Q, steps, cols, c->stream));
  SH_TRY(run_ntt(c, fwd_s, Q, Q, (uint32_t)cols));
  // D = C / Z and B = (P - I) / Z2 (stark.py:38-104), evaluated on the whole domain, and
  // mtree = merkelize_polynomial_evaluations(width, P + D + B evaluations) (stark.py:257)
  uint32_t* mtree = reinterpret_cast<uint32_t*>(mt);
  HIP_TRY(c, shk_stark_quotients_and_merkelize(a, mtree, c->stream));
  // l = pseudorandom linear combination keyed by mtree's root (stark.py:128-177, 259-263), on evaluations
  FriBuffers fb;
  SH_TRY(fri_buffers(c, n, batch, samples, &fb));
  HIP_TRY(c, shk_stark_scalars(mtree, 2 * n * 8, width, batch, cpow, scal, c->stream));
  HIP_TRY(c, shk_stark_lincomb_tree(a, scal, fb.vals, fb.tree, c->stream));  // l and l_mtree = merkelize(l) in one pass
  // spot checks (stark.py:390-402)
  const uint64_t stride = stark_header_len(n, width, samples) + fri_proof_len(n, steps * (uint64_t)degree, 40);
  HIP_TRY(c, shk_sample_indices(fb.tree, 2 * n * 8, (uint32_t)n, batch, samples, ext, ys, c->stream));
  HIP_TRY(c, shk_stark_gather(a, mtree, fb.tree, fb.vals, ys, samples, d_proof, stride, c->stream));
  // fri.generate_proximity_proof(l_poly, G2, steps * degree, exclude_multiples_of=ext) (stark.py:271-276); its first
  // tree is l_mtree
  return fri_rounds(c, fwd_n, fb, n, steps * (uint64_t)degree, ext, 40, batch, d_proof + stark_header_len(n, width, samples),
                    stride, true);
}

// ---- AIR.generate_witness (air.py:32-52, 121-123) on the device: witness.hip, launched in slices of steps -------------------------
int witness_check(const void* in, const void* out, uint64_t steps, uint32_t width, const uint8_t* coefs, const uint8_t* exps,
                         const uint32_t* counts, uint32_t batch) {
  if (!in || !out || !coefs || !exps || !counts || steps == 0 || batch == 0 || width == 0) return SH_ERR_INVALID;
  if (width > SHK_STARK_MAX_WIDTH) return SH_ERR_UNSUPPORTED;
  uint64_t total = 0;
  for (uint32_t d = 0; d < width; ++d) total += counts[d];
  if (total == 0) return SH_ERR_INVALID;
  if (total > SHK_STARK_MAX_TERMS) return SH_ERR_UNSUPPORTED;
  const uint64_t cols = (uint64_t)batch * width;
  if (cols > 0xffffffffull || steps > (~0ull / 32) / cols) return SH_ERR_UNSUPPORTED;  // the witness's byte count must fit 64 bits
  return SH_OK;
}

// d_wit [batch][width][steps] from d_in [batch][width]; the terms are the ones stark_terms just uploaded
int run_witness(sh_ctx* c, const fp* d_in, fp* d_wit, uint64_t steps, uint32_t width, const uint8_t* coefs, const uint8_t* exps,
                       const uint32_t* counts, uint32_t batch) {
  WiRow rows[SHK_STARK_MAX_TERMS];
  uint32_t T = 0;
  const fp one = fp_one();
  for (uint32_t d = 0; d < width; ++d)
    for (uint32_t i = 0; i < counts[d]; ++i, ++T) rows[T] = wi_pack_row(d, fp_eq_canon(h_from_wire(coefs + 32ull * T), one), exps + (size_t)T * width, width);
  WitnessArgs a;
  memset(&a, 0, sizeof a);
  wi_plan(rows, T, width, (uint32_t)shk_knobs().witness_group, (uint64_t)shk_knobs().witness_slice, &a.plan);
  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->terms_dev);
  a.inputs = d_in;
  a.wit = d_wit;
  a.steps = steps;
  a.batch = batch;
  a.nterms = T;
  a.coef = reinterpret_cast<const fp*>(tb + TermLayout::coef);
  a.exps = tb + TermLayout::exps;
  memcpy(a.begin, c->terms_begin, sizeof a.begin);
  for (a.k0 = 0; a.k0 < steps; a.k0 = a.k1) {  // each dispatch resumes from the last row the previous one wrote
    a.k1 = steps - a.k0 > a.plan.slice ? a.k0 + a.plan.slice : steps;
    HIP_TRY(c, shk_stark_witness_slice(a, width, c->stream));
  }
  return SH_OK;
}
}  // namespace

extern "C" {

uint64_t sh_stark_proof_len(uint64_t steps, uint32_t ext, uint32_t width, uint32_t degree, uint32_t samples) {
  if (stark_check_shape(steps, ext, width, degree, samples) != SH_OK) return 0;
  const uint64_t n = steps * ext;
  return stark_header_len(n, width, samples) + fri_proof_len(n, steps * (uint64_t)degree, 40);
}

int sh_stark_status_batch(sh_ctx* c, uint8_t* bad, uint32_t batch) {
  if (!c || (batch && !bad)) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (bad) memset(bad, 0, batch);
  if (!c->bad_flag) return SH_OK;
  std::vector<uint32_t> flags(c->bad_cap);
  HIP_TRY(c, hipMemcpy(flags.data(), c->bad_flag, (size_t)c->bad_cap * 4, hipMemcpyDeviceToHost));
  bool any = false;
  for (uint32_t b = 0; b < c->bad_cap; ++b) {
    if (!flags[b]) continue;
    any = true;
    if (b < batch) bad[b] = 1;
  }
  if (!any) return SH_OK;
  HIP_TRY(c, hipMemset(c->bad_flag, 0, (size_t)c->bad_cap * 4));
  return SH_ERR_CONSTRAINT;
}
int sh_stark_status(sh_ctx* c) { return sh_stark_status_batch(c, nullptr, 0); }

int sh_dev_fill_mimc_units(sh_ctx* c, void* d_witness, void* d_inputs, uint64_t steps, uint32_t first_unit, uint32_t batch,
                           uint32_t constant) {
  if (!c || !d_witness || !d_inputs || steps == 0 || batch == 0) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, shk_fill_mimc_units(reinterpret_cast<fp*>(d_witness), reinterpret_cast<fp*>(d_inputs), steps, first_unit, batch,
                                 constant, c->stream));
  return SH_OK;
}

int sh_dev_stark_prove(sh_ctx* c, void* d_witness, const void* d_inputs, uint64_t steps, uint32_t ext, uint32_t width,
                       const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts, uint32_t samples,
                       uint32_t batch, void* d_proof) {
  if (!c || width == 0 || width > SHK_STARK_MAX_WIDTH) return c && width > SHK_STARK_MAX_WIDTH ? SH_ERR_UNSUPPORTED : SH_ERR_INVALID;
  SH_TRY(enter(c));
  SH_TRY(stark_terms(c, width, term_coefs, term_exps, term_counts));
  return run_stark(c, reinterpret_cast<fp*>(d_witness), reinterpret_cast<const fp*>(d_inputs), steps, ext, width, samples,
                   batch, reinterpret_cast<uint8_t*>(d_proof));
}

int sh_stark_prove(sh_ctx* c, const uint8_t* witness, const uint8_t* inputs, uint64_t steps, uint32_t ext, uint32_t width,
                   const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts, uint32_t samples,
                   uint32_t batch, uint8_t* proof, uint64_t proof_cap) {
  if (!c || !witness || !inputs || !proof || batch == 0 || width == 0) return SH_ERR_INVALID;
  if (width > SHK_STARK_MAX_WIDTH) return SH_ERR_UNSUPPORTED;
  SH_TRY(enter(c));
  SH_TRY(stark_terms(c, width, term_coefs, term_exps, term_counts));
  SH_TRY(stark_check_shape(steps, ext, width, c->terms_degree, samples));
  const uint64_t n = steps * ext;
  const uint64_t stride = stark_header_len(n, width, samples) + fri_proof_len(n, steps * (uint64_t)c->terms_degree, 40);
  if (proof_cap < stride * batch) return SH_ERR_TOO_SMALL;
  const uint64_t cols = (uint64_t)batch * width;
  fp *w = nullptr, *in = nullptr;
  SH_TRY(upload_padded(c, witness, steps, steps, (uint32_t)cols, sh_ctx::WS_ST_TRACE, &w));
  SH_TRY(upload_padded(c, inputs, 1, 1, (uint32_t)cols, sh_ctx::WS_Y, &in));
  void* dp = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_PROOF, (size_t)stride * batch, &dp));
  // this call reports on its own witnesses only: flags left by unchecked sh_dev_stark_prove calls are dropped
  if (c->bad_flag) HIP_TRY(c, hipMemsetAsync(c->bad_flag, 0, (size_t)c->bad_cap * 4, c->stream));
  SH_TRY(run_stark(c, w, in, steps, ext, width, samples, batch, reinterpret_cast<uint8_t*>(dp)));
  SH_TRY(d2h(c, proof, dp, (size_t)stride * batch));
  return sh_stark_status(c);
}

int sh_dev_stark_witness(sh_ctx* c, const void* d_inputs, uint64_t steps, uint32_t width, const uint8_t* term_coefs,
                         const uint8_t* term_exps, const uint32_t* term_counts, uint32_t batch, void* d_witness) {
  if (!c) return SH_ERR_INVALID;
  SH_TRY(witness_check(d_inputs, d_witness, steps, width, term_coefs, term_exps, term_counts, batch));
  if (any_overlap(d_inputs, 32ull * batch * width, d_witness, 32ull * batch * width * steps)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  SH_TRY(stark_terms(c, width, term_coefs, term_exps, term_counts));
  return run_witness(c, reinterpret_cast<const fp*>(d_inputs), reinterpret_cast<fp*>(d_witness), steps, width, term_coefs, term_exps,
                     term_counts, batch);
}

int sh_stark_witness(sh_ctx* c, const uint8_t* inputs, uint64_t steps, uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps,
                     const uint32_t* term_counts, uint32_t batch, uint8_t* witness, uint64_t witness_cap) {
  if (!c) return SH_ERR_INVALID;
  SH_TRY(witness_check(inputs, witness, steps, width, term_coefs, term_exps, term_counts, batch));
  const uint64_t count = (uint64_t)batch * width * steps;
  if (witness_cap / 32 < count) return SH_ERR_TOO_SMALL;
  SH_TRY(enter(c));
  SH_TRY(stark_terms(c, width, term_coefs, term_exps, term_counts));
  fp* in = nullptr;
  SH_TRY(upload_padded(c, inputs, 1, 1, batch * width, sh_ctx::WS_Y, &in));
  void* w = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_ST_TRACE, (size_t)count * sizeof(fp), &w));
  SH_TRY(run_witness(c, in, reinterpret_cast<fp*>(w), steps, width, term_coefs, term_exps, term_counts, batch));
  return download_wire(c, reinterpret_cast<fp*>(w), witness, count);
}
}  // extern "C"
