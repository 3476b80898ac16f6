// api_modstark.hip -- STARK.mk_proof (stark.py:233-279) over any prime modulus below 2^256 on the host side, and its entry points: the
// transforms are api_modntt.hip's, the middle of the prover modstark.hip's, the commit rounds api_modfri.hip's (modfri_rounds, on the
// evaluations and the tree built here), the tree levels above the leaf kernels and the index sampler the MiMC path's (kernels.hip).
// Also AIR.generate_witness over any odd modulus (sh_mod_stark_witness, sh_dev_mod_stark_witness: modwitness.hip launched in slices).
// Every check runs on the host before anything is launched.
#include "ctx.hpp"
#include "modstark_items.cuh"
using namespace shk;

namespace {
// everything the host derives from the arguments before a launch
struct ModStarkCall {
  ModCall fwd_n, inv_s, fwd_s;  // the n-point transform over G2, the steps-point inverse and forward transforms over G1
  fpm g2;                       // Montgomery form
  fpm pm2;                      // p - 2, an integer
  uint32_t degree;
  uint64_t total_terms;
  uint64_t stride;              // bytes of one proof
};

int refuse(sh_ctx* c, const char* who, int rc, const char* why) {
  c->err = std::string(who) + ": " + why;
  return rc;
}

// every host check of a proof; on SH_OK sc holds the call's constants.  Nothing here touches the device.
int mod_stark_check(sh_ctx* c, const char* who, const uint8_t modulus[32], uint64_t steps, uint32_t ext, uint32_t width,
                    const uint8_t* exps, const uint32_t* counts, uint32_t samples, uint32_t batch, ModStarkCall* sc) {
  fpm_mod M;
  if (!fpm_mod_init(modulus, &M)) return refuse(c, who, SH_ERR_INVALID, "the modulus must be odd and at least 3");
  if (width == 0 || batch == 0) return refuse(c, who, SH_ERR_INVALID, "width and batch must be at least 1");
  if (width > SHK_STARK_MAX_WIDTH) return refuse(c, who, SH_ERR_UNSUPPORTED, "width is limited to 9 (stark.py:106-126)");
  if (batch > 65535) return refuse(c, who, SH_ERR_UNSUPPORTED, "a call takes at most 65535 proofs");
  uint64_t total = 0;
  for (uint32_t d = 0; d < width; ++d) total += counts[d];
  if (total == 0) return refuse(c, who, SH_ERR_INVALID, "the step polynomials have no terms");
  if (total > SHK_STARK_MAX_TERMS) return refuse(c, who, SH_ERR_UNSUPPORTED, "more step-polynomial terms than SHK_STARK_MAX_TERMS");
  const uint32_t degree = ms_terms_degree(exps, width, total);
  const int rc = stark_check_shape(steps, ext, width, degree, samples);
  if (rc != SH_OK)
    return refuse(c, who, rc,
                  "steps and ext must be powers of two >= 2 with steps * ext < 2^24, degree * (steps - 1) + 1 < steps * ext, samples >= 1, "
                  "and the commit of steps * degree coefficients on steps * ext points must be one sh_mod_fri_prove accepts");
  const uint64_t n = steps * ext, cols = (uint64_t)batch * width;
  sc->g2 = ms_g2(M, ilog2(n));  // 7^((p - 1) // (steps * ext)) (stark.py:205)
  uint8_t g2b[32], g1b[32];
  fpm_to_wire_bytes(fpm_from_mont(sc->g2, M), g2b);
  fpm_to_wire_bytes(fpm_from_mont(fpm_pow(sc->g2, ext, M), M), g1b);
  const int rr = mod_prepare(c, modulus, g2b, n, cols, false, false, &sc->fwd_n, who);
  if (rr == SH_ERR_ROOT_ORDER)
    return refuse(c, who, rr, "G2 = 7^((p - 1) // (steps * ext)) does not have order steps * ext modulo p (G2^(n/2) != -1)");
  SH_TRY(rr);
  SH_TRY(mod_prepare(c, modulus, g1b, steps, cols, true, true, &sc->inv_s, who));
  SH_TRY(mod_prepare(c, modulus, g1b, steps, cols, false, false, &sc->fwd_s, who));
  sc->pm2 = ms_pm2(M);
  sc->degree = degree;
  sc->total_terms = total;
  sc->stride = stark_header_len(n, width, samples) + fri_proof_len(n, steps * (uint64_t)degree, 40);
  if (sc->stride / 32 > (0x7fffffffull * MS_WG) / batch)  // the gather launches one thread per 32-byte slot, on a one-dimensional grid
    return refuse(c, who, SH_ERR_UNSUPPORTED, "samples * batch gives proofs of 2^39 32-byte values or more in one call");
  return SH_OK;
}

}  // namespace

namespace shk {
// Parse + upload the step polynomials' terms and their partial derivatives over M (skipped when equal to the previous generic call's)
int mod_stark_terms(sh_ctx* c, const fpm_mod& M, uint32_t width, const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts,
                    uint64_t total) {
  std::vector<uint8_t> key(reinterpret_cast<const uint8_t*>(M.p), reinterpret_cast<const uint8_t*>(M.p) + 32);
  key.push_back((uint8_t)width);
  key.insert(key.end(), reinterpret_cast<const uint8_t*>(counts), reinterpret_cast<const uint8_t*>(counts + width));
  key.insert(key.end(), coefs, coefs + 32 * total);
  key.insert(key.end(), exps, exps + (size_t)width * total);
  if (c->mod_terms_dev && key == c->mod_terms_key) return SH_OK;
  std::vector<uint8_t> img(ModTermLayout::total, 0);
  fpm* cf = reinterpret_cast<fpm*>(img.data() + ModTermLayout::coef);
  fpm* dcf = reinterpret_cast<fpm*>(img.data() + ModTermLayout::dcoef);
  uint8_t* ex = img.data() + ModTermLayout::exps;
  uint8_t* dex = img.data() + ModTermLayout::dexps;
  uint32_t* dbeg = reinterpret_cast<uint32_t*>(img.data() + ModTermLayout::dbegin);
  uint32_t begin[SHK_STARK_MAX_WIDTH + 1] = {0};
  ms_terms_build(M, width, coefs, exps, counts, total, cf, dcf, ex, dex, dbeg, begin);
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // earlier launches may still read the old terms
  if (!c->mod_terms_dev) HIP_TRY(c, hipMalloc(&c->mod_terms_dev, ModTermLayout::total));
  HIP_TRY(c, hipMemcpy(c->mod_terms_dev, img.data(), ModTermLayout::total, hipMemcpyHostToDevice));
  memcpy(c->mod_terms_begin, begin, sizeof begin);
  c->mod_terms_key.swap(key);
  return SH_OK;
}
}  // namespace shk

namespace {
// the domain tables of (p, steps, ext) -- inv_z2 | fz | xpow, 3 n elements shared by every proof --: a plan like any other, in the
// byte-budgeted cache.  scratch = 2 n elements that nothing queued still reads.
int mod_stark_tables(sh_ctx* c, const ModStarkCall& sc, const fpm* tw, uint64_t steps, uint32_t ext, const fpm& x_last, fpm* scratch,
                     const fpm** out) {
  const fpm_mod& M = sc.fwd_n.M;
  const uint64_t n = steps * ext;
  std::string key("mst:");
  key.append(reinterpret_cast<const char*>(M.p), 32);
  key += std::to_string(steps) + ":" + std::to_string(ext);
  if (const NttPlan* hit = plan_find(c, key)) {
    *out = reinterpret_cast<const fpm*>(hit->owned[0]);
    return SH_OK;
  }
  PlanHolder holder;  // frees the table on every exit before plan_commit
  holder.p->n = n;
  holder.p->log_n = sc.fwd_n.log_n;
  void* d = nullptr;
  SH_TRY(plan_alloc(c, holder.p, (size_t)3 * n * sizeof(fpm), &d));
  MsTables t;
  memset(&t, 0, sizeof t);
  t.den = scratch;
  t.table = reinterpret_cast<fpm*>(d);
  t.tw = tw;
  t.n = n;
  t.steps = steps;
  t.ext = ext;
  t.log_n = (uint32_t)sc.fwd_n.log_n;
  t.x_last = x_last;
  const hipError_t e = shk_ms_tables(t, sc.pm2, M, c->stream);
  if (e != hipSuccess) {  // never cache a table whose fill did not launch
    c->err = std::string("generic STARK domain tables: ") + hipGetErrorString(e);
    return SH_ERR_HIP;
  }
  plan_commit(c, key, &holder);
  *out = t.table;
  return SH_OK;
}

int run_mod_stark(sh_ctx* c, const ModStarkCall& sc, fpm* d_wit, const fpm* d_inputs, uint64_t steps, uint32_t ext, uint32_t width,
                  uint32_t samples, uint32_t batch, uint8_t* d_proof) {
  const fpm_mod& M = sc.fwd_n.M;
  const uint64_t n = steps * ext, cols = (uint64_t)batch * width;
  const fpm *tw_n = nullptr, *tw_is = nullptr, *tw_fs = nullptr;
  SH_TRY(mod_table(c, sc.fwd_n, &tw_n));
  SH_TRY(mod_table(c, sc.inv_s, &tw_is));
  SH_TRY(mod_table(c, sc.fwd_s, &tw_fs));
  const fpm one = fpm_from_words(M.one);
  const fpm g1 = fpm_pow(sc.g2, ext, M);
  const fpm x_last = fpm_pow(sc.g2, (steps - 1) * ext, M);               // stark.py:212
  const fpm inv_last_m1 = fpm_pow_limbs(fpm_sub(x_last, one, M), sc.pm2.v, M);  // Fermat: the modulus is prime by contract
  const fpm cpow = fpm_pow(fpm_pow(sc.g2, steps, M), n - 1, M);          // `powers[i]` after the loop (stark.py:150-158)

  void *pe, *dw, *bw, *qv, *small, *mt;
  SH_TRY(ws_get(c, sh_ctx::WS_ST_P, (cols > 2 ? cols : 2) * n * sizeof(fpm), &pe));  // also the table build's 2 n of scratch
  SH_TRY(ws_get(c, sh_ctx::WS_ST_D, cols * n * sizeof(fpm), &dw));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_B, cols * n * sizeof(fpm), &bw));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_Q, cols * steps * sizeof(fpm), &qv));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_MTREE, (size_t)batch * 2 * n * 32, &mt));
  const size_t iab_bytes = cols * 2 * sizeof(fpm), scal_bytes = cols * 3 * sizeof(fpm);
  SH_TRY(ws_get(c, sh_ctx::WS_ST_SMALL, iab_bytes + scal_bytes + (size_t)batch * samples * 4, &small));
  fpm* iab = reinterpret_cast<fpm*>(small);
  fpm* scal = reinterpret_cast<fpm*>(reinterpret_cast<uint8_t*>(small) + iab_bytes);
  uint32_t* ys = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(small) + iab_bytes + scal_bytes);
  SH_TRY(bad_flags(c, batch));
  fpm* P = reinterpret_cast<fpm*>(pe);
  fpm* Q = reinterpret_cast<fpm*>(qv);
  const fpm* tables = nullptr;
  SH_TRY(mod_stark_tables(c, sc, tw_n, steps, ext, x_last, P, &tables));

  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->mod_terms_dev);
  MsArgs a;
  memset(&a, 0, sizeof a);
  a.p_evals = P;
  a.d_work = reinterpret_cast<fpm*>(dw);
  a.b_work = reinterpret_cast<fpm*>(bw);
  a.q_evals = Q;
  a.wit = d_wit;
  a.inputs = d_inputs;
  a.iab = iab;
  a.n = n;
  a.steps = steps;
  a.ext = ext;
  a.width = width;
  a.batch = batch;
  a.log_n = (uint32_t)sc.fwd_n.log_n;
  a.tw = tw_n;
  a.inv_z2 = tables;
  a.fz = tables + n;
  a.xpow = tables + 2 * n;
  a.x_last = x_last;
  a.g1 = g1;
  a.inv_last_m1 = inv_last_m1;
  a.inv_1_m_last = fpm_neg(inv_last_m1, M);
  a.inv_steps = sc.inv_s.scale;  // 1 / steps, plain: the inverse transform's own factor
  a.bad = c->bad_flag;
  a.term_coef = reinterpret_cast<const fpm*>(tb + ModTermLayout::coef);
  a.term_exps = tb + ModTermLayout::exps;
  memcpy(a.term_begin, c->mod_terms_begin, sizeof a.term_begin);
  a.dterm_coef = reinterpret_cast<const fpm*>(tb + ModTermLayout::dcoef);
  a.dterm_exps = tb + ModTermLayout::dexps;
  a.dterm_begin = reinterpret_cast<const uint32_t*>(tb + ModTermLayout::dbegin);

  // boundary interpolants need witness[dim][-1] (stark.py:91-96)
  HIP_TRY(c, shk_ms_interp(a, M, c->stream));
  // trace polynomials and their evaluations: the low-degree extension (stark.py:27-36, 253-256); the coefficients go to the Q buffer,
  // the witness stays what it is -- the trace polynomials' values on the trace points
  SH_TRY(mod_run(c, sc.inv_s, tw_is, d_wit, steps, Q, (uint32_t)cols, false, false));
  SH_TRY(mod_run(c, sc.fwd_n, tw_n, Q, steps, P, (uint32_t)cols, false, false));  // fft_1d's zero padding is implicit (fft.py:323-324)
  // Q = X P'(X) on the trace points, for the quotients' values there
  HIP_TRY(c, shk_ms_qprep(Q, Q, steps, cols, M, c->stream));
  SH_TRY(mod_run(c, sc.fwd_s, tw_fs, Q, steps, Q, (uint32_t)cols, false, false));
  // D = C / Z and B = (P - I) / Z2 (stark.py:38-104) on the whole domain, and
  // mtree = merkelize_polynomial_evaluations(width, P + D + B evaluations) (stark.py:257)
  uint32_t* mtree = reinterpret_cast<uint32_t*>(mt);
  HIP_TRY(c, shk_ms_quotients_and_merkelize(a, M, mtree, c->stream));
  // l = the pseudorandom linear combination keyed by mtree's root (stark.py:128-177, 259-263), on evaluations, and l_mtree
  FriBuffers fb;
  SH_TRY(fri_buffers(c, n, batch, samples, &fb));
  fpm* l = reinterpret_cast<fpm*>(fb.vals);
  HIP_TRY(c, shk_ms_scalars(mtree, 2 * n * 8, width, batch, cpow, scal, M, c->stream));
  HIP_TRY(c, shk_ms_lincomb(a, scal, l, M, c->stream));
  MfTree lt = {l, fb.tree, n, batch, 0};
  HIP_TRY(c, shk_mf_leaves(lt, c->stream));
  HIP_TRY(c, shk_merkle_upper_levels(n, batch, fb.tree, c->stream));
  // spot checks (stark.py:390-402)
  HIP_TRY(c, shk_sample_indices(fb.tree, 2 * n * 8, (uint32_t)n, batch, samples, ext, ys, c->stream));
  MsGather ga;
  memset(&ga, 0, sizeof ga);
  ga.mnodes = mtree;
  ga.lnodes = fb.tree;
  ga.lvals = l;
  ga.ys = ys;
  ga.samples = samples;
  ga.lg = (uint32_t)sc.fwd_n.log_n;
  ga.proof = d_proof;
  ga.stride = sc.stride;
  HIP_TRY(c, shk_ms_gather(a, ga, c->stream));
  // fri.generate_proximity_proof(l_poly, G2, steps * degree, exclude_multiples_of=ext) (stark.py:271-276); its first tree is l_mtree
  return modfri_rounds(c, sc.fwd_n, tw_n, fb, n, steps * (uint64_t)sc.degree, ext, 40, batch,
                       d_proof + stark_header_len(n, width, samples), sc.stride, true);
}

// ---- AIR.generate_witness (air.py:32-52, 121-123) over any odd modulus: modwitness.hip, launched in slices of steps ---------------------
// every host check of a witness call but the null pointers; on SH_OK M holds the modulus block and *total the number of terms
int mod_witness_check(sh_ctx* c, const char* who, const uint8_t modulus[32], uint64_t steps, uint32_t width, const uint32_t* counts,
                      uint32_t batch, fpm_mod* M, uint64_t* total) {
  if (!fpm_mod_init(modulus, M)) return refuse(c, who, SH_ERR_INVALID, "the modulus must be odd and at least 3");
  if (steps == 0 || width == 0 || batch == 0) return refuse(c, who, SH_ERR_INVALID, "steps, width and batch must be at least 1");
  if (width > SHK_STARK_MAX_WIDTH) return refuse(c, who, SH_ERR_UNSUPPORTED, "width is limited to 9 (stark.py:106-126)");
  *total = 0;
  for (uint32_t d = 0; d < width; ++d) *total += counts[d];
  if (*total == 0) return refuse(c, who, SH_ERR_INVALID, "the step polynomials have no terms");
  if (*total > SHK_STARK_MAX_TERMS) return refuse(c, who, SH_ERR_UNSUPPORTED, "more step-polynomial terms than SHK_STARK_MAX_TERMS");
  const uint64_t cols = (uint64_t)batch * width;
  if (cols > 0xffffffffull || steps > (~0ull / 32) / cols)
    return refuse(c, who, SH_ERR_UNSUPPORTED, "batch * width must be below 2^32 and the witness's byte count must fit 64 bits");
  return SH_OK;
}

// d_wit [batch][width][steps], plain and canonical, from d_in [batch][width]; the terms are the ones mod_stark_terms just uploaded.
// The plan comes from the caller's term bytes: a coefficient counts as 1 when it is 1 modulo p, as the kernel derives it from the image.
int run_mod_witness(sh_ctx* c, const fpm_mod& M, const fpm* d_in, fpm* d_wit, uint64_t steps, uint32_t width, const uint8_t* coefs,
                    const uint8_t* exps, const uint32_t* counts, uint32_t batch) {
  WiRow rows[SHK_STARK_MAX_TERMS];
  uint32_t T = 0;
  for (uint32_t d = 0; d < width; ++d)
    for (uint32_t i = 0; i < counts[d]; ++i, ++T)
      rows[T] = wi_pack_row(d, mwi_unit(fpm_to_mont(fpm_from_wire_bytes(coefs + 32ull * T), M), M), exps + (size_t)T * width, width);
  ModWitnessArgs a;
  memset(&a, 0, sizeof a);
  mwi_plan(rows, T, width, (uint32_t)shk_knobs().witness_group, (uint64_t)shk_knobs().witness_slice, &a.plan);
  const bool inl = shk_knobs().witness_inline;
  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->mod_terms_dev);
  a.inputs = d_in;
  a.wit = d_wit;
  a.steps = steps;
  a.batch = batch;
  a.nterms = T;
  a.coef = reinterpret_cast<const fpm*>(tb + ModTermLayout::coef);
  a.exps = tb + ModTermLayout::exps;
  memcpy(a.begin, c->mod_terms_begin, sizeof a.begin);
  for (a.k0 = 0; a.k0 < steps; a.k0 = a.k1) {  // each dispatch resumes from the last row the previous one wrote
    a.k1 = steps - a.k0 > a.plan.slice ? a.k0 + a.plan.slice : steps;
    HIP_TRY(c, shk_mod_witness_slice(a, M, width, inl, c->stream));
  }
  if (!inl) HIP_TRY(c, shk_mod_witness_finish(d_wit, (uint64_t)batch * width * steps, M, c->stream));
  return SH_OK;
}
}  // namespace

extern "C" {

int sh_dev_mod_stark_prove(sh_ctx* c, const uint8_t modulus[32], void* d_witness, const void* d_inputs, uint64_t steps, uint32_t ext,
                           uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts,
                           uint32_t samples, uint32_t batch, void* d_proof) {
  const char* who = "sh_dev_mod_stark_prove";
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !d_witness || !d_inputs || !term_coefs || !term_exps || !term_counts || !d_proof)
    return refuse(c, who, SH_ERR_INVALID, "null pointer");
  ModStarkCall sc;
  SH_TRY(mod_stark_check(c, who, modulus, steps, ext, width, term_exps, term_counts, samples, batch, &sc));
  SH_TRY(enter(c));
  SH_TRY(mod_stark_terms(c, sc.fwd_n.M, width, term_coefs, term_exps, term_counts, sc.total_terms));
  return run_mod_stark(c, sc, reinterpret_cast<fpm*>(d_witness), reinterpret_cast<const fpm*>(d_inputs), steps, ext, width, samples, batch,
                       reinterpret_cast<uint8_t*>(d_proof));
}

int sh_mod_stark_prove(sh_ctx* c, const uint8_t modulus[32], const uint8_t* witness, const uint8_t* inputs, uint64_t steps, uint32_t ext,
                       uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts, uint32_t samples,
                       uint32_t batch, uint8_t* proof, uint64_t proof_cap) {
  const char* who = "sh_mod_stark_prove";
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !witness || !inputs || !term_coefs || !term_exps || !term_counts || !proof)
    return refuse(c, who, SH_ERR_INVALID, "null pointer");
  ModStarkCall sc;
  SH_TRY(mod_stark_check(c, who, modulus, steps, ext, width, term_exps, term_counts, samples, batch, &sc));
  if (proof_cap / sc.stride < batch) return refuse(c, who, SH_ERR_TOO_SMALL, "proof_cap is below batch * sh_stark_proof_len(steps, ext, width, degree, samples)");
  SH_TRY(enter(c));
  SH_TRY(mod_stark_terms(c, sc.fwd_n.M, width, term_coefs, term_exps, term_counts, sc.total_terms));
  // wire form -> limbs is a byte reversal per value; nothing is reduced here (the kernels take any 256-bit value modulo p)
  const uint64_t cols = (uint64_t)batch * width, wn = cols * steps;
  std::vector<uint8_t> limbs((size_t)(wn + cols) * 32);
  for (uint64_t i = 0; i < wn + cols; ++i) {
    const uint8_t* src = i < wn ? witness + 32 * i : inputs + 32 * (i - wn);
    for (int k = 0; k < 32; ++k) limbs[32 * i + k] = src[31 - k];
  }
  void *w = nullptr, *dp = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_ST_TRACE, limbs.size(), &w));
  SH_TRY(ws_get(c, sh_ctx::WS_PROOF, (size_t)sc.stride * batch, &dp));
  SH_TRY(h2d(c, w, limbs.data(), limbs.size()));
  // this call reports on its own witnesses only: flags left by unchecked device-form calls are dropped
  if (c->bad_flag) HIP_TRY(c, hipMemsetAsync(c->bad_flag, 0, (size_t)c->bad_cap * 4, c->stream));
  fpm* dwit = reinterpret_cast<fpm*>(w);
  SH_TRY(run_mod_stark(c, sc, dwit, dwit + wn, steps, ext, width, samples, batch, reinterpret_cast<uint8_t*>(dp)));
  SH_TRY(d2h(c, proof, dp, (size_t)sc.stride * batch));
  return sh_stark_status(c);
}

int sh_dev_mod_stark_witness(sh_ctx* c, const uint8_t modulus[32], const void* d_inputs, uint64_t steps, uint32_t width,
                             const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts, uint32_t batch,
                             void* d_witness) {
  const char* who = "sh_dev_mod_stark_witness";
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !d_inputs || !term_coefs || !term_exps || !term_counts || !d_witness) return refuse(c, who, SH_ERR_INVALID, "null pointer");
  fpm_mod M;
  uint64_t total = 0;
  SH_TRY(mod_witness_check(c, who, modulus, steps, width, term_counts, batch, &M, &total));
  if (any_overlap(d_inputs, 32ull * batch * width, d_witness, 32ull * batch * width * steps))
    return refuse(c, who, SH_ERR_INVALID, "d_inputs and d_witness overlap");
  SH_TRY(enter(c));
  SH_TRY(mod_stark_terms(c, M, width, term_coefs, term_exps, term_counts, total));
  return run_mod_witness(c, M, reinterpret_cast<const fpm*>(d_inputs), reinterpret_cast<fpm*>(d_witness), steps, width, term_coefs,
                         term_exps, term_counts, batch);
}

int sh_mod_stark_witness(sh_ctx* c, const uint8_t modulus[32], const uint8_t* inputs, uint64_t steps, uint32_t width,
                         const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts, uint32_t batch, uint8_t* witness,
                         uint64_t witness_cap) {
  const char* who = "sh_mod_stark_witness";
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !inputs || !term_coefs || !term_exps || !term_counts || !witness) return refuse(c, who, SH_ERR_INVALID, "null pointer");
  fpm_mod M;
  uint64_t total = 0;
  SH_TRY(mod_witness_check(c, who, modulus, steps, width, term_counts, batch, &M, &total));
  const uint64_t cols = (uint64_t)batch * width, count = cols * steps;
  if (witness_cap / 32 < count) return refuse(c, who, SH_ERR_TOO_SMALL, "witness_cap is below 32 * batch * width * steps");
  SH_TRY(enter(c));
  SH_TRY(mod_stark_terms(c, M, width, term_coefs, term_exps, term_counts, total));
  // wire form <-> limbs is a byte reversal per value; nothing is reduced on the host (row 0 reduces an input >= p on the device)
  std::vector<uint8_t> limbs((size_t)cols * 32);
  for (uint64_t i = 0; i < cols; ++i)
    for (int k = 0; k < 32; ++k) limbs[32 * i + k] = inputs[32 * i + 31 - k];
  void *in = nullptr, *w = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_Y, limbs.size(), &in));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_TRACE, (size_t)count * sizeof(fpm), &w));
  SH_TRY(h2d(c, in, limbs.data(), limbs.size()));
  SH_TRY(run_mod_witness(c, M, reinterpret_cast<const fpm*>(in), reinterpret_cast<fpm*>(w), steps, width, term_coefs, term_exps,
                         term_counts, batch));
  SH_TRY(d2h(c, witness, w, (size_t)count * 32));
  for (uint64_t i = 0; i < count; ++i)
    for (int k = 0; k < 16; ++k) std::swap(witness[32 * i + k], witness[32 * i + 31 - k]);
  return SH_OK;
}
}  // extern "C"
