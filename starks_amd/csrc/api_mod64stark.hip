// api_mod64stark.hip -- STARK.mk_proof (stark.py:233-279) over any prime modulus below 2^64 on packed 64-bit words, on the host side, and
// its entry points: run_mod_stark's sequence (api_modstark.hip) with 8 bytes per value from the first kernel to the gather.  The
// transforms are api_ntt64.hip's, the middle of the prover mod64stark.hip's, the commit rounds api_mod64fri.hip's (mod64fri_rounds, on the
// evaluations and the tree built here), the tree levels above the leaf kernels and the index sampler the MiMC path's (kernels.hip).
// The proof bytes are sh_mod_stark_prove's over the same modulus on the same values.  Every check runs on the host before anything is
// launched.
// Also AIR.generate_witness on packed words over any odd modulus below 2^64 (sh_mod64_stark_witness, sh_dev_mod64_stark_witness:
// mod64witness.hip launched in slices), through the same term image and key: generate -> prove over one system uploads once.
#include "ctx.hpp"
#include "mod64stark_items.cuh"
using namespace shk;

namespace {
// everything the host derives from the arguments before a launch
struct Mod64StarkCall {
  Mod64Call fwd_n, inv_s, fwd_s;  // the n-point transform over G2, the steps-point inverse and forward transforms over G1
  uint64_t g2;                    // Montgomery form
  uint32_t degree;
  uint64_t total_terms;
  uint64_t stride;                // bytes of one proof
};

int refuse(sh_ctx* c, const char* who, int rc, const char* why) {
  c->err = std::string(who) + ": " + why;
  return rc;
}

// every host check of a proof; on SH_OK sc holds the call's constants.  Nothing here touches the device.
int mod64_stark_check(sh_ctx* c, const char* who, uint64_t modulus, uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* exps,
                      const uint32_t* counts, uint32_t samples, uint32_t batch, Mod64StarkCall* sc) {
  f64_mod M;
  if (!f64_mod_init(modulus, &M)) return refuse(c, who, SH_ERR_INVALID, "the modulus must be odd and at least 3");
  if (width == 0 || batch == 0) return refuse(c, who, SH_ERR_INVALID, "width and batch must be at least 1");
  if (width > SHK_STARK_MAX_WIDTH) return refuse(c, who, SH_ERR_UNSUPPORTED, "width is limited to 9 (stark.py:106-126)");
  if (batch > 65535) return refuse(c, who, SH_ERR_UNSUPPORTED, "a call takes at most 65535 proofs");
  uint64_t total = 0;
  for (uint32_t d = 0; d < width; ++d) total += counts[d];
  if (total == 0) return refuse(c, who, SH_ERR_INVALID, "the step polynomials have no terms");
  if (total > SHK_STARK_MAX_TERMS) return refuse(c, who, SH_ERR_UNSUPPORTED, "more step-polynomial terms than SHK_STARK_MAX_TERMS");
  const uint32_t degree = m6s_terms_degree(exps, width, total);
  const int rc = stark_check_shape(steps, ext, width, degree, samples);
  if (rc != SH_OK)
    return refuse(c, who, rc,
                  "steps and ext must be powers of two >= 2 with steps * ext < 2^24, degree * (steps - 1) + 1 < steps * ext, samples >= 1, "
                  "and the commit of steps * degree coefficients on steps * ext points must be one sh_mod64_fri_prove accepts");
  const uint64_t n = steps * ext, cols = (uint64_t)batch * width;
  sc->g2 = m6s_g2(M, ilog2(n));  // 7^((p - 1) // (steps * ext)) (stark.py:205)
  const uint64_t g2 = f64_from_mont(sc->g2, M), g1 = f64_from_mont(f64_pow(sc->g2, ext, M), M);
  const int rr = mod64_prepare(c, modulus, g2, n, cols, false, false, &sc->fwd_n, who);
  if (rr == SH_ERR_ROOT_ORDER)
    return refuse(c, who, rr, "G2 = 7^((p - 1) // (steps * ext)) does not have order steps * ext modulo p (G2^(n/2) != -1)");
  SH_TRY(rr);
  SH_TRY(mod64_prepare(c, modulus, g1, steps, cols, true, true, &sc->inv_s, who));
  SH_TRY(mod64_prepare(c, modulus, g1, steps, cols, false, false, &sc->fwd_s, who));
  sc->degree = degree;
  sc->total_terms = total;
  sc->stride = stark_header_len(n, width, samples) + fri_proof_len(n, steps * (uint64_t)degree, 40);
  if (sc->stride / 32 > (0x7fffffffull * M6S_WG) / batch)  // the gather launches one thread per 32-byte slot, on a one-dimensional grid
    return refuse(c, who, SH_ERR_UNSUPPORTED, "samples * batch gives proofs of 2^39 32-byte values or more in one call");
  return SH_OK;
}

// Parse + upload the step polynomials' terms and their partial derivatives over M as words (skipped when equal to the previous packed
// call's).  The image and its key are the packed prover's own: the generic prover's (mod_terms_dev) is neither read nor written.
int mod64_stark_terms(sh_ctx* c, const f64_mod& M, uint32_t width, const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts,
                      uint64_t total) {
  std::vector<uint8_t> key(reinterpret_cast<const uint8_t*>(&M.p), reinterpret_cast<const uint8_t*>(&M.p) + 8);
  key.push_back((uint8_t)width);
  key.insert(key.end(), reinterpret_cast<const uint8_t*>(counts), reinterpret_cast<const uint8_t*>(counts + width));
  key.insert(key.end(), coefs, coefs + 32 * total);
  key.insert(key.end(), exps, exps + (size_t)width * total);
  if (c->mod64_terms_dev && key == c->mod64_terms_key) return SH_OK;
  std::vector<uint8_t> img(Mod64TermLayout::total, 0);
  uint64_t* cf = reinterpret_cast<uint64_t*>(img.data() + Mod64TermLayout::coef);
  uint64_t* dcf = reinterpret_cast<uint64_t*>(img.data() + Mod64TermLayout::dcoef);
  uint8_t* ex = img.data() + Mod64TermLayout::exps;
  uint8_t* dex = img.data() + Mod64TermLayout::dexps;
  uint32_t* dbeg = reinterpret_cast<uint32_t*>(img.data() + Mod64TermLayout::dbegin);
  uint32_t begin[SHK_STARK_MAX_WIDTH + 1] = {0};
  m6s_terms_build(M, width, coefs, exps, counts, total, cf, dcf, ex, dex, dbeg, begin);
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // earlier launches may still read the old terms
  if (!c->mod64_terms_dev) HIP_TRY(c, hipMalloc(&c->mod64_terms_dev, Mod64TermLayout::total));
  HIP_TRY(c, hipMemcpy(c->mod64_terms_dev, img.data(), Mod64TermLayout::total, hipMemcpyHostToDevice));
  memcpy(c->mod64_terms_begin, begin, sizeof begin);
  c->mod64_terms_key.swap(key);
  return SH_OK;
}

// the domain tables of (p, steps, ext) -- inv_z2 | fz | xpow, 3 n words shared by every proof --: a plan like any other, in the
// byte-budgeted cache.  The key opens with "m6st:", the 32-byte tables' with "mst:": the two never meet.  scratch = 2 n words that
// nothing queued still reads.
int mod64_stark_tables(sh_ctx* c, const Mod64StarkCall& sc, const uint64_t* tab, uint64_t steps, uint32_t ext, uint64_t x_last,
                       uint64_t* scratch, const uint64_t** out) {
  const f64_mod& M = sc.fwd_n.M;
  const uint64_t n = steps * ext;
  std::string key("m6st:");
  key.append(reinterpret_cast<const char*>(&M.p), 8);
  key += std::to_string(steps) + ":" + std::to_string(ext);
  if (const NttPlan* hit = plan_find(c, key)) {
    *out = reinterpret_cast<const uint64_t*>(hit->owned[0]);
    return SH_OK;
  }
  PlanHolder holder;  // frees the table on every exit before plan_commit
  holder.p->n = n;
  holder.p->log_n = sc.fwd_n.log_n;
  void* d = nullptr;
  SH_TRY(plan_alloc(c, holder.p, (size_t)3 * n * sizeof(uint64_t), &d));
  M6sTables t;
  memset(&t, 0, sizeof t);
  t.den = scratch;
  t.table = reinterpret_cast<uint64_t*>(d);
  t.log_h = (uint32_t)n64_log_h(sc.fwd_n.log_n);
  t.lo = tab;
  t.hi = tab + (1ull << t.log_h);
  t.n = n;
  t.steps = steps;
  t.ext = ext;
  t.x_last = x_last;
  const hipError_t e = shk_m6s_tables(t, M, c->stream);
  if (e != hipSuccess) {  // never cache a table whose fill did not launch
    c->err = std::string("packed-word STARK domain tables: ") + hipGetErrorString(e);
    return SH_ERR_HIP;
  }
  plan_commit(c, key, &holder);
  *out = t.table;
  return SH_OK;
}

int run_mod64_stark(sh_ctx* c, const Mod64StarkCall& sc, uint64_t* d_wit, const uint64_t* d_inputs, uint64_t steps, uint32_t ext,
                    uint32_t width, uint32_t samples, uint32_t batch, uint8_t* d_proof) {
  const f64_mod& M = sc.fwd_n.M;
  const uint64_t n = steps * ext, cols = (uint64_t)batch * width;
  const uint64_t *tab_n = nullptr, *tab_is = nullptr, *tab_fs = nullptr;
  SH_TRY(mod64_table(c, sc.fwd_n, &tab_n));
  SH_TRY(mod64_table(c, sc.inv_s, &tab_is));
  SH_TRY(mod64_table(c, sc.fwd_s, &tab_fs));
  const uint64_t g1 = f64_pow(sc.g2, ext, M);
  const uint64_t x_last = f64_pow(sc.g2, (steps - 1) * ext, M);                      // stark.py:212
  const uint64_t inv_last_m1 = f64_pow(f64_sub(x_last, M.one, M), M.p - 2, M);        // Fermat: the modulus is prime by contract
  const uint64_t cpow = f64_pow(f64_pow(sc.g2, steps, M), n - 1, M);                 // `powers[i]` after the loop (stark.py:150-158)

  void *pe, *dw, *bw, *qv, *small, *mt;
  SH_TRY(ws_get(c, sh_ctx::WS_ST_P, (cols > 2 ? cols : 2) * n * 8, &pe));  // also the table build's 2 n of scratch
  SH_TRY(ws_get(c, sh_ctx::WS_ST_D, cols * n * 8, &dw));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_B, cols * n * 8, &bw));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_Q, cols * steps * 8, &qv));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_MTREE, (size_t)batch * 2 * n * 32, &mt));
  const size_t iab_bytes = cols * 2 * 8, scal_bytes = cols * 3 * 8;
  SH_TRY(ws_get(c, sh_ctx::WS_ST_SMALL, iab_bytes + scal_bytes + (size_t)batch * samples * 4, &small));
  uint64_t* iab = reinterpret_cast<uint64_t*>(small);
  uint64_t* scal = reinterpret_cast<uint64_t*>(reinterpret_cast<uint8_t*>(small) + iab_bytes);
  uint32_t* ys = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(small) + iab_bytes + scal_bytes);
  SH_TRY(bad_flags(c, batch));
  uint64_t* P = reinterpret_cast<uint64_t*>(pe);
  uint64_t* Q = reinterpret_cast<uint64_t*>(qv);
  const uint64_t* tables = nullptr;
  SH_TRY(mod64_stark_tables(c, sc, tab_n, steps, ext, x_last, P, &tables));

  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->mod64_terms_dev);
  M6sArgs a;
  memset(&a, 0, sizeof a);
  a.p_evals = P;
  a.d_work = reinterpret_cast<uint64_t*>(dw);
  a.b_work = reinterpret_cast<uint64_t*>(bw);
  a.q_evals = Q;
  a.wit = d_wit;
  a.inputs = d_inputs;
  a.iab = iab;
  a.n = n;
  a.steps = steps;
  a.ext = ext;
  a.width = width;
  a.batch = batch;
  a.inv_z2 = tables;
  a.fz = tables + n;
  a.xpow = tables + 2 * n;
  a.x_last = x_last;
  a.g1 = g1;
  a.inv_last_m1 = inv_last_m1;
  a.inv_1_m_last = f64_neg(inv_last_m1, M);
  a.inv_steps = sc.inv_s.scale;  // 1 / steps, plain: the inverse transform's own factor
  a.bad = c->bad_flag;
  a.term_coef = reinterpret_cast<const uint64_t*>(tb + Mod64TermLayout::coef);
  a.term_exps = tb + Mod64TermLayout::exps;
  memcpy(a.term_begin, c->mod64_terms_begin, sizeof a.term_begin);
  a.dterm_coef = reinterpret_cast<const uint64_t*>(tb + Mod64TermLayout::dcoef);
  a.dterm_exps = tb + Mod64TermLayout::dexps;
  a.dterm_begin = reinterpret_cast<const uint32_t*>(tb + Mod64TermLayout::dbegin);

  // boundary interpolants need witness[dim][-1] (stark.py:91-96)
  HIP_TRY(c, shk_m6s_interp(a, M, c->stream));
  // trace polynomials and their evaluations: the low-degree extension (stark.py:27-36, 253-256); the coefficients go to the Q buffer,
  // the witness stays what it is -- the trace polynomials' values on the trace points
  SH_TRY(mod64_run(c, sc.inv_s, tab_is, d_wit, steps, Q, (uint32_t)cols));
  SH_TRY(mod64_run(c, sc.fwd_n, tab_n, Q, steps, P, (uint32_t)cols));  // fft_1d's zero padding is implicit (fft.py:323-324)
  // Q = X P'(X) on the trace points, for the quotients' values there
  HIP_TRY(c, shk_m6s_qprep(Q, Q, steps, cols, M, c->stream));
  SH_TRY(mod64_run(c, sc.fwd_s, tab_fs, Q, steps, Q, (uint32_t)cols));
  // D = C / Z and B = (P - I) / Z2 (stark.py:38-104) on the whole domain, and
  // mtree = merkelize_polynomial_evaluations(width, P + D + B evaluations) (stark.py:257)
  uint32_t* mtree = reinterpret_cast<uint32_t*>(mt);
  HIP_TRY(c, shk_m6s_quotients_and_merkelize(a, M, mtree, c->stream));
  // l = the pseudorandom linear combination keyed by mtree's root (stark.py:128-177, 259-263), on evaluations, and l_mtree
  Fri64Buffers fb;
  SH_TRY(mod64fri_buffers(c, n, batch, samples, &fb));
  uint64_t* l = fb.vals;
  HIP_TRY(c, shk_m6s_scalars(mtree, 2 * n * 8, width, batch, cpow, scal, M, c->stream));
  HIP_TRY(c, shk_m6s_lincomb(a, scal, l, M, c->stream));
  M6Tree lt = {l, fb.tree, n, batch, 0};
  HIP_TRY(c, shk_m6_leaves(lt, c->stream));
  HIP_TRY(c, shk_merkle_upper_levels(n, batch, fb.tree, c->stream));
  // spot checks (stark.py:390-402)
  HIP_TRY(c, shk_sample_indices(fb.tree, 2 * n * 8, (uint32_t)n, batch, samples, ext, ys, c->stream));
  M6sGather ga;
  memset(&ga, 0, sizeof ga);
  ga.mnodes = mtree;
  ga.lnodes = fb.tree;
  ga.lvals = l;
  ga.ys = ys;
  ga.samples = samples;
  ga.lg = (uint32_t)sc.fwd_n.log_n;
  ga.proof = d_proof;
  ga.stride = sc.stride;
  HIP_TRY(c, shk_m6s_gather(a, ga, c->stream));
  // fri.generate_proximity_proof(l_poly, G2, steps * degree, exclude_multiples_of=ext) (stark.py:271-276); its first tree is l_mtree
  return mod64fri_rounds(c, sc.fwd_n, tab_n, fb, n, steps * (uint64_t)sc.degree, ext, 40, batch,
                         d_proof + stark_header_len(n, width, samples), sc.stride, true);
}

// ---- AIR.generate_witness (air.py:32-52, 121-123) on packed words: mod64witness.hip, launched in slices of steps ------------------------
// every host check of a witness call but the null pointers; on SH_OK M holds the modulus block and *total the number of terms
int mod64_witness_check(sh_ctx* c, const char* who, uint64_t modulus, uint64_t steps, uint32_t width, const uint32_t* counts,
                        uint32_t batch, f64_mod* M, uint64_t* total) {
  if (!f64_mod_init(modulus, M)) return refuse(c, who, SH_ERR_INVALID, "the modulus must be odd and at least 3");
  if (steps == 0 || width == 0 || batch == 0) return refuse(c, who, SH_ERR_INVALID, "steps, width and batch must be at least 1");
  if (width > SHK_STARK_MAX_WIDTH) return refuse(c, who, SH_ERR_UNSUPPORTED, "width is limited to 9 (stark.py:106-126)");
  *total = 0;
  for (uint32_t d = 0; d < width; ++d) *total += counts[d];
  if (*total == 0) return refuse(c, who, SH_ERR_INVALID, "the step polynomials have no terms");
  if (*total > SHK_STARK_MAX_TERMS) return refuse(c, who, SH_ERR_UNSUPPORTED, "more step-polynomial terms than SHK_STARK_MAX_TERMS");
  const uint64_t cols = (uint64_t)batch * width;
  if (cols > 0xffffffffull || steps > (~0ull / 8) / cols)
    return refuse(c, who, SH_ERR_UNSUPPORTED, "batch * width must be below 2^32 and the witness's byte count must fit 64 bits");
  return SH_OK;
}

// d_wit [batch][width][steps], plain canonical words, from d_in [batch][width]; the terms are the ones mod64_stark_terms just uploaded.
// The plan comes from the caller's term bytes: a coefficient counts as 1 when it is 1 modulo p, as the kernel derives it from the image.
int run_mod64_witness(sh_ctx* c, const f64_mod& M, const uint64_t* d_in, uint64_t* d_wit, uint64_t steps, uint32_t width,
                      const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts, uint32_t batch) {
  WiRow rows[SHK_STARK_MAX_TERMS];
  uint32_t T = 0;
  for (uint32_t d = 0; d < width; ++d)
    for (uint32_t i = 0; i < counts[d]; ++i, ++T)
      rows[T] = wi_pack_row(d, m6w_unit(f64_to_mont(m6s_from_wire(coefs + 32ull * T, M), M), M), exps + (size_t)T * width, width);
  Mod64WitnessArgs a;
  memset(&a, 0, sizeof a);
  m6w_plan(rows, T, width, (uint32_t)shk_knobs().witness_group, (uint64_t)shk_knobs().witness_slice, &a.plan);
  const bool inl = shk_knobs().witness_inline;
  const uint8_t* tb = reinterpret_cast<const uint8_t*>(c->mod64_terms_dev);
  a.inputs = d_in;
  a.wit = d_wit;
  a.steps = steps;
  a.batch = batch;
  a.nterms = T;
  a.coef = reinterpret_cast<const uint64_t*>(tb + Mod64TermLayout::coef);
  a.exps = tb + Mod64TermLayout::exps;
  memcpy(a.begin, c->mod64_terms_begin, sizeof a.begin);
  for (a.k0 = 0; a.k0 < steps; a.k0 = a.k1) {  // each dispatch resumes from the last row the previous one wrote
    a.k1 = steps - a.k0 > a.plan.slice ? a.k0 + a.plan.slice : steps;
    HIP_TRY(c, shk_mod64_witness_slice(a, M, width, inl, c->stream));
  }
  if (!inl) HIP_TRY(c, shk_mod64_witness_finish(d_wit, (uint64_t)batch * width * steps, M, c->stream));
  return SH_OK;
}
}  // namespace

extern "C" {

int sh_dev_mod64_stark_prove(sh_ctx* c, uint64_t modulus, void* d_witness, const void* d_inputs, uint64_t steps, uint32_t ext,
                             uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts,
                             uint32_t samples, uint32_t batch, void* d_proof) {
  const char* who = "sh_dev_mod64_stark_prove";
  if (!c) return SH_ERR_INVALID;
  if (!d_witness || !d_inputs || !term_coefs || !term_exps || !term_counts || !d_proof) return refuse(c, who, SH_ERR_INVALID, "null pointer");
  Mod64StarkCall sc;
  SH_TRY(mod64_stark_check(c, who, modulus, steps, ext, width, term_exps, term_counts, samples, batch, &sc));
  SH_TRY(enter(c));
  SH_TRY(mod64_stark_terms(c, sc.fwd_n.M, width, term_coefs, term_exps, term_counts, sc.total_terms));
  return run_mod64_stark(c, sc, reinterpret_cast<uint64_t*>(d_witness), reinterpret_cast<const uint64_t*>(d_inputs), steps, ext, width,
                         samples, batch, reinterpret_cast<uint8_t*>(d_proof));
}

int sh_mod64_stark_prove(sh_ctx* c, uint64_t modulus, const uint64_t* witness, const uint64_t* inputs, uint64_t steps, uint32_t ext,
                         uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts,
                         uint32_t samples, uint32_t batch, uint8_t* proof, uint64_t proof_cap) {
  const char* who = "sh_mod64_stark_prove";
  if (!c) return SH_ERR_INVALID;
  if (!witness || !inputs || !term_coefs || !term_exps || !term_counts || !proof) return refuse(c, who, SH_ERR_INVALID, "null pointer");
  Mod64StarkCall sc;
  SH_TRY(mod64_stark_check(c, who, modulus, steps, ext, width, term_exps, term_counts, samples, batch, &sc));
  if (proof_cap / sc.stride < batch)
    return refuse(c, who, SH_ERR_TOO_SMALL, "proof_cap is below batch * sh_stark_proof_len(steps, ext, width, degree, samples)");
  SH_TRY(enter(c));
  SH_TRY(mod64_stark_terms(c, sc.fwd_n.M, width, term_coefs, term_exps, term_counts, sc.total_terms));
  // the words go up as they are: nothing is reduced here (the kernels take any 64-bit word modulo p)
  const uint64_t cols = (uint64_t)batch * width, wn = cols * steps;
  void *w = nullptr, *dp = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_ST_TRACE, (size_t)(wn + cols) * 8, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_PROOF, (size_t)sc.stride * batch, &dp));
  uint64_t* dwit = reinterpret_cast<uint64_t*>(w);
  SH_TRY(h2d(c, dwit, witness, (size_t)wn * 8));
  SH_TRY(h2d(c, dwit + wn, inputs, (size_t)cols * 8));
  // this call reports on its own witnesses only: flags left by unchecked device-form calls are dropped
  if (c->bad_flag) HIP_TRY(c, hipMemsetAsync(c->bad_flag, 0, (size_t)c->bad_cap * 4, c->stream));
  SH_TRY(run_mod64_stark(c, sc, dwit, dwit + wn, steps, ext, width, samples, batch, reinterpret_cast<uint8_t*>(dp)));
  SH_TRY(d2h(c, proof, dp, (size_t)sc.stride * batch));
  return sh_stark_status(c);
}

int sh_dev_mod64_stark_witness(sh_ctx* c, uint64_t modulus, const void* d_inputs, uint64_t steps, uint32_t width,
                               const uint8_t* term_coefs, const uint8_t* term_exps, const uint32_t* term_counts, uint32_t batch,
                               void* d_witness) {
  const char* who = "sh_dev_mod64_stark_witness";
  if (!c) return SH_ERR_INVALID;
  if (!d_inputs || !term_coefs || !term_exps || !term_counts || !d_witness) return refuse(c, who, SH_ERR_INVALID, "null pointer");
  f64_mod M;
  uint64_t total = 0;
  SH_TRY(mod64_witness_check(c, who, modulus, steps, width, term_counts, batch, &M, &total));
  if (any_overlap(d_inputs, 8ull * batch * width, d_witness, 8ull * batch * width * steps))
    return refuse(c, who, SH_ERR_INVALID, "d_inputs and d_witness overlap");
  SH_TRY(enter(c));
  SH_TRY(mod64_stark_terms(c, M, width, term_coefs, term_exps, term_counts, total));
  return run_mod64_witness(c, M, reinterpret_cast<const uint64_t*>(d_inputs), reinterpret_cast<uint64_t*>(d_witness), steps, width,
                           term_coefs, term_exps, term_counts, batch);
}

int sh_mod64_stark_witness(sh_ctx* c, uint64_t modulus, const uint64_t* inputs, uint64_t steps, uint32_t width, const uint8_t* term_coefs,
                           const uint8_t* term_exps, const uint32_t* term_counts, uint32_t batch, uint64_t* witness,
                           uint64_t witness_cap) {
  const char* who = "sh_mod64_stark_witness";
  if (!c) return SH_ERR_INVALID;
  if (!inputs || !term_coefs || !term_exps || !term_counts || !witness) return refuse(c, who, SH_ERR_INVALID, "null pointer");
  f64_mod M;
  uint64_t total = 0;
  SH_TRY(mod64_witness_check(c, who, modulus, steps, width, term_counts, batch, &M, &total));
  const uint64_t cols = (uint64_t)batch * width, count = cols * steps;
  if (witness_cap < count) return refuse(c, who, SH_ERR_TOO_SMALL, "witness_cap is below batch * width * steps words");
  SH_TRY(enter(c));
  SH_TRY(mod64_stark_terms(c, M, width, term_coefs, term_exps, term_counts, total));
  // the words go up as they are: row 0 reduces an input at or above p on the device
  void *in = nullptr, *w = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_Y, (size_t)cols * 8, &in));
  SH_TRY(ws_get(c, sh_ctx::WS_ST_TRACE, (size_t)count * 8, &w));
  SH_TRY(h2d(c, in, inputs, (size_t)cols * 8));
  SH_TRY(run_mod64_witness(c, M, reinterpret_cast<const uint64_t*>(in), reinterpret_cast<uint64_t*>(w), steps, width, term_coefs,
                           term_exps, term_counts, batch));
  return d2h(c, witness, w, (size_t)count * 8);
}
}  // extern "C"
