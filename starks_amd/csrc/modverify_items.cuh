// modverify_items.cuh -- the per-item checks of the batched FRI verifier over any odd modulus below 2^256 (modverify_dev.hip) and the
// host plan they run by: verify_items.cuh's decomposition on the run-time-modulus arithmetic of fpm.cuh.
//
// The field-free pieces are verify_items.cuh's own -- vb_branch, vb_hash_two, vb_final_leaf, vb_npts, vb_pt, the index sampler -- and
// every byte offset of a shape sits in a VbPlan (MvPlan::shape: its fp fields stay zero), so the index-set and branch kernels of
// verify_dev.hip run as they are.  What depends on the field is here: the row item, the two final-layer items and the plan's
// constants.  Everything is __host__ __device__: tests/native/modverify_host.cpp walks the same items on the CPU over the same plan
// and compares every decision with the host verifier's (modverify.hip), which shares none of this code.
//
// Forms.  A value read from a proof is any 256-bit number and is taken modulo p (mv_field: plain, canonical).  The plan's constants --
// generators, I^-1, the final layer's x_k, cofactors and D -- are in Montgomery form, so fpm_mul(plain, constant) is plain and
// canonical and two canonical plain values compare limb for limb.
//
// NO INVERSION, anywhere: p may be composite (root^(n/2) = -1 is all that is asked of it), where x^(p-2) is not an inverse.
//   row          the closed form of mf_fold_row / vb_fri_row: I^-1 = w^(3 n/4), the 1/4 is two halvings (p is odd).
//   final layer  the interpolant through the first k retained points, cross-multiplied.  With den_a = prod_{b != a} (x_a - x_b),
//                D = prod_a den_a and cof_a = D / den_a = prod_{c != a} den_c (a product, not a quotient), point t passes when
//                    sum_a data_a cof_a prod_{b != a} (x_t - x_b) == data_t D.
//                root^(n/2) = -1 modulo an odd p gives w order n modulo every prime factor of p, so every w^d - 1, 0 < d < n, and with
//                them every den_a and D are units: the check is the reference's data_t == sum_a data_a / den_a prod (x_t - x_b)
//                multiplied through by a unit, the same decision for every proof.
//
//   spot checks  (STARK proofs, mv_spot) Z(x) = (x^steps - 1) / (x - x_last) is not formed: the transition check is multiplied through by
//                x - x_last, as vb_spot does, and 1 / (x_last - 1) of the boundary interpolant is a plan constant (mv_inverse: the binary
//                extended Euclid algorithm on the host, once per call).  Both are units wherever G2^(n/2) = -1: with G2 of order n modulo
//                every prime factor of p, x - x_last = G2^pos - G2^((steps-1) ext) = G2^e (G2^d - 1) with d = pos - (steps - 1) ext != 0
//                modulo n (a sampled position is no multiple of ext), and x_last - 1 = G2^((steps-1) ext) - 1 with 0 < (steps-1) ext < n.
//
// Forms of the spot item.  mv_spot computes in MONTGOMERY form throughout: every value it reads -- the P, D and B values of the two
// leaves (mv_field_mont), the inputs and outputs (fpm_to_mont of any 256-bit limb value) -- is brought there by its one product, the
// term coefficients (ModTermLayout) and the MvSpotConst constants are stored there.  A term's product coef prod P_v^e therefore keeps
// one factor R however many proof values it takes (a plain factor would lose an R each), and both sides of each comparison are
// canonical Montgomery residues, equal limb for limb exactly when the residues are.
//
// Addressing rule (verify_items.cuh): every byte offset is a function of (shape, proof, item) alone; what is read from a proof only
// chooses hash order and exponents.
#pragma once
#include "fpm.cuh"
#include "modfri_items.cuh"  // mf_half
#include "modstark_items.cuh"  // ms_g2, ms_terms_degree
#include "verify_items.cuh"

#define MV_HD __host__ __device__ __forceinline__

// int.from_bytes(b, 'big') % p of 32 proof bytes (4-byte aligned): plain, canonical
MV_HD fpm mv_field(const uint8_t* b, const fpm_mod& M) {
  uint32_t w[8];
  vb_load8(b, w);
  return fpm_canon(fpm_from_wire_words(w), M);
}
// the same in Montgomery form (one product: fpm_to_mont takes any 256-bit value)
MV_HD fpm mv_field_mont(const uint8_t* b, const fpm_mod& M) {
  uint32_t w[8];
  vb_load8(b, w);
  return fpm_to_mont(fpm_from_wire_words(w), M);
}

// ---- one sampled FRI row (fri.py:318-337) -----------------------------------------------------------------------------------------
// sample = column branch (l2 entries) | 4 row branches (l1 entries each); w, inv_i and sx_mont = field(merkle_root) in Montgomery form
MV_HD bool mv_fri_row(const uint8_t* sample, uint32_t l1, uint32_t l2, const fpm& w, const fpm& inv_i, uint64_t roudeg, uint64_t y,
                      const fpm& sx_mont, const fpm_mod& M) {
  const uint8_t* rows = sample + 32ull * l2;
  const fpm r0 = mv_field(rows, M), r1 = mv_field(rows + 32ull * l1, M), r2 = mv_field(rows + 64ull * l1, M),
            r3 = mv_field(rows + 96ull * l1, M);
  const fpm colval = mv_field(sample, M);
  const fpm t = fpm_mul(sx_mont, fpm_pow(w, (roudeg - y % roudeg) % roudeg, M), M);  // x* w^-y, Montgomery form
  const fpm u0 = fpm_add(r0, r2, M), u1 = fpm_sub(r0, r2, M), u2 = fpm_add(r1, r3, M);
  const fpm u3 = fpm_mul(fpm_sub(r1, r3, M), inv_i, M);
  const fpm G0 = fpm_add(u0, u2, M), G2 = fpm_sub(u0, u2, M), G1 = fpm_add(u1, u3, M), G3 = fpm_sub(u1, u3, M);
  fpm acc = fpm_add(fpm_mul(G3, t, M), G2, M);
  acc = fpm_add(fpm_mul(acc, t, M), G1, M);
  acc = fpm_add(fpm_mul(acc, t, M), G0, M);
  return fpm_eq(mf_half(mf_half(acc, M), M), colval);
}

// ---- the final layer (fri.py:340-366), cross-multiplied -----------------------------------------------------------------------------
// data_a D / den_a of retained point a < k (plain)
MV_HD fpm mv_final_weight(uint64_t a, uint32_t exclude, const uint8_t* data, const fpm* cof, const fpm_mod& M) {
  return fpm_mul(mv_field(data + 32 * vb_pt(a, exclude), M), cof[a], M);
}
// retained point t >= k lies on the interpolant through the first k (xk[b] = x of retained point b, Montgomery form; wgt = the weights)
MV_HD bool mv_final_point(uint64_t t, uint64_t k, const fpm& w, uint32_t exclude, const uint8_t* data, const fpm* xk, const fpm* wgt,
                          const fpm& D, const fpm_mod& M) {
  const uint64_t pt = vb_pt(t, exclude);
  const fpm x = fpm_pow(w, pt, M);
  fpm total = fpm_zero();
#pragma unroll 1
  for (uint64_t a = 0; a < k; ++a) {
    fpm num = wgt[a];
#pragma unroll 1
    for (uint64_t b = 0; b < k; ++b)
      if (b != a) num = fpm_mul(num, fpm_sub(x, xk[b], M), M);
    total = fpm_add(total, num, M);
  }
  return fpm_eq(total, fpm_mul(mv_field(data + 32 * pt, M), D, M));
}

// ---- one STARK spot check (stark.py:355-374) -----------------------------------------------------------------------------------------
struct MvSpotConst {
  fpm g2, last, inv_last_m1;  // G2, x_last = G2^((steps - 1) ext), 1 / (x_last - 1): Montgomery form
  uint64_t steps;
  uint32_t width;
};
// a plain limb value (any 256 bits, 4-byte aligned) in Montgomery form
MV_HD fpm mv_limbs_mont(const fpm* p, const fpm_mod& M) {
  uint32_t w[8];
  vb_load8(reinterpret_cast<const uint8_t*>(p), w);
  return fpm_to_mont(fpm_from_words(w), M);
}
// vb_spot over the run-time modulus.  b1 / b2 = the two packed branches of the sample (leaf = P | D | B of the position, resp. of its
// g1 successor); in / out = the boundary values (plain limbs, element d at d * io_stride); terms: coef[t] (Montgomery form), exps rows
// of `row` bytes, dimension d owns [tbegin[d], tbegin[d + 1]).  Reads field values from memory where it needs them: no per-dimension
// register arrays.  Everything below is in Montgomery form (see "Forms of the spot item" above).
MV_HD bool mv_spot(const uint8_t* b1, const uint8_t* b2, uint64_t pos, const MvSpotConst& c, const fpm* in, const fpm* out,
                   uint64_t io_stride, const fpm* coef, const uint8_t* exps, uint32_t row, const uint32_t* tbegin, const fpm_mod& M) {
  const uint32_t W = c.width;
  const fpm one = fpm_from_words(M.one);
  const fpm x = fpm_pow(c.g2, pos, M);
  const fpm xm = fpm_sub(x, c.last, M);
  if (fpm_eq(xm, fpm_zero())) return false;  // the sampling excludes the trace points; a proof that lands there is malformed
  // P(g1 x) - step(P(x)) = Z(x) D(x), Z(x) = (x^steps - 1) / (x - x_last), is checked multiplied through by the unit x - x_last: the
  // same decision without an inversion per lane.  x^steps: log2(steps) squarings.
  fpm xs = x;
#pragma unroll 1
  for (uint64_t s = c.steps; s > 1; s >>= 1) xs = fpm_mul(xs, xs, M);
  const fpm zn = fpm_sub(xs, one, M);
  const fpm z2 = fpm_mul(fpm_sub(x, one, M), xm, M);
  bool ok = true;
#pragma unroll 1
  for (uint32_t d = 0; d < W; ++d) {
    fpm acc = fpm_zero();
#pragma unroll 1
    for (uint32_t t = tbegin[d]; t < tbegin[d + 1]; ++t) {
      fpm prod = mn_ld(coef + t);
#pragma unroll 1
      for (uint32_t v = 0; v < W; ++v) {
        const uint32_t e = exps[(uint64_t)t * row + v];
        if (!e) continue;
        const fpm pv = mv_field_mont(b1 + 32ull * v, M);
#pragma unroll 1
        for (uint32_t k = 0; k < e; ++k) prod = fpm_mul(prod, pv, M);
      }
      acc = fpm_add(acc, prod, M);
    }
    const fpm pg = mv_field_mont(b2 + 32ull * d, M), dx = mv_field_mont(b1 + 32ull * (W + d), M);
    ok = ok && fpm_eq(fpm_mul(fpm_sub(pg, acc, M), xm, M), fpm_mul(zn, dx, M));
    // B(x) Z2(x) + I(x) = P(x), I through (1, input) and (x_last, output)
    const fpm px = mv_field_mont(b1 + 32ull * d, M), bx = mv_field_mont(b1 + 32ull * (2 * W + d), M);
    const fpm iv = mv_limbs_mont(in + d * io_stride, M), ov = mv_limbs_mont(out + d * io_stride, M);
    const fpm slope = fpm_mul(fpm_sub(ov, iv, M), c.inv_last_m1, M);
    const fpm interp = fpm_add(fpm_sub(iv, slope, M), fpm_mul(slope, x, M), M);
    ok = ok && fpm_eq(fpm_sub(px, fpm_mul(bx, z2, M), M), interp);
  }
  return ok;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------
struct MvPlan {
  fpm_mod M;
  VbPlan shape;  // every offset and count of the shape (stark = 1 for a STARK proof); its field constants are not used
  MvSpotConst sc;  // STARK proofs only
  fpm w[SHK_FRI_MAX_ROUNDS], inv_i[SHK_FRI_MAX_ROUNDS];  // per round: the domain's generator and I^-1 = w^(3 n_r / 4), Montgomery form
  fpm w_final;         // generator of the final layer's domain, Montgomery form
  fpm xk[VB_MAX_K];    // x of the first k retained points of the final layer, Montgomery form
  fpm cof[VB_MAX_K];   // prod_{c != a} den_c, Montgomery form
  fpm D;               // prod_a den_a, Montgomery form
};

constexpr uint64_t MV_MAX_N = 1ull << 26;  // as sh_mod_fri_prove (MN_MAX_LOG_N)

// The FRI part of a plan (fri.py:268-366 on the flat layout from byte `off`, the round-0 root at root_off, -1: the caller's; its index
// sets from set_off) over p->M, w = the domain's generator in Montgomery form, n >= 4.  Returns what the host verifier returns for a
// proof of this shape that passes every check, or SH_ERR_UNSUPPORTED for a final layer over VB_MAX_FINAL.
inline int mv_plan_fri(MvPlan* p, uint64_t off, int64_t root_off, uint64_t n, fpm w, uint64_t md, uint32_t exclude, uint32_t samples,
                       uint64_t set_off, const char** why) {
  const fpm_mod& M = p->M;
  VbPlan& s = p->shape;
  s.exclude = exclude;
  uint64_t roudeg = n;
  bool first = true;
  while (md > 16) {
    *why = "a round with fewer than 16 points (maxdeg_plus_1 is too large for n)";
    if (roudeg < 16) return SH_ERR_INVALID;
    const uint32_t smp = first ? samples : 40;
    const uint64_t q = roudeg / 4;
    *why = "a column of 2^24 rows or more cannot be sampled (utils.py:69)";
    if (q >= (1ull << 24)) return SH_ERR_INVALID;  // n = 2^26 with a round: the host verifier's sampler refuses it with this code
    *why = "exclude_multiples_of = 1 divides by zero in the reference (utils.py:90)";
    if (exclude == 1) return SH_ERR_INVALID;
    *why = "exclude_multiples_of leaves no row to sample";
    if ((exclude ? q * (exclude - 1) / exclude : q) == 0) return SH_ERR_INVALID;
    *why = "more sampled rows per proof than the index sets hold (2^32)";
    if (set_off + smp > 0xffffffffull) return SH_ERR_UNSUPPORTED;
    // (q < 2^24 and 16 points or more per round: at most SHK_FRI_MAX_ROUNDS rounds)
    const uint32_t r = s.rounds++;
    p->w[r] = w;
    p->inv_i[r] = fpm_pow(w, 3 * q, M);
    VbRound& rd = s.r[r];
    rd.roudeg = roudeg;
    rd.off = off;
    rd.root_off = root_off;
    rd.samples = smp;
    rd.set_off = (uint32_t)set_off;
    const uint32_t lg = vb_ilog2(roudeg);
    rd.l1 = lg + 1;
    rd.l2 = lg - 1;
    set_off += smp;
    root_off = (int64_t)off;  // the next round's committed root is this round's root2
    off += 32 + (uint64_t)smp * 32 * (rd.l2 + 4ull * rd.l1);
    w = fpm_pow(w, 4, M);
    md /= 4;
    roudeg /= 4;
    first = false;
  }
  // (roudeg >= 4 here: n >= 4 without a round, and a round keeps a quarter of 16 points or more)
  *why = "the batch verifiers take a final layer of at most 2^10 points";
  if (roudeg > VB_MAX_FINAL) return SH_ERR_UNSUPPORTED;
  s.final_off = off;
  s.final_len = roudeg;
  const uint64_t np = vb_npts(roudeg, exclude);
  const uint64_t k = md < np ? md : np;
  s.k = k;
  s.plen = off + 32 * roudeg;
  s.ys_per_proof = (uint32_t)set_off;
  p->w_final = w;
  fpm den[VB_MAX_K];
  const fpm one = fpm_from_words(M.one);
  for (uint64_t a = 0; a < k; ++a) p->xk[a] = fpm_pow(w, vb_pt(a, exclude), M);
  p->D = one;
  for (uint64_t a = 0; a < k; ++a) {
    den[a] = one;
    for (uint64_t b = 0; b < k; ++b)
      if (b != a) den[a] = fpm_mul(den[a], fpm_sub(p->xk[a], p->xk[b], M), M);
    p->D = fpm_mul(p->D, den[a], M);
  }
  for (uint64_t a = 0; a < k; ++a) {
    p->cof[a] = one;
    for (uint64_t c = 0; c < k; ++c)
      if (c != a) p->cof[a] = fpm_mul(p->cof[a], den[c], M);
  }
  *why = "";
  return SH_OK;
}

// sh_mod_fri_verify's verdict on the shape -- what it returns for a proof of that shape that passes every check -- then the plan;
// SH_ERR_UNSUPPORTED for a final layer over VB_MAX_FINAL.  `why` receives the reason of a refusal.
inline int mv_plan_fri_proof(MvPlan* p, const uint8_t modulus[32], uint64_t n, const uint8_t root[32], uint64_t md, uint32_t exclude,
                             uint32_t samples, const char** why) {
  memset(p, 0, sizeof *p);
  *why = "null pointer";
  if (!modulus || !root) return SH_ERR_INVALID;
  *why = "the modulus must be odd and at least 3";
  if (!fpm_mod_init(modulus, &p->M)) return SH_ERR_INVALID;
  const fpm_mod& M = p->M;
  *why = "n must be a power of two and at least 4";
  if (n < 4 || (n & (n - 1))) return SH_ERR_INVALID;
  *why = "samples must be at least 1";
  if (samples == 0) return SH_ERR_INVALID;
  *why = "n is limited to 2^26";
  if (n > MV_MAX_N) return SH_ERR_UNSUPPORTED;
  const fpm wp = fpm_from_wire_bytes(root);
  *why = "root is not below the modulus";
  if (!fpm_below_p(wp, M)) return SH_ERR_ROOT_ORDER;
  const fpm w = fpm_to_mont(wp, M);
  *why = "root does not have order n in this ring (root^(n/2) != -1)";
  if (!fpm_eq(fpm_pow(w, n / 2, M), fpm_neg(fpm_from_words(M.one), M))) return SH_ERR_ROOT_ORDER;
  return mv_plan_fri(p, 0, -1, n, w, md, exclude, samples, 0, why);
}

// a^-1 modulo the odd p for a canonical plain a (plain), by the binary extended Euclid algorithm: x1 a = u and x2 a = v hold modulo p
// while u and v shrink.  false: a is no unit.  The plan's one inversion, 1 / (x_last - 1); exact for any unit of any odd modulus.
inline bool mv_inverse(const fpm& a, const fpm_mod& M, fpm* out) {
  auto is_one = [](const fpm& t) { return fpm_eq(t, fpm_from_u32(1u)); };
  auto shr1 = [](const fpm& t) {
    fpm r;
    for (int i = 0; i < 8; ++i) r.v[i] = (t.v[i] >> 1) | (i < 7 ? t.v[i + 1] << 31 : 0u);
    return r;
  };
  auto geq = [](const fpm& s, const fpm& t) {
    for (int i = 7; i >= 0; --i)
      if (s.v[i] != t.v[i]) return s.v[i] > t.v[i];
    return true;
  };
  auto sub_int = [](const fpm& s, const fpm& t) {  // s - t as integers, s >= t
    fpm r;
    uint64_t borrow = 0;
    for (int i = 0; i < 8; ++i) {
      const uint64_t x = (uint64_t)s.v[i] - t.v[i] - borrow;
      r.v[i] = (uint32_t)x;
      borrow = (x >> 32) & 1;
    }
    return r;
  };
  fpm u = a, v = fpm_from_words(M.p), x1 = fpm_from_u32(1u), x2 = fpm_zero();
  if (fpm_eq(u, fpm_zero())) return false;
  while (!is_one(u) && !is_one(v)) {
    while (!(u.v[0] & 1)) {
      u = shr1(u);
      x1 = mf_half(x1, M);
    }
    while (!(v.v[0] & 1)) {
      v = shr1(v);
      x2 = mf_half(x2, M);
    }
    if (geq(u, v)) {
      u = sub_int(u, v);
      x1 = fpm_sub(x1, x2, M);
      if (fpm_eq(u, fpm_zero())) return false;  // u == v > 1: a common factor
    } else {
      v = sub_int(v, u);
      x2 = fpm_sub(x2, x1, M);
    }
  }
  *out = is_one(u) ? x1 : x2;
  return true;
}

// sh_mod_stark_verify's verdict on the shape -- what it returns for a proof of that shape that passes every check -- then the plan
// (vb_plan_stark_proof over a run-time modulus): the STARK fields of the VbPlan, so that shk_verify_sets_and_branches draws the spot
// set and checks the packed branches and the l branch as it does for the MiMC prime, the spot constants, and the FRI proof of the
// linear combination from fri_off against l_root (byte 32), its index sets behind the spot set.
inline int mv_plan_stark_proof(MvPlan* p, const uint8_t modulus[32], uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* term_exps,
                               const uint32_t* term_counts, uint32_t samples, const char** why) {
  memset(p, 0, sizeof *p);
  *why = "null pointer";
  if (!modulus || !term_exps || !term_counts) return SH_ERR_INVALID;
  *why = "the modulus must be odd and at least 3";
  if (!fpm_mod_init(modulus, &p->M)) return SH_ERR_INVALID;
  const fpm_mod& M = p->M;
  *why = "width and samples must be at least 1";
  if (width == 0 || samples == 0) return SH_ERR_INVALID;
  *why = "steps and ext must be powers of two and at least 2";
  if (steps < 2 || (steps & (steps - 1)) || ext < 2 || (ext & (ext - 1))) return SH_ERR_INVALID;
  *why = "steps * ext must be below 2^24 (utils.py:69)";
  if (steps >= (1ull << 24) || ext >= (1u << 24) || steps * ext >= (1ull << 24)) return SH_ERR_INVALID;
  *why = "width is limited to 9 (stark.py:106-126)";
  if (width > SHK_STARK_MAX_WIDTH) return SH_ERR_UNSUPPORTED;
  uint64_t total = 0;
  *why = "more step-polynomial terms than SHK_STARK_MAX_TERMS (256)";
  for (uint32_t d = 0; d < width; ++d) {
    if (term_counts[d] > SHK_STARK_MAX_TERMS) return SH_ERR_UNSUPPORTED;
    total += term_counts[d];
  }
  if (total > SHK_STARK_MAX_TERMS) return SH_ERR_UNSUPPORTED;
  *why = "the step polynomials have no terms";
  if (total == 0) return SH_ERR_INVALID;
  const uint32_t degree = ms_terms_degree(term_exps, width, total);  // as sh_mod_stark_prove takes it: every listed term counts
  const uint64_t n = steps * ext;
  const uint32_t lg = vb_ilog2(n), k = 3 * width;
  const fpm one = fpm_from_words(M.one);
  const fpm g2 = ms_g2(M, (int)lg);  // 7^((p - 1) // (steps * ext)) (stark.py:205)
  *why = "G2 = 7^((p - 1) // (steps * ext)) does not have order steps * ext modulo p (G2^(n/2) != -1)";
  if (!fpm_eq(fpm_pow(g2, n / 2, M), fpm_neg(one, M))) return SH_ERR_ROOT_ORDER;
  VbPlan& s = p->shape;
  s.stark = 1;
  s.steps = steps;
  s.n = n;
  s.ext = ext;
  s.width = width;
  s.samples = samples;
  s.lg = lg;
  s.pb = 32ull * (2 * k + (lg - 1));
  s.lb = 32ull * (lg + 1);
  p->sc.g2 = g2;
  p->sc.last = fpm_pow(g2, (steps - 1) * ext, M);
  p->sc.steps = steps;
  p->sc.width = width;
  // x_last - 1 = G2^((steps-1) ext) - 1 with 0 < (steps - 1) ext < n: a unit (the header of this file)
  fpm inv;
  *why = "x_last - 1 is no unit modulo p (unreachable where G2^(n/2) = -1)";
  if (!mv_inverse(fpm_from_mont(fpm_sub(p->sc.last, one, M), M), M, &inv)) return SH_ERR_ROOT_ORDER;
  p->sc.inv_last_m1 = fpm_to_mont(inv, M);
  const uint64_t fri_off = 64 + (2 * s.pb + s.lb) * samples;
  return mv_plan_fri(p, fri_off, 32, n, g2, steps * (uint64_t)degree, ext, 40, samples, why);
}

// modverify_dev.hip: launch the whole verification of `batch` proofs of plan p.  ys / flags: device scratch of batch *
// p.shape.ys_per_proof and batch u32 (flags zeroed here); roots [batch][32] = the committed roots.
hipError_t shk_mod_verify_batch(const MvPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, uint32_t* ys,
                                uint32_t* flags, int32_t* status, hipStream_t st);
// the same for a STARK plan (mv_plan_stark_proof): inputs / outputs = plain limbs (any 256-bit values, 4-byte aligned; element (b, d)
// at (b width + d) io_stride), coef / exps / tbegin = the step polynomials as ModTermLayout holds them (Montgomery-form coefficients,
// exponent rows of `row` bytes)
hipError_t shk_mod_verify_stark_batch(const MvPlan& p, const uint8_t* proofs, uint32_t batch, const fpm* inputs, const fpm* outputs,
                                      uint64_t io_stride, const fpm* coef, const uint8_t* exps, uint32_t row, const uint32_t* tbegin,
                                      uint32_t* ys, uint32_t* flags, int32_t* status, hipStream_t st);
