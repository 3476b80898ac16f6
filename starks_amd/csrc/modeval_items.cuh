// modeval_items.cuh -- evaluation at arbitrary points over any PRIME modulus below 2^256 given at run time (sh_mod_poly_eval): the
// element steps of poly_items.cuh's pe_* restated over fpm + fpm_mod.  The drivers are poly_items.cuh's own (pa_eval, pa_eval_direct,
// pa_eval_tree: templates over the element type), run by api_modpoly.hip over the generic transform and the kernels of modeval.hip,
// and by tests/native/modeval_host.cpp over a textbook transform and loops.
//
// Forms.  Every array between two launches holds PLAIN values, as everywhere in modpoly_items.cuh, with one exception that never
// leaves the direct path: the per-point power table tbl[b m + i] = x_i^(2^b) R is kept in MONTGOMERY form.  fpm_mul(a, b) is
// a b R^-1 for ANY 256-bit a and canonical b, so with y = x^S R from the table the Horner step
//     acc = fpm_add(fpm_mul(acc, y), c)
// maps a plain canonical acc to a plain canonical acc: ONE product per coefficient per point and no conversion.  fpm_add wants a
// canonical c, and a caller's coefficient may be any 256-bit value: me_coef reduces it with one product by R mod p
// (fpm_mul(c, R) = c R R^-1 = c mod p) only when c >= p.  The test is a plain branch, which the device skips a whole wave at a time
// when every lane's coefficient is already canonical -- the common case; the reduced coefficient then serves all G points of the lane.
// Products per coefficient per point: 1, plus 1 / G for a coefficient stored unreduced.  The x^g factor at the end costs one product per
// set bit of g per point, and the table lg S + 1 products per point.
#pragma once
#include <stdint.h>

#include "modpoly_items.cuh"

// points per lane of the direct path over fpm (poly_items.cuh: pe_group; PeDirect.G carries it).  fpm_mul keeps a nine-word running
// sum beside its operands: modeval.hip records the compiler's figures for the choice.
constexpr uint32_t ME_GROUP = 4;
template <>
struct pe_group<fpm> {
  static constexpr uint32_t value = ME_GROUP;
};

// a < p as integers (fpm_below_p, for the device too)
FPM_HD bool me_below_p(const fpm& a, const fpm_mod& M) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) borrow = (((uint64_t)a.v[i] - M.p[i] - borrow) >> 32) & 1;
  return borrow != 0;
}
// any 256-bit value -> its canonical residue, one product and only when needed
FPM_HD fpm me_coef(const fpm& c, const fpm_mod& M) {
  return me_below_p(c, M) ? c : fpm_mul(c, fpm_from_words(M.one), M);
}

// tbl[b m + i] = x_i^(2^b) R, b <= lgS (y = x^S is entry lgS); x any 256-bit value
FPM_HD void me_pow_table_item(const fpm* xs, uint64_t m, uint32_t lgS, fpm* tbl, uint64_t i, const fpm_mod& M) {
  fpm v = fpm_to_mont(mn_ld(xs + i), M);
  for (uint32_t b = 0;; ++b) {
    mn_st(tbl + b * m + i, v);
    if (b == lgS) break;
    v = fpm_mul(v, v, M);
  }
}

// pe_lane over fpm: acc[q] = x_q^g sum_t c[g + S t] x_q^(S t), plain and canonical (zero for a point at or beyond m)
template <int G>
FPM_HD void me_lane(const PeDirect& s, const fpm* c, const fpm* tbl, uint64_t i0, uint64_t g, fpm acc[G], const fpm_mod& M) {
  fpm y[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    y[q] = i0 + q < s.m ? mn_ld(tbl + (uint64_t)s.lgS * s.m + i0 + q) : fpm_zero();
    acc[q] = fpm_zero();
  }
  for (uint64_t t = s.T; t-- > 0;) {
    const uint64_t k = g + (t << s.lgS);
    const fpm v = k < s.n ? me_coef(mn_ld(c + k), M) : fpm_zero();
#pragma unroll
    for (int q = 0; q < G; ++q) acc[q] = fpm_add(fpm_mul(acc[q], y[q], M), v, M);
  }
  for (uint32_t b = 0; b < s.lgS; ++b)
    if ((g >> b) & 1) {
#pragma unroll
      for (int q = 0; q < G; ++q)
        if (i0 + q < s.m) acc[q] = fpm_mul(acc[q], mn_ld(tbl + (uint64_t)b * s.m + i0 + q), M);
    }
}

// out[b][i] from the W workgroup sums part[b][w][i] (canonical): exact, so the grid shape never changes a bit of the result
FPM_HD fpm me_sum_item(const PeDirect& s, const fpm* part, uint64_t b, uint64_t i, const fpm_mod& M) {
  fpm acc = fpm_zero();
  for (uint64_t w = 0; w < s.W; ++w) acc = fpm_add(acc, mn_ld(part + (b * s.W + w) * s.m + i), M);
  return acc;
}

// pe_chunk_rev_item over fpm: the limbs as they are (the transform reduces on its first loads)
FPM_HD fpm me_chunk_rev_item(const fpm* coefs, uint64_t n, uint64_t N, uint64_t C, uint64_t r, uint64_t k) {
  const uint64_t b = r / C, s = (r - b * C) * N + N - 1 - k;
  return s < n ? mn_ld(coefs + b * n + s) : fpm_zero();
}

// a[r][i] b[i] for two transform outputs (canonical)
FPM_HD fpm me_bcast_mul_item(const fpm& a, const fpm& b, const fpm_mod& M) { return mp_mulp(a, b, M); }

// pe_combine_item over fpm: sum_j P_{b,j}(x_i) (x_i^N)^j by Horner in x^N R; the leaves are canonical (inverse transform outputs)
FPM_HD fpm me_combine_item(const fpm* leaves, const fpm* xs, uint64_t N, uint64_t C, uint64_t b, uint64_t i, const fpm_mod& M) {
  fpm xN = fpm_zero();
  if (C > 1) {
    xN = fpm_to_mont(mn_ld(xs + i), M);
    for (uint64_t e = 1; e < N; e <<= 1) xN = fpm_mul(xN, xN, M);
  }
  fpm acc = fpm_zero();
  for (uint64_t j = C; j-- > 0;) acc = fpm_add(fpm_mul(acc, xN, M), mn_ld(leaves + (b * C + j) * N + i), M);
  return acc;
}

// The generic entries' path rule (poly_items.cuh: pe_direct_preferred over PeCost).  The constants are fitted by least squares on
// relative error to the MI355X times of both forced paths over BN254 on the twelve crossover shapes of profiles/r10_poly_eval.json
// (tools/mod_poly_eval_time.py, profiles/r22_mod_poly_eval.json, "fit": 6.83e4 products per us, floor 354 us, 384 us per level,
// 1.32e4 elements per us, 1.50 us per row; rounded here).  With them the rule takes the faster path on all twelve: the crossover at
// 2^10 points lies between 2^18 and 2^19 coefficients, and (2^16, 2^16) runs the tree (7.5 ms against 64 ms).  The MiMC constants
// scaled by the transform ratio, which this replaces, sent (2^18, 2^10), (2^16, 2^12) and (2^14, 2^14) to the tree, 9 - 36 % slower.
constexpr PeCost ME_COST = {6.8e4, 350.0, 380.0, 1.32e4, 1.5};

// the tree path's largest transform (the root product of the remainder tree); the direct path runs none
inline uint64_t me_tree_transform(uint64_t m) { return 2 * pa_pow2_at_least(m); }
// the per-call choice: the direct path when the tree's transform exceeds the root's order, else the cost rule
inline bool me_direct_preferred(uint64_t n, uint64_t m, uint64_t batch, uint32_t root_log) {
  if (me_tree_transform(m) > (1ull << root_log)) return true;
  return pe_direct_preferred(ME_COST, n, m, batch);
}
