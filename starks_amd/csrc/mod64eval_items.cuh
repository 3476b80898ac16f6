// mod64eval_items.cuh -- evaluation at arbitrary points over any PRIME modulus below 2^64 on packed 64-bit words (sh_mod64_poly_eval):
// the element steps of modeval_items.cuh restated over uint64_t + f64_mod.  The drivers are poly_items.cuh's own (pa_eval,
// pa_eval_direct, pa_eval_tree: templates over the element type), run by api_mod64poly.hip over the packed-word transform and the
// kernels of mod64eval.hip, and by tests/native/mod64eval_host.cpp over a textbook transform and loops.
//
// Forms.  Every array between two launches holds PLAIN words, as everywhere in mod64poly_items.cuh, with one exception that never
// leaves the direct path: the per-point power table tbl[b m + i] = x_i^(2^b) R is kept in MONTGOMERY form.  f64_mul(a, b) is
// a b R^-1 for ANY 64-bit a and canonical b, so with y = x^S R from the table the Horner step
//     acc = f64_add(f64_mul(acc, y), c)
// maps a plain canonical acc to a plain canonical acc: ONE product per coefficient per point and no conversion.  f64_add wants a
// canonical c, and a caller's coefficient may be any 64-bit value: m6e_coef reduces it with one product by R mod p
// (f64_mul(c, R) = c R R^-1 = c mod p; f64_canon's two products are not needed) only when c >= p.  The test is a plain branch, which
// the device skips a whole wave at a time when every lane's coefficient is already canonical; the reduced coefficient then serves all
// G points of the lane.  The x^g factor at the end costs one product per set bit of g per point, and the table lg S + 1 products per
// point.
#pragma once
#include <stdint.h>

#include "mod64poly_items.cuh"

// points per lane of the direct path over words (poly_items.cuh: pe_group; PeDirect.G carries it).  A word costs 2 VGPRs where an fpm
// costs 8, so 8 and 16 points fit the registers as well, but 4 is the fastest of the three on the MI355X: mod64eval.hip records the
// compiler's figures and the times of 4, 8 and 16 (M6E_GROUP_POINTS selects one in an A/B build).
#ifndef M6E_GROUP_POINTS
#define M6E_GROUP_POINTS 4
#endif
constexpr uint32_t M6E_GROUP = M6E_GROUP_POINTS;
template <>
struct pe_group<uint64_t> {
  static constexpr uint32_t value = M6E_GROUP;
};

// any 64-bit value -> its canonical residue, one product and only when needed
F64_HD uint64_t m6e_coef(uint64_t c, const f64_mod& M) { return c >= M.p ? f64_mul(c, M.one, M) : c; }

// tbl[b m + i] = x_i^(2^b) R, b <= lgS (y = x^S is entry lgS); x any 64-bit value
F64_HD void m6e_pow_table_item(const uint64_t* xs, uint64_t m, uint32_t lgS, uint64_t* tbl, uint64_t i, const f64_mod& M) {
  uint64_t v = f64_to_mont(xs[i], M);
  for (uint32_t b = 0;; ++b) {
    tbl[b * m + i] = v;
    if (b == lgS) break;
    v = f64_mul(v, v, M);
  }
}

// pe_lane over words: acc[q] = x_q^g sum_t c[g + S t] x_q^(S t), plain and canonical (a point at or beyond m: some canonical value,
// never stored)
template <int G>
F64_HD void m6e_lane(const PeDirect& s, const uint64_t* c, const uint64_t* tbl, uint64_t i0, uint64_t g, uint64_t acc[G],
                     const f64_mod& M) {
  uint64_t y[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    y[q] = i0 + q < s.m ? tbl[(uint64_t)s.lgS * s.m + i0 + q] : 0;
    acc[q] = 0;
  }
  for (uint64_t t = s.T; t-- > 0;) {
    const uint64_t k = g + (t << s.lgS);
    const uint64_t v = k < s.n ? m6e_coef(c[k], M) : 0;
#pragma unroll
    for (int q = 0; q < G; ++q) acc[q] = f64_add(f64_mul(acc[q], y[q], M), v, M);
  }
  for (uint32_t b = 0; b < s.lgS; ++b)
    if ((g >> b) & 1) {
#pragma unroll
      for (int q = 0; q < G; ++q)
        if (i0 + q < s.m) acc[q] = f64_mul(acc[q], tbl[(uint64_t)b * s.m + i0 + q], M);
    }
}

// out[b][i] from the W workgroup sums part[b][w][i] (canonical), here those of w = w0, w0 + step, ... (0, 1: all of them; the device
// shares an output among `step` lanes): exact, so neither the grid shape nor the order changes a bit of the result
F64_HD uint64_t m6e_sum_item(const PeDirect& s, const uint64_t* part, uint64_t b, uint64_t i, uint64_t w0, uint64_t step,
                             const f64_mod& M) {
  uint64_t acc = 0;
  for (uint64_t w = w0; w < s.W; w += step) acc = f64_add(acc, part[(b * s.W + w) * s.m + i], M);
  return acc;
}

// pe_chunk_rev_item over words: the words as they are (the transform reduces on its first loads)
F64_HD uint64_t m6e_chunk_rev_item(const uint64_t* coefs, uint64_t n, uint64_t N, uint64_t C, uint64_t r, uint64_t k) {
  const uint64_t b = r / C, s = (r - b * C) * N + N - 1 - k;
  return s < n ? coefs[b * n + s] : 0;
}

// a[r][i] b[i] for two transform outputs (canonical)
F64_HD uint64_t m6e_bcast_mul_item(uint64_t a, uint64_t b, const f64_mod& M) { return m6p_mulp(a, b, M); }

// pe_combine_item over words: sum_j P_{b,j}(x_i) (x_i^N)^j by Horner in x^N R; the leaves are canonical (inverse transform outputs)
F64_HD uint64_t m6e_combine_item(const uint64_t* leaves, const uint64_t* xs, uint64_t N, uint64_t C, uint64_t b, uint64_t i,
                                 const f64_mod& M) {
  uint64_t xN = 0;
  if (C > 1) {
    xN = f64_to_mont(xs[i], M);
    for (uint64_t e = 1; e < N; e <<= 1) xN = f64_mul(xN, xN, M);
  }
  uint64_t acc = 0;
  for (uint64_t j = C; j-- > 0;) acc = f64_add(f64_mul(acc, xN, M), leaves[(b * C + j) * N + i], M);
  return acc;
}

// The packed entries' path rule (poly_items.cuh: pe_direct_preferred over PeCost).  The constants are fitted to the MI355X times of
// both forced paths over Goldilocks on the twelve crossover shapes of tools/mod_poly_eval_time.py (tools/mod64_poly_eval_time.py,
// profiles/r24_mod64_poly_eval.json, "fit_weighted": 9.94e5 products per us, floor 67.5 us, 185 us per level, 1.137e4 elements per
// us, 0 us per row; rounded here), by least squares on relative error with every shape weighted by min / max of its two paths' times.
// On this path the direct kernel runs about a million products per us and wins ALL twelve shapes, eleven of them by 4.8x - 28000x;
// only (2^16, 2^16) is near a decision (4.37 ms against 5.02 ms), and the tree's time there is 314 us per level where it is 160 at
// 2^10 points, which the model's single per-level term cannot follow: the unweighted fit ("fit" in the profile) puts 198 us per
// level, prices that tree at 3.6 ms and picks it, 15 % slower.  The starting point, ME_COST with its two throughputs divided by the
// packed : generic transform ratio 0.26 ({2.6e5, 350, 380, 5.1e4, 1.5}), made the same one mistake.  With the constants below the
// rule takes the faster path on all twelve; beyond them it sends (2^17, 2^17), (2^20, 2^20) and many-row shapes such as (2^25, 2^12)
// to the tree.  The last is timed in profiles/r24_mod64_poly_eval_check.json ("beyond_ms"): 156.6 ms direct, 31.4 ms tree.  The
// weighted model is loose where its weights are small (32 ms for the 52 ms tree at (2^24, 128)) and has no per-row term.
constexpr PeCost M6E_COST = {9.9e5, 67.0, 185.0, 1.14e4, 0.0};

// the tree path's largest transform (the root product of the remainder tree); the direct path runs none
inline uint64_t m6e_tree_transform(uint64_t m) { return 2 * pa_pow2_at_least(m); }
// the per-call choice: the direct path when the tree's transform exceeds the root's order, else the cost rule
inline bool m6e_direct_preferred(uint64_t n, uint64_t m, uint64_t batch, uint32_t root_log) {
  if (m6e_tree_transform(m) > (1ull << root_log)) return true;
  return pe_direct_preferred(M6E_COST, n, m, batch);
}
