// mod64poly_items.cuh -- polynomial arithmetic and batch inversion over any PRIME modulus below 2^64 on packed 64-bit words
// (fp64m.cuh): the element steps of modpoly_items.cuh restated over uint64_t + f64_mod.  The drivers are poly_items.cuh's own (pa_mul,
// pa_divmod, pa_zpoly, pa_lagrange: templates over the element type), run by api_mod64poly.hip over the packed-word transform and the
// kernels of mod64poly.hip, and by tests/native/mod64poly_host.cpp over a textbook transform and loops.
//
// Forms.  Every array between two launches holds PLAIN words, as sh_mod64_ntt's word form does: the caller's inputs (any 64-bit value,
// reduced where first touched), the transforms' inputs and outputs (mod64_run converts on its first loads and last stores), the tree
// levels, the remainders, the results (canonical).  A step that multiplies two plain values pays one extra Montgomery product:
// f64_mul(x, y) is x y R^-1, so either one operand is taken to Montgomery form first (m6p_mulp) or a sum of such products is multiplied
// by R^2 once (m6p_num_node).  Montgomery form is kept inside the batch inversion's tiles only: the items' leaf() and finish() convert.
//
// Inverses are Fermat's a^(p - 2) (f64_pow): the modulus is prime by contract, and for a composite one every value is unspecified but
// no address depends on a field value.
#pragma once
#include <stdint.h>

#include "fp64m.cuh"
#include "inv_items.cuh"   // IvLevels, iv_levels: the level plan is the MiMC one's
#include "poly_items.cuh"  // PaCopy and the drivers

// x y for plain x, y (any 64-bit values), canonical
F64_HD uint64_t m6p_mulp(uint64_t x, uint64_t y, const f64_mod& M) { return f64_mul(x, f64_to_mont(y, M), M); }

// ---- products and division (poly_items.cuh has the algebra) --------------------------------------------------------------------------
// A B + (-1)^i (A + B); A, B canonical (transform outputs)
F64_HD uint64_t m6p_tree_node(uint64_t A, uint64_t B, uint64_t i, const f64_mod& M) {
  const uint64_t ab = m6p_mulp(A, B, M), s = f64_add(A, B, M);
  return (i & 1) ? f64_sub(ab, s, M) : f64_add(ab, s, M);
}
// N_A (B + (-1)^i) + N_B (A + (-1)^i): the two products carry R^-1, their sum is brought back by one product with R^2
F64_HD uint64_t m6p_num_node(uint64_t NA, uint64_t NB, uint64_t A, uint64_t B, uint64_t i, const f64_mod& M) {
  const uint64_t b1 = (i & 1) ? f64_sub(B, 1u, M) : f64_add(B, 1u, M);
  const uint64_t a1 = (i & 1) ? f64_sub(A, 1u, M) : f64_add(A, 1u, M);
  return f64_mul(f64_add(f64_mul(NA, b1, M), f64_mul(NB, a1, M), M), M.r2, M);
}
// G (2 - F G); F, G canonical.  Three products: G R, F G, (2 - F G) G.  2 is canonical: p >= 3
F64_HD uint64_t m6p_newton(uint64_t F, uint64_t G, const f64_mod& M) {
  const uint64_t g = f64_to_mont(G, M), fg = f64_mul(F, g, M);
  return f64_mul(f64_sub(2u, fg, M), g, M);
}
// the middle product of a sibling pair: D RB and D RA (D, RA, RB canonical)
F64_HD void m6p_mid(uint64_t D, uint64_t RA, uint64_t RB, uint64_t* outA, uint64_t* outB, const f64_mod& M) {
  const uint64_t d = f64_to_mont(D, M);
  *outA = f64_mul(RB, d, M);
  *outB = f64_mul(RA, d, M);
}
// x^-1, plain and canonical, for any 64-bit x (0 mod p gives 0)
F64_HD uint64_t m6p_inv1(uint64_t x, const f64_mod& M) { return f64_from_mont(f64_pow(f64_to_mont(x, M), M.p - 2, M), M); }
// pa_copy_item over words: PA_NEG and PA_CANON reduce (two products), a plain copy moves the word as it is
F64_HD uint64_t m6p_copy_item(const PaCopy& c, const uint64_t* src, uint64_t r, uint64_t k, const f64_mod& M) {
  const int64_t s = c.off + (int64_t)c.dir * (int64_t)k;
  uint64_t v = 0;
  if (s >= 0 && (uint64_t)s < c.src_len) v = src[r * c.ss + (uint64_t)s];
  else if ((c.flags & PA_ONE_AT_END) && s >= 0 && (uint64_t)s == c.src_len) v = 1;
  if (c.flags & (PA_NEG | PA_CANON)) v = f64_canon(v, M);
  if (c.flags & PA_NEG) v = f64_neg(v, M);
  return v;
}
// pa_deriv_rev over words: (N - k) Z[N - k]; the integer factor may exceed p and is taken as it is (f64_mul reduces any first operand)
F64_HD uint64_t m6p_deriv_rev(const uint64_t* top, uint64_t N, uint64_t n, uint64_t k, const f64_mod& M) {
  const uint64_t m = N - k;
  if (m > n) return 0;
  const uint64_t z = m == n ? 1 : top[m + N - n];
  return f64_mul(m, f64_to_mont(z, M), M);
}
// y / d, inv = multi_inv(d) canonical and 0 exactly where d = 0: there the weight is y (a zero denominator counts as 1)
F64_HD uint64_t m6p_weight(uint64_t y, uint64_t inv, const f64_mod& M) {
  return inv == 0 ? f64_canon(y, M) : f64_mul(y, f64_to_mont(inv, M), M);
}
// a - b, a any 64-bit value (a caller's dividend), b canonical
F64_HD uint64_t m6p_sub(uint64_t a, uint64_t b, const f64_mod& M) { return f64_sub(f64_canon(a, M), b, M); }

// ---- batch inversion (inv_items.cuh has the decomposition) ---------------------------------------------------------------------------
// The tile is M6P_IV_LANES lanes x chunk items with a product tree of 2 lanes words in LDS (4 KiB).  A word costs 2 VGPRs where an fpm
// costs 8 and f64_mul keeps four constants live, not seventeen, so the chunks are four times the generic ones (256 x 2, 256 x 1):
// leaf[] and pre[] of eight values are 32 VGPRs.  mod64poly.hip's header has the compiler's figures for these constants.
constexpr uint32_t M6P_IV_LANES = 256;
constexpr uint32_t M6P_IV_CHUNK = 8;      // values per lane of multi_inv: T = 2048
constexpr uint32_t M6P_IV_ROW_CHUNK = 4;  // rows per lane of multi_interp_4: T = 1024

// Items: leaf() gives the Montgomery form of the item's value (zero: whether the value is 0 mod p, then the leaf is 1), finish() takes
// the Montgomery form of its inverse.
struct M6pElems {  // the caller's values: plain in (any 64-bit value), plain canonical out, 0 for 0; in may equal out
  const uint64_t* in;
  uint64_t* out;
  F64_HD uint64_t leaf(uint64_t i, bool& zero, const f64_mod& M) const {
    const uint64_t x = f64_to_mont(in[i], M);
    zero = x == 0;
    return zero ? M.one : x;
  }
  F64_HD void finish(uint64_t i, bool zero, uint64_t inv, const f64_mod& M) const { out[i] = zero ? 0 : f64_from_mont(inv, M); }
};
struct M6pMont {  // the tile products of a level above: Montgomery form in and out, in place
  uint64_t* v;
  F64_HD uint64_t leaf(uint64_t i, bool& zero, const f64_mod&) const {
    zero = false;
    return v[i];
  }
  F64_HD void finish(uint64_t i, bool, uint64_t inv, const f64_mod&) const { v[i] = inv; }
};
// IvRows over words: every value of a row is taken to Montgomery form on its load, the four coefficients leave it on their store
struct M6pRows {
  const uint64_t* xs;
  const uint64_t* ys;
  uint64_t* coeffs;
  F64_HD static void es(const uint64_t x[4], uint64_t e[4], const f64_mod& M) {
    const uint64_t d01 = f64_sub(x[0], x[1], M), d02 = f64_sub(x[0], x[2], M), d03 = f64_sub(x[0], x[3], M);
    const uint64_t d12 = f64_sub(x[1], x[2], M), d13 = f64_sub(x[1], x[3], M), d23 = f64_sub(x[2], x[3], M);
    e[0] = f64_mul(f64_mul(d01, d02, M), d03, M);
    e[1] = f64_neg(f64_mul(f64_mul(d01, d12, M), d13, M), M);
    e[2] = f64_mul(f64_mul(d02, d12, M), d23, M);
    e[3] = f64_neg(f64_mul(f64_mul(d03, d13, M), d23, M), M);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (e[k] == 0) e[k] = M.one;
  }
  // c += (s3, s2, s1, 1) w over the points a, b, d
  F64_HD static void term(uint64_t a, uint64_t b, uint64_t d, uint64_t w, uint64_t c[4], const f64_mod& M) {
    const uint64_t ab = f64_mul(a, b, M), apb = f64_add(a, b, M);
    c[0] = f64_add(c[0], f64_mul(f64_mul(ab, d, M), w, M), M);
    c[1] = f64_add(c[1], f64_mul(f64_add(ab, f64_mul(apb, d, M), M), w, M), M);
    c[2] = f64_add(c[2], f64_mul(f64_add(apb, d, M), w, M), M);
    c[3] = f64_add(c[3], w, M);
  }
  F64_HD void load(uint64_t i, uint64_t x[4], const f64_mod& M) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = f64_to_mont(xs[4 * i + k], M);
  }
  F64_HD uint64_t leaf(uint64_t i, bool& zero, const f64_mod& M) const {
    uint64_t x[4], e[4];
    load(i, x, M);
    es(x, e, M);
    zero = false;
    return f64_mul(f64_mul(e[0], e[1], M), f64_mul(e[2], e[3], M), M);
  }
  F64_HD void finish(uint64_t i, bool, uint64_t inv, const f64_mod& M) const {
    uint64_t x[4], y[4], e[4];
    load(i, x, M);
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = f64_to_mont(ys[4 * i + k], M);
    es(x, e, M);
    const uint64_t p1 = e[0], p2 = f64_mul(p1, e[1], M), p3 = f64_mul(p2, e[2], M);
    uint64_t I = inv, w[4];
    w[3] = f64_mul(y[3], f64_mul(I, p3, M), M);
    I = f64_mul(I, e[3], M);
    w[2] = f64_mul(y[2], f64_mul(I, p2, M), M);
    I = f64_mul(I, e[2], M);
    w[1] = f64_mul(y[1], f64_mul(I, p1, M), M);
    I = f64_mul(I, e[1], M);
    w[0] = f64_mul(y[0], I, M);
    // eq_k = X^3 - s1_k X^2 + s2_k X - s3_k over the three other points, one k at a time (written out: the indices stay static)
    uint64_t c[4] = {0, 0, 0, 0};
    term(x[1], x[2], x[3], w[0], c, M);
    term(x[0], x[2], x[3], w[1], c, M);
    term(x[0], x[1], x[3], w[2], c, M);
    term(x[0], x[1], x[2], w[3], c, M);
    coeffs[4 * i + 0] = f64_from_mont(f64_neg(c[0], M), M);
    coeffs[4 * i + 1] = f64_from_mont(c[1], M);
    coeffs[4 * i + 2] = f64_from_mont(f64_neg(c[2], M), M);
    coeffs[4 * i + 3] = f64_from_mont(c[3], M);
  }
};

// one lane's chunk: iv_chunk_forward / iv_chunk_backward over words
template <uint32_t C>
struct M6pChunk {
  uint64_t leaf[C], pre[C];  // pre[k] = leaf[0] ... leaf[k - 1]
  bool zero[C];
};
template <uint32_t L, uint32_t C, class Src>
F64_HD uint64_t m6p_chunk_forward(const Src& s, const f64_mod& M, uint64_t count, uint64_t tile, uint32_t l, M6pChunk<C>& ch) {
  const uint64_t base = tile * L * C + l;
#pragma unroll
  for (uint32_t k = 0; k < C; ++k) {
    ch.zero[k] = false;
    ch.leaf[k] = M.one;
    if (base + (uint64_t)k * L < count) ch.leaf[k] = s.leaf(base + (uint64_t)k * L, ch.zero[k], M);
    ch.pre[k] = k == 0 ? M.one : k == 1 ? ch.leaf[0] : f64_mul(ch.pre[k - 1], ch.leaf[k - 1], M);
  }
  return C == 1 ? ch.leaf[0] : f64_mul(ch.pre[C - 1], ch.leaf[C - 1], M);
}
// item K of the chunk, then items K - 1 .. 0: a recursion over the template parameter, so that every index into ch is static whatever
// the optimizer makes of a loop around a finish() as long as M6pRows' (an unroll pragma is declined there, and ch goes to scratch)
template <uint32_t L, uint32_t C, uint32_t K, class Src>
F64_HD void m6p_chunk_back_from(const Src& s, const f64_mod& M, uint64_t count, uint64_t base, const M6pChunk<C>& ch, uint64_t inv) {
  if (base + (uint64_t)K * L < count) s.finish(base + (uint64_t)K * L, ch.zero[K], K == 0 ? inv : f64_mul(inv, ch.pre[K], M), M);
  if constexpr (K > 0) m6p_chunk_back_from<L, C, K - 1>(s, M, count, base, ch, f64_mul(inv, ch.leaf[K], M));
}
template <uint32_t L, uint32_t C, class Src>
F64_HD void m6p_chunk_backward(const Src& s, const f64_mod& M, uint64_t count, uint64_t tile, uint32_t l, const M6pChunk<C>& ch,
                               uint64_t inv) {
  m6p_chunk_back_from<L, C, C - 1>(s, M, count, tile * L * C + l, ch, inv);
}
// the tile's product tree t[1 .. 2L), heap order (iv_tree_up / iv_tree_down)
F64_HD void m6p_tree_up(uint64_t* t, uint32_t node, const f64_mod& M) { t[node] = f64_mul(t[2 * node], t[2 * node + 1], M); }
F64_HD void m6p_tree_down(uint64_t* t, uint32_t node, const f64_mod& M) {
  const uint64_t a = t[2 * node], b = t[2 * node + 1], v = t[node];
  t[2 * node] = f64_mul(v, b, M);
  t[2 * node + 1] = f64_mul(v, a, M);
}
// the single power of a call: the top tile's product (Montgomery form) to its inverse
F64_HD uint64_t m6p_top_inv(uint64_t prod, const f64_mod& M) { return f64_pow(prod, M.p - 2, M); }

// the levels of a call over tiles of L x C items (inv_items.cuh: iv_levels)
template <uint32_t L, uint32_t C>
inline IvLevels m6p_iv_levels(uint64_t n) {
  return iv_levels(n, (uint64_t)L * C);
}
