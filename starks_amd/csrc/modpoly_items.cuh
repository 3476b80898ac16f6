// modpoly_items.cuh -- polynomial arithmetic and batch inversion over any PRIME modulus below 2^256 given at run time (fpm.cuh): the
// element steps of poly_items.cuh and inv_items.cuh restated over fpm + fpm_mod.  The drivers are poly_items.cuh's own (pa_mul,
// pa_divmod, pa_zpoly, pa_lagrange: templates over the element type), run by api_modpoly.hip over the generic transform and the
// kernels of modpoly.hip, and by tests/native/modpoly_host.cpp over a textbook transform and loops.
//
// Forms.  Every array between two launches holds PLAIN values: the caller's inputs (any 256-bit value, reduced where first touched),
// the transforms' inputs and outputs (mod_run converts on its first loads and last stores), the tree levels, the remainders, the
// results (canonical).  A step that multiplies two plain values therefore pays one extra Montgomery product: fpm_mul(x, y) is
// x y R^-1, so either one operand is taken to Montgomery form first (mp_mulp) or a sum of such products is multiplied by R^2 once
// (mp_num_node).  Inside the batch inversion the tile products of the upper levels stay in Montgomery form: only the items' leaf()
// and finish() convert.
//
// Inverses are Fermat's a^(p - 2) (fpm_pow_limbs): the modulus is prime by contract, and for a composite one every value is
// unspecified but no address depends on a field value.
#pragma once
#include <stdint.h>

#include "inv_items.cuh"      // IvLevels, iv_levels: the level plan is the MiMC one's
#include "modstark_items.cuh"  // fpm_pow_limbs, fpm_is_zero, ms_pm2 (and fpm.cuh, modntt_items.cuh: mn_ld, mn_st)
#include "poly_items.cuh"     // PaCopy and the drivers

// x y for plain x, y (any 256-bit values), canonical
FPM_HD fpm mp_mulp(const fpm& x, const fpm& y, const fpm_mod& M) { return fpm_mul(x, fpm_to_mont(y, M), M); }
FPM_HD fpm mp_r2(const fpm_mod& M) { return fpm_from_words(M.r2); }

// ---- products and division (poly_items.cuh has the algebra) --------------------------------------------------------------------------
// A B + (-1)^i (A + B); A, B canonical (transform outputs)
FPM_HD fpm mp_tree_node(const fpm& A, const fpm& B, uint64_t i, const fpm_mod& M) {
  const fpm ab = mp_mulp(A, B, M), s = fpm_add(A, B, M);
  return (i & 1) ? fpm_sub(ab, s, M) : fpm_add(ab, s, M);
}
// N_A (B + (-1)^i) + N_B (A + (-1)^i): the two products carry R^-1, their sum is brought back by one product with R^2
FPM_HD fpm mp_num_node(const fpm& NA, const fpm& NB, const fpm& A, const fpm& B, uint64_t i, const fpm_mod& M) {
  const fpm one = fpm_from_u32(1u);
  const fpm b1 = (i & 1) ? fpm_sub(B, one, M) : fpm_add(B, one, M);
  const fpm a1 = (i & 1) ? fpm_sub(A, one, M) : fpm_add(A, one, M);
  return fpm_mul(fpm_add(fpm_mul(NA, b1, M), fpm_mul(NB, a1, M), M), mp_r2(M), M);
}
// G (2 - F G); F, G canonical.  Three products: G R, F G, (2 - F G) G
FPM_HD fpm mp_newton(const fpm& F, const fpm& G, const fpm_mod& M) {
  const fpm g = fpm_to_mont(G, M), fg = fpm_mul(F, g, M);
  const fpm two = fpm_from_u32(2u);  // canonical: p >= 3
  return fpm_mul(fpm_sub(two, fg, M), g, M);
}
// the middle product of a sibling pair: D RB and D RA (D, RA, RB canonical)
FPM_HD void mp_mid(const fpm& D, const fpm& RA, const fpm& RB, fpm* outA, fpm* outB, const fpm_mod& M) {
  const fpm d = fpm_to_mont(D, M);
  *outA = fpm_mul(RB, d, M);
  *outB = fpm_mul(RA, d, M);
}
// src[0]^-1, plain and canonical, for any 256-bit src[0] (0 gives 0)
FPM_HD fpm mp_inv1(const fpm& x, const fpm& pm2, const fpm_mod& M) {
  return fpm_from_mont(fpm_pow_limbs(fpm_to_mont(x, M), pm2.v, M), M);
}
// pa_copy_item over fpm: PA_NEG and PA_CANON reduce (two products), a plain copy moves the limbs as they are
FPM_HD fpm mp_copy_item(const PaCopy& c, const fpm* src, uint64_t r, uint64_t k, const fpm_mod& M) {
  const int64_t s = c.off + (int64_t)c.dir * (int64_t)k;
  fpm v = fpm_zero();
  if (s >= 0 && (uint64_t)s < c.src_len) v = mn_ld(src + r * c.ss + (uint64_t)s);
  else if ((c.flags & PA_ONE_AT_END) && s >= 0 && (uint64_t)s == c.src_len) v = fpm_from_u32(1u);
  if (c.flags & (PA_NEG | PA_CANON)) v = fpm_canon(v, M);
  if (c.flags & PA_NEG) v = fpm_neg(v, M);
  return v;
}
// pa_deriv_rev over fpm: (N - k) Z[N - k]; the integer factor may exceed p and is taken as it is (fpm_mul reduces any first operand)
FPM_HD fpm mp_deriv_rev(const fpm* top, uint64_t N, uint64_t n, uint64_t k, const fpm_mod& M) {
  const uint64_t m = N - k;
  if (m > n) return fpm_zero();
  const fpm z = m == n ? fpm_from_u32(1u) : mn_ld(top + m + N - n);
  return fpm_mul(fpm_from_u32((uint32_t)m), fpm_to_mont(z, M), M);
}
// y / d, inv = multi_inv(d) canonical and 0 exactly where d = 0: there the weight is y (a zero denominator counts as 1)
FPM_HD fpm mp_weight(const fpm& y, const fpm& inv, const fpm_mod& M) {
  return fpm_is_zero(inv) ? fpm_canon(y, M) : fpm_mul(y, fpm_to_mont(inv, M), M);
}
// a - b, a any 256-bit value (a caller's dividend), b canonical
FPM_HD fpm mp_sub(const fpm& a, const fpm& b, const fpm_mod& M) { return fpm_sub(fpm_canon(a, M), b, M); }

// The largest transform a call runs: what the drivers of poly_items.cuh ask of Ops::ntt for these sizes (the host test compares it
// with what its Ops saw).  0: the call runs no transform.
enum : int { MP_OP_MUL = 0, MP_OP_DIVMOD = 1, MP_OP_ZPOLY = 2, MP_OP_LAGRANGE = 3, MP_OP_EVAL = 4 };
inline uint64_t mp_max_transform(int op, uint64_t na, uint64_t nb) {
  auto mx = [](uint64_t a, uint64_t b) { return a > b ? a : b; };
  switch (op) {
    case MP_OP_MUL:
      return na && nb ? pa_pow2_at_least(na + nb - 1) : 0;
    case MP_OP_DIVMOD: {
      if (nb == 0 || na < nb) return 0;
      const uint64_t L = na - nb + 1;
      uint64_t s = pa_pow2_at_least(2 * L - 1);  // rev(a) rev(b)^-1
      for (uint64_t m = 1; m < L; m *= 2) s = mx(s, pa_pow2_at_least(2 * m + (2 * m < L ? 2 * m : L) - 2));  // the Newton steps
      if (nb > 1) s = mx(s, pa_pow2_at_least(na));                                                          // q b
      return s;
    }
    case MP_OP_ZPOLY:
      return na ? pa_pow2_at_least(na) : 0;
    case MP_OP_LAGRANGE:
      return na ? 2 * pa_pow2_at_least(na) : 0;  // the root product of the remainder tree
    case MP_OP_EVAL:
      return na && nb ? 2 * pa_pow2_at_least(nb) : 0;  // na coefficients at nb points on the tree path (the direct path runs none)
  }
  return 0;
}

// ---- batch inversion (inv_items.cuh has the decomposition) ---------------------------------------------------------------------------
// The tile is MP_IV_LANES lanes x MP_IV_CHUNK values: fpm_mul keeps the modulus and a ninth word live beside its operands, so the chunk
// is half the MiMC one's (with four values per lane the compiler keeps leaf[] and pre[] in scratch, 264 bytes per lane, in both kernels
// over MpElems; with two: 51 and 110 VGPRs, none).
constexpr uint32_t MP_IV_LANES = 256;
constexpr uint32_t MP_IV_CHUNK = 2;      // values per lane of multi_inv: T = 512
constexpr uint32_t MP_IV_ROW_CHUNK = 1;  // rows per lane of multi_interp_4: T = 256

// Items: leaf() gives the Montgomery form of the item's value (zero: whether the value is 0 mod p, then the leaf is 1), finish() takes
// the Montgomery form of its inverse.
struct MpElems {  // the caller's values: plain in (any 256-bit value), plain canonical out, 0 for 0; in may equal out
  const fpm* in;
  fpm* out;
  FPM_HD fpm leaf(uint64_t i, bool& zero, const fpm_mod& M) const {
    const fpm x = fpm_to_mont(mn_ld(in + i), M);
    zero = fpm_is_zero(x);
    return zero ? fpm_from_words(M.one) : x;
  }
  FPM_HD void finish(uint64_t i, bool zero, const fpm& inv, const fpm_mod& M) const {
    mn_st(out + i, zero ? fpm_zero() : fpm_from_mont(inv, M));
  }
};
struct MpMont {  // the tile products of a level above: Montgomery form in and out, in place
  fpm* v;
  FPM_HD fpm leaf(uint64_t i, bool& zero, const fpm_mod&) const {
    zero = false;
    return mn_ld(v + i);
  }
  FPM_HD void finish(uint64_t i, bool, const fpm& inv, const fpm_mod&) const { mn_st(v + i, inv); }
};
// IvRows over fpm: every value of a row is taken to Montgomery form on its load, the four coefficients leave it on their store
struct MpRows {
  const fpm* xs;
  const fpm* ys;
  fpm* coeffs;
  FPM_HD static void es(const fpm x[4], fpm e[4], const fpm_mod& M) {
    const fpm d01 = fpm_sub(x[0], x[1], M), d02 = fpm_sub(x[0], x[2], M), d03 = fpm_sub(x[0], x[3], M);
    const fpm d12 = fpm_sub(x[1], x[2], M), d13 = fpm_sub(x[1], x[3], M), d23 = fpm_sub(x[2], x[3], M);
    e[0] = fpm_mul(fpm_mul(d01, d02, M), d03, M);
    e[1] = fpm_neg(fpm_mul(fpm_mul(d01, d12, M), d13, M), M);
    e[2] = fpm_mul(fpm_mul(d02, d12, M), d23, M);
    e[3] = fpm_neg(fpm_mul(fpm_mul(d03, d13, M), d23, M), M);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (fpm_is_zero(e[k])) e[k] = fpm_from_words(M.one);
  }
  // c += (s3, s2, s1, 1) w over the points a, b, d
  FPM_HD static void term(const fpm& a, const fpm& b, const fpm& d, const fpm& w, fpm c[4], const fpm_mod& M) {
    const fpm ab = fpm_mul(a, b, M), apb = fpm_add(a, b, M);
    c[0] = fpm_add(c[0], fpm_mul(fpm_mul(ab, d, M), w, M), M);
    c[1] = fpm_add(c[1], fpm_mul(fpm_add(ab, fpm_mul(apb, d, M), M), w, M), M);
    c[2] = fpm_add(c[2], fpm_mul(fpm_add(apb, d, M), w, M), M);
    c[3] = fpm_add(c[3], w, M);
  }
  FPM_HD void load(uint64_t i, fpm x[4], const fpm_mod& M) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = fpm_to_mont(mn_ld(xs + 4 * i + k), M);
  }
  FPM_HD fpm leaf(uint64_t i, bool& zero, const fpm_mod& M) const {
    fpm x[4], e[4];
    load(i, x, M);
    es(x, e, M);
    zero = false;
    return fpm_mul(fpm_mul(e[0], e[1], M), fpm_mul(e[2], e[3], M), M);
  }
  FPM_HD void finish(uint64_t i, bool, const fpm& inv, const fpm_mod& M) const {
    fpm x[4], y[4], e[4];
    load(i, x, M);
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = fpm_to_mont(mn_ld(ys + 4 * i + k), M);
    es(x, e, M);
    const fpm p1 = e[0], p2 = fpm_mul(p1, e[1], M), p3 = fpm_mul(p2, e[2], M);
    fpm I = inv, w[4];
    w[3] = fpm_mul(y[3], fpm_mul(I, p3, M), M);
    I = fpm_mul(I, e[3], M);
    w[2] = fpm_mul(y[2], fpm_mul(I, p2, M), M);
    I = fpm_mul(I, e[2], M);
    w[1] = fpm_mul(y[1], fpm_mul(I, p1, M), M);
    I = fpm_mul(I, e[1], M);
    w[0] = fpm_mul(y[0], I, M);
    // eq_k = X^3 - s1_k X^2 + s2_k X - s3_k over the three other points, one k at a time (written out: the indices stay static)
    fpm c[4] = {fpm_zero(), fpm_zero(), fpm_zero(), fpm_zero()};
    term(x[1], x[2], x[3], w[0], c, M);
    term(x[0], x[2], x[3], w[1], c, M);
    term(x[0], x[1], x[3], w[2], c, M);
    term(x[0], x[1], x[2], w[3], c, M);
    mn_st(coeffs + 4 * i + 0, fpm_from_mont(fpm_neg(c[0], M), M));
    mn_st(coeffs + 4 * i + 1, fpm_from_mont(c[1], M));
    mn_st(coeffs + 4 * i + 2, fpm_from_mont(fpm_neg(c[2], M), M));
    mn_st(coeffs + 4 * i + 3, fpm_from_mont(c[3], M));
  }
};

// one lane's chunk: iv_chunk_forward / iv_chunk_backward over fpm
template <uint32_t C>
struct MpChunk {
  fpm leaf[C], pre[C];  // pre[k] = leaf[0] ... leaf[k - 1]
  bool zero[C];
};
template <uint32_t L, uint32_t C, class Src>
FPM_HD fpm mp_chunk_forward(const Src& s, const fpm_mod& M, uint64_t count, uint64_t tile, uint32_t l, MpChunk<C>& ch) {
  const uint64_t base = tile * L * C + l;
  const fpm one = fpm_from_words(M.one);
#pragma unroll
  for (uint32_t k = 0; k < C; ++k) {
    ch.zero[k] = false;
    ch.leaf[k] = one;
    if (base + (uint64_t)k * L < count) ch.leaf[k] = s.leaf(base + (uint64_t)k * L, ch.zero[k], M);
    ch.pre[k] = k == 0 ? one : k == 1 ? ch.leaf[0] : fpm_mul(ch.pre[k - 1], ch.leaf[k - 1], M);
  }
  return C == 1 ? ch.leaf[0] : fpm_mul(ch.pre[C - 1], ch.leaf[C - 1], M);
}
template <uint32_t L, uint32_t C, class Src>
FPM_HD void mp_chunk_backward(const Src& s, const fpm_mod& M, uint64_t count, uint64_t tile, uint32_t l, const MpChunk<C>& ch, fpm inv) {
  const uint64_t base = tile * L * C + l;
#pragma unroll
  for (uint32_t j = 0; j < C; ++j) {  // k = C - 1 .. 0, counted up so that the unrolled k stays static
    const uint32_t k = C - 1 - j;
    if (base + (uint64_t)k * L < count) s.finish(base + (uint64_t)k * L, ch.zero[k], k == 0 ? inv : fpm_mul(inv, ch.pre[k], M), M);
    if (k) inv = fpm_mul(inv, ch.leaf[k], M);
  }
}
// the tile's product tree t[1 .. 2L), heap order (iv_tree_up / iv_tree_down)
FPM_HD void mp_tree_up(fpm* t, uint32_t node, const fpm_mod& M) { t[node] = fpm_mul(t[2 * node], t[2 * node + 1], M); }
FPM_HD void mp_tree_down(fpm* t, uint32_t node, const fpm_mod& M) {
  const fpm a = t[2 * node], b = t[2 * node + 1], v = t[node];
  t[2 * node] = fpm_mul(v, b, M);
  t[2 * node + 1] = fpm_mul(v, a, M);
}
// the single power of a call: the top tile's product (Montgomery form) to its inverse
FPM_HD fpm mp_top_inv(const fpm& prod, const fpm& pm2, const fpm_mod& M) { return fpm_pow_limbs(prod, pm2.v, M); }

// the levels of a call over tiles of L x C items (inv_items.cuh: iv_levels)
template <uint32_t L, uint32_t C>
inline IvLevels mp_iv_levels(uint64_t n) {
  return iv_levels(n, (uint64_t)L * C);
}
