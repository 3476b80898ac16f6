// poly_items.cuh -- the per-element and per-node steps of univariate polynomial arithmetic on the device (poly_arith.hip and
// poly_eval.hip, driven from api_poly.hip): exact products, division with remainder, zpoly and lagrange_interp (starks/polynomial.py:
// 116-150, starks/poly_utils.py:322-369), all built from batched cyclic NTTs of power-of-two sizes, and evaluation at arbitrary
// points (polynomial.py:158-164; at the end of this file).
//
// Product tree.  n points are padded with zeros to N = 2^lg points (a zero point adds a factor X, which the callers shift out
// again).  A node of degree d is monic and stored as its d lower coefficients a, the leading 1 implicit.  Two siblings multiply
// without wrap-around in a cyclic convolution of size 2d:
//     (X^d + a)(X^d + b) = X^2d + X^d (a + b) + ab,     deg ab <= 2d - 2,
// and in the size-2d transform X^d is (w^d)^i = (-1)^i, so the parent's 2d lower coefficients are the inverse transform of
// A B + (-1)^i (A + B) (pa_tree_node).  A level of the tree is two batched forward transforms (one of them shared when both
// siblings sit in one batch), one pointwise launch and one batched inverse transform.
//
// Numerators.  N_v = N_L Z_R + N_R Z_L with deg N < d: in the same size-2d transform N_L (X^d + b) is N_L (B + (-1)^i)
// (pa_num_node).  At the leaves N = w_i, at the top N = sum_i w_i prod_{j != i} (X - x_j).
//
// Multipoint evaluation (Bernstein's scaled remainder tree; used by lagrange_interp and, batched over chunks, by pa_eval_tree).  For P with deg P < N and Z = prod (X - x_i), the fractional part
// of P / Z_v at a node v is y D_v(y), y = 1/X, where D_v holds |v| coefficients.  At the root D = rev_{N-1}(P) rev(Z)^-1 mod y^N
// (one Newton inverse); a child c with sibling s takes D_c[k] = (D_v rev(Z_s))[d + k], k < d, the middle of a product that a
// size-2d cyclic convolution leaves intact (pa_mid); at a leaf D = P(x_i).  rev(Z_s) = 1 + a_{d-1} y + ... + a_0 y^d
// (pa_copy with PA_ONE_AT_END: the implicit leading 1).
//
// Division.  q = rev(rev(a) rev(b)^-1 mod X^(m-k+1)), the inverse by Newton's iteration g <- g (2 - f g) (pa_newton), then
// r = a - q b on the low k - 1 coefficients.
//
// The element steps are __host__ __device__, and the drivers below are templates over an Ops back end that supplies the
// transforms and the per-level launches: api_poly.hip's runs batched NTT plans and the poly_arith.hip kernels on the ctx stream,
// tests/native/poly_tree_host.cpp's a textbook NTT and loops, so the host test runs this very driver and checks it against exact
// integers.
#pragma once
#include <stdint.h>

#include "fp256.cuh"

FP_HD fp pa_ld(const fp* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fp_load(p);
#else
  return *p;
#endif
}

// Z-node of the parent at transform index i: A B + (-1)^i (A + B)
FP_HD fp pa_tree_node(const fp& A, const fp& B, uint64_t i) {
  const fp ab = fp_mul(A, B), s = fp_add(A, B);
  return (i & 1) ? fp_sub(ab, s) : fp_add(ab, s);
}

// numerator of the parent at transform index i: N_A (B + (-1)^i) + N_B (A + (-1)^i)
FP_HD fp pa_num_node(const fp& NA, const fp& NB, const fp& A, const fp& B, uint64_t i) {
  const fp one = fp_one();
  const fp b1 = (i & 1) ? fp_sub(B, one) : fp_add(B, one);
  const fp a1 = (i & 1) ? fp_sub(A, one) : fp_add(A, one);
  return fp_add(fp_mul(NA, b1), fp_mul(NB, a1));
}

// one Newton step of the power-series inverse in the transform domain: G (2 - F G)
FP_HD fp pa_newton(const fp& F, const fp& G) {
  const fp fg = fp_mul(F, G);
  return fp_mul(G, fp_sub(fp_from_u32(2u), fg));
}

// A strided, optionally reversed copy of rows: dst[r * ds + k] = v(off + dir * k) for k < len, where v(s) = src[r * ss + s] for
// 0 <= s < src_len, 1 at s == src_len when PA_ONE_AT_END (a monic node's implicit leading coefficient), 0 elsewhere; PA_NEG
// negates, PA_CANON stores the canonical residue.
enum : uint32_t { PA_NEG = 1u, PA_ONE_AT_END = 2u, PA_CANON = 4u };
struct PaCopy {
  uint64_t rows, len;     // rows x len outputs
  uint64_t ss, ds;        // row strides of src and dst (elements)
  uint64_t src_len;       // valid elements per source row
  int64_t off;            // source index of output 0
  int32_t dir;            // +1 or -1
  uint32_t flags;
};

FP_HD fp pa_copy_item(const PaCopy& c, const fp* src, uint64_t r, uint64_t k) {
  const int64_t s = c.off + (int64_t)c.dir * (int64_t)k;
  fp v = fp_zero();
  if (s >= 0 && (uint64_t)s < c.src_len) v = pa_ld(src + r * c.ss + (uint64_t)s);
  else if ((c.flags & PA_ONE_AT_END) && s >= 0 && (uint64_t)s == c.src_len) v = fp_one();
  if (c.flags & PA_NEG) v = fp_neg(fp_canon(v));
  if (c.flags & PA_CANON) v = fp_canon(v);
  return v;
}

// rev_{N-1}(Z')[k], Z = the true product of the first n points: Z[m] = top[m + N - n] for m < n, Z[n] = 1, where top holds the N
// lower coefficients of the padded product X^(N-n) Z.  Z'[m] = (m + 1) Z[m + 1], so rev[k] = Z'[N-1-k] = (N - k) Z[N - k], zero
// where N - 1 - k >= n.
FP_HD fp pa_deriv_rev(const fp* top, uint64_t N, uint64_t n, uint64_t k) {
  const uint64_t m = N - k;  // index into Z, 1 <= m <= N
  if (m > n) return fp_zero();
  const fp z = m == n ? fp_one() : pa_ld(top + m + N - n);
  return fp_mul(fp_from_u32((uint32_t)m), z);
}

// the weight of point i: y_i / d_i, where a zero d_i (a repeated x) counts as 1 -- what the reference's multi_inv returns for a
// zero field element (poly_utils.py:317); inv = multi_inv(d) is 0 exactly there
FP_HD fp pa_weight(const fp& y, const fp& inv) {
  const fp ic = fp_canon(inv);
  return fp_eq_canon(ic, fp_zero()) ? y : fp_mul(y, ic);
}

// ---- the drivers -------------------------------------------------------------------------------------------------------------------
// Ops: int ntt(src, dst, batch, n, n_in, inverse)  [batch][n] size-n cyclic transforms over 7^((p - 1) / n) of [batch][n_in] inputs
//                                                  (zero beyond; n_in = 0: n), the inverse scaled by 1/n; src may equal dst when n_in = 0
//      int copy(PaCopy, src, dst), pointwise(a, b, out, n), tree(hz, oz, hn, on, log2d, nodes), mid(hd, hr, log2d, children),
//      newton(F, G, n), inv1(src, dst), deriv_rev(top, out, N, n), multi_inv(in, out, n), weights(ys, inv, out, n, N), sub(a, b, out, n)
//      int buf(slot, elems, E**)                      scratch that stays valid for the call (one request per slot per call)
// Every call returns 0 or an error code, which the drivers pass on.
#define PA_TRY(expr)           \
  do {                         \
    const int rc_ = (expr);    \
    if (rc_ != 0) return rc_;  \
  } while (0)

enum : int { PA_BUF_TREE = 0, PA_BUF_1, PA_BUF_2, PA_BUF_3, PA_BUF_4, PA_BUF_5, PA_BUF_COUNT };

inline uint64_t pa_pow2_at_least(uint64_t n) {
  uint64_t s = 2;
  while (s < n) s <<= 1;
  return s;
}
inline uint32_t pa_log2(uint64_t n) {
  uint32_t k = 0;
  while ((1ull << k) < n) ++k;
  return k;
}
// The drivers are templates over the element type E as well, deduced from their pointer arguments: fp here (api_poly.hip), fpm for the
// entries over a run-time modulus (api_modpoly.hip, whose Ops carries the modulus).  A parameter written pa_id<E>::type* takes no part
// in the deduction, so a call may pass nullptr there.
template <class T>
struct pa_id {
  typedef T type;
};
template <class Ops, class E>
int pa_cp(Ops& o, const typename pa_id<E>::type* src, E* dst, uint64_t rows, uint64_t len, uint64_t ss, uint64_t ds, uint64_t src_len, int64_t off, int dir,
          uint32_t flags) {
  return o.copy(PaCopy{rows, len, ss, ds, src_len, off, (int32_t)dir, flags}, src, dst);
}

// out[0, na + nb - 1) = a b, canonical; na, nb >= 1; out must not alias a or b; t1, t2: pa_pow2_at_least(na + nb - 1) elements each
template <class Ops, class E>
int pa_mul(Ops& o, const E* a, uint64_t na, const E* b, uint64_t nb, E* out, E* t1, E* t2) {
  const uint64_t nc = na + nb - 1, S = pa_pow2_at_least(nc);
  PA_TRY(o.ntt(a, t1, 1, S, na, false));
  PA_TRY(o.ntt(b, t2, 1, S, nb, false));
  PA_TRY(o.pointwise(t1, t2, t1, S));
  PA_TRY(o.ntt(t1, t1, 1, S, 0, true));
  return pa_cp(o, t1, out, 1, nc, 0, 0, nc, 0, 1, PA_CANON);
}

// elements t1 and t2 of pa_inverse need for L coefficients
inline uint64_t pa_inverse_scratch(uint64_t L) { return 2 * pa_pow2_at_least(L); }
// g[0, L) = f^-1 mod X^L by Newton's iteration (precision 1, 2, 4, ..., L); f is given by its first nf >= 1 coefficients, f[0] != 0
template <class Ops, class E>
int pa_inverse(Ops& o, const E* f, uint64_t nf, uint64_t L, E* g, E* t1, E* t2) {
  PA_TRY(o.inv1(f, g));
  for (uint64_t m = 1; m < L; m *= 2) {
    const uint64_t m2 = 2 * m < L ? 2 * m : L, S = pa_pow2_at_least(2 * m + m2 - 2);  // deg g^2 f < 2m + m2 - 2: no wrap-around
    PA_TRY(o.ntt(f, t1, 1, S, nf < m2 ? nf : m2, false));
    PA_TRY(o.ntt(g, t2, 1, S, m, false));
    PA_TRY(o.newton(t1, t2, S));
    PA_TRY(o.ntt(t2, t2, 1, S, 0, true));
    PA_TRY(pa_cp(o, t2, g, 1, m2, 0, 0, m2, 0, 1, 0));
  }
  return 0;
}

// q[0, na - nb + 1) and r[0, nb - 1) with a = q b + r (na >= nb); or, for na < nb, q empty and r[0, na) = a.  b[nb - 1] != 0 mod p.
template <class Ops, class E>
int pa_divmod(Ops& o, const E* a, uint64_t na, const E* b, uint64_t nb, E* q, E* r) {
  if (na < nb) return pa_cp(o, a, r, 1, na, 0, 0, na, 0, 1, PA_CANON);
  const uint64_t L = na - nb + 1, lb = nb < L ? nb : L;
  uint64_t S = pa_inverse_scratch(L);
  if (pa_pow2_at_least(2 * L - 1) > S) S = pa_pow2_at_least(2 * L - 1);
  if (pa_pow2_at_least(na) > S) S = pa_pow2_at_least(na);
  E *t1, *t2, *w, *qb;
  PA_TRY(o.buf(PA_BUF_1, S, &t1));
  PA_TRY(o.buf(PA_BUF_2, S, &t2));
  PA_TRY(o.buf(PA_BUF_3, 5 * L, &w));
  PA_TRY(o.buf(PA_BUF_4, na, &qb));
  E *ra = w, *rb = w + L, *g = w + 2 * L, *qr = w + 3 * L;  // qr: 2L - 1
  PA_TRY(pa_cp(o, a, ra, 1, L, 0, 0, na, (int64_t)na - 1, -1, 0));   // rev(a) mod X^L
  PA_TRY(pa_cp(o, b, rb, 1, lb, 0, 0, nb, (int64_t)nb - 1, -1, 0));  // rev(b) mod X^L
  PA_TRY(pa_inverse(o, rb, lb, L, g, t1, t2));
  PA_TRY(pa_mul(o, ra, L, g, L, qr, t1, t2));
  PA_TRY(pa_cp(o, qr, q, 1, L, 0, 0, L, (int64_t)L - 1, -1, PA_CANON));
  if (nb == 1) return 0;
  PA_TRY(pa_mul(o, q, L, b, nb, qb, t1, t2));
  return o.sub(a, qb, r, nb - 1);
}

// level j of a product tree over N points: [N >> j] monic nodes of degree 2^j, their 2^j lower coefficients each
template <class E>
inline E* pa_level(E* tree, uint64_t N, uint32_t j, bool keep) { return tree + (keep ? j : (j & 1)) * N; }

// the product tree of x_0 .. x_{n-1} padded with zeros to N points; keep: every level in tree[(lg + 1) N], else two alternating
// levels in tree[2N] (the top is pa_level(tree, N, lg, keep)); hat: 2N elements
template <class Ops, class E>
int pa_tree_up(Ops& o, const E* xs, uint64_t n, uint64_t N, E* tree, bool keep, E* hat) {
  const uint32_t lg = pa_log2(N);
  PA_TRY(pa_cp(o, xs, pa_level(tree, N, 0, keep), 1, N, 0, 0, n, 0, 1, PA_NEG));  // X - x_i, X beyond n
  for (uint32_t j = 0; j < lg; ++j) {
    const uint64_t d = 1ull << j, nodes = N >> j;
    E *lo = pa_level(tree, N, j, keep), *up = pa_level(tree, N, j + 1, keep);
    PA_TRY(o.ntt(lo, hat, nodes, 2 * d, d, false));
    PA_TRY(o.tree(hat, up, nullptr, nullptr, j + 1, nodes));
    PA_TRY(o.ntt(up, up, nodes / 2, 2 * d, 0, true));
  }
  return 0;
}

// out[0, n + 1) = prod (X - x_i), leading 1
template <class Ops, class E>
int pa_zpoly(Ops& o, const E* xs, uint64_t n, E* out) {
  if (n == 0) return pa_cp(o, nullptr, out, 1, 1, 0, 0, 0, 0, 1, PA_ONE_AT_END);
  const uint64_t N = pa_pow2_at_least(n);
  E *tree, *hat;
  PA_TRY(o.buf(PA_BUF_TREE, 2 * N, &tree));
  PA_TRY(o.buf(PA_BUF_3, 2 * N, &hat));
  PA_TRY(pa_tree_up(o, xs, n, N, tree, false, hat));
  // the padded product is X^(N - n) Z: Z's coefficients are the top's from N - n on, and the implicit 1
  return pa_cp(o, pa_level(tree, N, pa_log2(N), false), out, 1, n + 1, 0, 0, N, (int64_t)(N - n), 1, PA_ONE_AT_END | PA_CANON);
}

// The descent of the scaled remainder tree for `rows` polynomials over one tree of N points (kept levels): d0 holds the root's
// [rows][N] coefficients D (above), d1 as much scratch; *leaves gets whichever of the two ends up holding [rows][N] leaf values, the
// polynomials at x_0 .. x_{N-1}.  Every level is one batched forward transform of the parents, one of the children's rev(Z_c), the
// middle-product launch and one batched inverse transform.  Scratch: t1 rows N, t2 2N, hat 2 rows N elements; for rows > 1 also zt
// (2N), from which the children's transforms are copied to every row (for one row they are made in hat directly).
template <class Ops, class E>
int pa_descend(Ops& o, E* tree, uint64_t N, uint64_t rows, E* d0, E* d1, E* t1, E* t2, E* hat, typename pa_id<E>::type* zt, E** leaves) {
  E *dcur = d0, *dnext = d1;
  for (int j = (int)pa_log2(N) - 1; j >= 0; --j) {
    const uint64_t d = 1ull << j, children = N >> j;
    PA_TRY(o.ntt(dcur, t1, rows * children / 2, 2 * d, 0, false));
    // rev(Z_c) = 1 + a_{d-1} y + ... + a_0 y^d of every child
    PA_TRY(pa_cp(o, pa_level(tree, N, (uint32_t)j, true), t2, children, d + 1, d, d + 1, d, (int64_t)d, -1, PA_ONE_AT_END));
    if (rows == 1) {
      PA_TRY(o.ntt(t2, hat, children, 2 * d, d + 1, false));
    } else {
      PA_TRY(o.ntt(t2, zt, children, 2 * d, d + 1, false));
      PA_TRY(pa_cp(o, zt, hat, rows, 2 * N, 0, 2 * N, 2 * N, 0, 1, 0));
    }
    PA_TRY(o.mid(t1, hat, (uint32_t)j + 1, rows * children));
    PA_TRY(o.ntt(hat, hat, rows * children, 2 * d, 0, true));
    PA_TRY(pa_cp(o, hat, dnext, rows * children, d, 2 * d, d, 2 * d, (int64_t)d, 1, 0));  // the middle: coefficients [d, 2d)
    E* t = dcur;
    dcur = dnext;
    dnext = t;
  }
  *leaves = dcur;
  return 0;
}

// out[0, n) = sum_i y_i w_i prod_{j != i} (X - x_j), w_i = 1 / Z'(x_i), or 1 where Z'(x_i) = 0 (poly_utils.py:337-369); n >= 1
template <class Ops, class E>
int pa_lagrange(Ops& o, const E* xs, const E* ys, uint64_t n, E* out) {
  const uint64_t N = pa_pow2_at_least(n);
  const uint32_t lg = pa_log2(N);
  E *tree, *hat, *t1, *t2, *r;
  PA_TRY(o.buf(PA_BUF_TREE, (lg + 1) * N, &tree));
  PA_TRY(o.buf(PA_BUF_3, 2 * N, &hat));
  PA_TRY(o.buf(PA_BUF_1, 2 * N, &t1));
  PA_TRY(o.buf(PA_BUF_2, 2 * N, &t2));
  PA_TRY(o.buf(PA_BUF_5, 4 * N, &r));
  E* R[4] = {r, r + N, r + 2 * N, r + 3 * N};
  PA_TRY(pa_tree_up(o, xs, n, N, tree, true, hat));
  const E* top = pa_level(tree, N, lg, true);
  // the root of the scaled remainder tree: D = rev_{N-1}(Z') rev(Z)^-1 mod y^N; rev(Z)[k] = Z[N - k] (1 at k = 0)
  PA_TRY(pa_cp(o, top, R[2], 1, N, 0, 0, N, (int64_t)N, -1, PA_ONE_AT_END));
  PA_TRY(pa_inverse(o, R[2], N, N, R[0], t1, t2));
  PA_TRY(o.deriv_rev(top, R[1], N, n));
  PA_TRY(pa_mul(o, R[1], N, R[0], N, hat, t1, t2));  // 2N - 1 coefficients, the low N are D
  PA_TRY(pa_cp(o, hat, R[2], 1, N, 0, 0, N, 0, 1, 0));
  E* dcur = nullptr;
  PA_TRY(pa_descend(o, tree, N, 1, R[2], R[3], t1, t2, hat, nullptr, &dcur));
  // dcur[i] = Z'(x_i) = prod_{j != i} (x_i - x_j); the weights y_i / Z'(x_i) are the leaves of the numerator tree
  PA_TRY(o.multi_inv(dcur, t1, n));
  PA_TRY(o.weights(ys, t1, R[0], n, N));
  E *ncur = R[0], *nnext = R[1];
  for (uint32_t j = 0; j < lg; ++j) {
    const uint64_t d = 1ull << j, nodes = N >> j;
    PA_TRY(o.ntt(pa_level(tree, N, j, true), hat, nodes, 2 * d, d, false));
    PA_TRY(o.ntt(ncur, t1, nodes, 2 * d, d, false));
    PA_TRY(o.tree(hat, nullptr, t1, nnext, j + 1, nodes));
    PA_TRY(o.ntt(nnext, nnext, nodes / 2, 2 * d, 0, true));
    E* t = ncur;
    ncur = nnext;
    nnext = t;
  }
  // the padded numerator is X^(N - n) times the true one
  return pa_cp(o, ncur, out, 1, n, 0, 0, N, (int64_t)(N - n), 1, PA_CANON);
}

// ---- evaluation at arbitrary points: out[b][i] = P_b(x_i) (polynomial.py:158-164) ---------------------------------------------------
FP_HD void pa_st(fp* p, const fp& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  fp_store(p, v);
#else
  *p = v;
#endif
}

// Direct path (poly_eval.hip).  The S = W * PE_WG lanes of a point group split the coefficients by residue: lane g runs Horner in
// y = x^S over c[g], c[g + S], c[g + 2S], ... for each of the group's G points (held in registers: every coefficient load feeds G
// independent products), then multiplies by x^g, one product per set bit of g from a per-point table of x^(2^b).  The lanes' sums
// are added across the workgroup and, when W > 1, across workgroups by a second launch: modular addition is exact, so neither the
// grid shape nor the order changes a bit of the result.  About batch n m products; the coefficients are read once per point group.
constexpr uint32_t PE_WG = 256;           // lanes per workgroup
constexpr uint32_t PE_GROUP = 4;          // points per lane when m >= 4 (else 1) over fp; pe_group<E> names another element type's
constexpr uint64_t PE_MIN_T = 64;         // W doubles only while every lane keeps at least this many coefficients
constexpr uint64_t PE_TARGET_WGS = 2048;  // ... and the grid is below this many workgroups (8 per CU)
struct PeDirect {
  uint64_t n, m, batch;
  uint64_t W;       // workgroups per point group; S = W PE_WG lanes share the group's coefficients
  uint64_t T;       // coefficients per lane, ceil(n / S)
  uint64_t groups;  // point groups, ceil(m / G)
  uint32_t lgS, G;
};
template <class E>
struct pe_group {
  static constexpr uint32_t value = PE_GROUP;
};
template <uint32_t GROUP>
inline PeDirect pe_direct_shape_of(uint64_t n, uint64_t m, uint64_t batch) {
  PeDirect s{n, m, batch, 1, 0, 0, 0, m >= GROUP ? GROUP : 1u};
  s.groups = (m + s.G - 1) / s.G;
  while (2 * s.W * PE_WG * PE_MIN_T <= n && s.W * s.groups * batch < PE_TARGET_WGS) s.W *= 2;
  s.lgS = pa_log2(s.W * PE_WG);
  s.T = (n + (s.W << 8) - 1) / (s.W << 8);
  return s;
}
inline PeDirect pe_direct_shape(uint64_t n, uint64_t m, uint64_t batch) { return pe_direct_shape_of<PE_GROUP>(n, m, batch); }

// tbl[b m + i] = x_i^(2^b), b <= lgS (y = x^S is entry lgS)
FP_HD void pe_pow_table_item(const fp* xs, uint64_t m, uint32_t lgS, fp* tbl, uint64_t i) {
  fp v = pa_ld(xs + i);
  for (uint32_t b = 0;; ++b) {
    pa_st(tbl + b * m + i, v);
    if (b == lgS) break;
    v = fp_sqr(v);
  }
}

// lane g of the group of points i0 .. i0 + G - 1 for the n coefficients c: acc[q] = x_q^g sum_t c[g + S t] x_q^(S t), lazily reduced
// (zero for a point at or beyond m)
template <int G>
FP_HD void pe_lane(const PeDirect& s, const fp* c, const fp* tbl, uint64_t i0, uint64_t g, fp acc[G]) {
  fp y[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    y[q] = i0 + q < s.m ? pa_ld(tbl + (uint64_t)s.lgS * s.m + i0 + q) : fp_zero();
    acc[q] = fp_zero();
  }
  for (uint64_t t = s.T; t-- > 0;) {
    const uint64_t k = g + (t << s.lgS);
    const fp v = k < s.n ? pa_ld(c + k) : fp_zero();
#pragma unroll
    for (int q = 0; q < G; ++q) acc[q] = fp_add(fp_mul(acc[q], y[q]), v);
  }
  for (uint32_t b = 0; b < s.lgS; ++b)
    if ((g >> b) & 1) {
#pragma unroll
      for (int q = 0; q < G; ++q)
        if (i0 + q < s.m) acc[q] = fp_mul(acc[q], pa_ld(tbl + (uint64_t)b * s.m + i0 + q));
    }
}

// out[b][i] from the W workgroup sums part[b][w][i], canonical
FP_HD fp pe_sum_item(const PeDirect& s, const fp* part, uint64_t b, uint64_t i) {
  fp acc = fp_zero();
  for (uint64_t w = 0; w < s.W; ++w) acc = fp_add(acc, pa_ld(part + (b * s.W + w) * s.m + i));
  return fp_canon(acc);
}

// Tree path.  Over the product tree of the points padded with zeros to N = 2^ceil(log2 m) (at least 2), each polynomial is split into
// C = ceil(n / N) chunks of N coefficients, P = sum_j P_j X^(jN).  One Newton inverse of rev(Z) serves every chunk: the root step
// D = rev_{N-1}(P_j) rev(Z)^-1 mod y^N is one batched product over all batch C rows, one batched descent (pa_descend) gives every
// P_j(x_i), and pe_combine_item adds the chunks by Horner in x_i^N.  Dividing P by Z instead (pa_divmod) would need a Newton inverse
// as long as P.
// row r = b C + j: rev_{N-1}(P_{b,j})[k] = coefs[b][j N + N - 1 - k], 0 beyond n
FP_HD fp pe_chunk_rev_item(const fp* coefs, uint64_t n, uint64_t N, uint64_t C, uint64_t r, uint64_t k) {
  const uint64_t b = r / C, s = (r - b * C) * N + N - 1 - k;
  return s < n ? pa_ld(coefs + b * n + s) : fp_zero();
}

// out[b][i] = sum_j P_{b,j}(x_i) (x_i^N)^j, canonical; leaves: [batch C][N]
FP_HD fp pe_combine_item(const fp* leaves, const fp* xs, uint64_t N, uint64_t C, uint64_t b, uint64_t i) {
  fp xN = fp_zero();
  if (C > 1) {
    xN = pa_ld(xs + i);
    for (uint64_t e = 1; e < N; e <<= 1) xN = fp_sqr(xN);
  }
  fp acc = fp_zero();
  for (uint64_t j = C; j-- > 0;) acc = fp_add(fp_mul(acc, xN), pa_ld(leaves + (b * C + j) * N + i));
  return fp_canon(acc);
}

// Path choice: the direct path costs about batch n m products at products_per_us plus a floor; the tree us_per_level of launches per
// level, its batched transforms (N lg^2 elements for the tree and the inverse, 3 R N lg for the R = batch C rows' root step and
// descent, at elements_per_us) and us_per_row per row (the batched transforms of many short rows).  The constants are data, one set
// per field.  The MiMC set is fitted to the MI355X times of both forced paths over twelve shapes (profiles/r10_poly_eval.json,
// crossover_ms), which put the crossover near n m = 2^29 for n = m / 4 .. 8 m: (2^15, 2^13) direct, (2^16, 2^13) tree.
struct PeCost {
  double direct_products_per_us, direct_floor_us, tree_us_per_level, tree_elements_per_us, tree_us_per_row;
};
constexpr double PE_DIRECT_PRODUCTS_PER_US = 1.9e5;
constexpr double PE_DIRECT_FLOOR_US = 50.0;
constexpr double PE_TREE_US_PER_LEVEL = 150.0;
constexpr double PE_TREE_ELEMENTS_PER_US = 8.0e4;
constexpr double PE_TREE_US_PER_ROW = 0.8;
constexpr PeCost PE_COST_MIMC = {PE_DIRECT_PRODUCTS_PER_US, PE_DIRECT_FLOOR_US, PE_TREE_US_PER_LEVEL, PE_TREE_ELEMENTS_PER_US, PE_TREE_US_PER_ROW};
inline bool pe_direct_preferred(const PeCost& k, uint64_t n, uint64_t m, uint64_t batch) {
  const uint64_t N = pa_pow2_at_least(m), C = (n + N - 1) / N;
  const double lg = (double)pa_log2(N), R = (double)batch * (double)C;
  const double direct = k.direct_floor_us + (double)batch * (double)n * (double)m / k.direct_products_per_us;
  const double tree = k.tree_us_per_level * lg + ((double)N * lg * lg + 3.0 * R * (double)N * lg) / k.tree_elements_per_us +
                      k.tree_us_per_row * R;
  return direct <= tree;
}
inline bool pe_direct_preferred(uint64_t n, uint64_t m, uint64_t batch) { return pe_direct_preferred(PE_COST_MIMC, n, m, batch); }

// Ops (evaluation only): eval_pow_table(xs, m, lgS, tbl), eval_direct(PeDirect, coefs, tbl, dst) (dst[b][w][i]: the workgroup sums,
//      canonical when W = 1), eval_sum(PeDirect, part, out), eval_chunks(coefs, n, batch, N, C, dst) ([batch C][N] rows of
//      pe_chunk_rev_item), bcast_mul(a, b, rows, len) (a[r][i] *= b[i]), eval_combine(leaves, xs, m, N, C, batch, out)
// The element type E is deduced from the pointers, as for the drivers above (fp: api_poly.hip, fpm: api_modpoly.hip).
template <class Ops, class E>
int pa_eval_direct(Ops& o, const typename pa_id<E>::type* coefs, uint64_t n, uint64_t batch, const E* xs, uint64_t m, E* out) {
  const PeDirect s = pe_direct_shape_of<pe_group<E>::value>(n, m, batch);
  E *tbl, *part = out;
  PA_TRY(o.buf(PA_BUF_1, (s.lgS + 1) * m, &tbl));
  if (s.W > 1) PA_TRY(o.buf(PA_BUF_2, batch * s.W * m, &part));
  PA_TRY(o.eval_pow_table(xs, m, s.lgS, tbl));
  PA_TRY(o.eval_direct(s, coefs, tbl, part));
  return s.W > 1 ? o.eval_sum(s, part, out) : 0;
}

template <class Ops, class E>
int pa_eval_tree(Ops& o, const typename pa_id<E>::type* coefs, uint64_t n, uint64_t batch, const E* xs, uint64_t m, E* out) {
  const uint64_t N = pa_pow2_at_least(m), C = (n + N - 1) / N, R = batch * C;
  const uint32_t lg = pa_log2(N);
  E *tree, *hat, *t1, *t2, *rows, *r;
  PA_TRY(o.buf(PA_BUF_TREE, (lg + 1) * N, &tree));
  PA_TRY(o.buf(PA_BUF_3, 2 * N, &hat));  // the tree's transforms, then the descent's zt
  PA_TRY(o.buf(PA_BUF_1, R * N > 2 * N ? R * N : 2 * N, &t1));
  PA_TRY(o.buf(PA_BUF_2, 2 * N, &t2));
  PA_TRY(o.buf(PA_BUF_4, 2 * R * N, &rows));  // the rows' root products, then the descent's transforms
  PA_TRY(o.buf(PA_BUF_5, 2 * N + 2 * R * N, &r));
  E *g = r, *rz = r + N, *d0 = r + 2 * N, *d1 = d0 + R * N;
  PA_TRY(pa_tree_up(o, xs, m, N, tree, true, hat));
  PA_TRY(pa_cp(o, pa_level(tree, N, lg, true), rz, 1, N, 0, 0, N, (int64_t)N, -1, PA_ONE_AT_END));  // rev(Z) mod y^N
  PA_TRY(pa_inverse(o, rz, N, N, g, t1, t2));
  PA_TRY(o.ntt(g, t2, 1, 2 * N, N, false));
  PA_TRY(o.eval_chunks(coefs, n, batch, N, C, d0));
  PA_TRY(o.ntt(d0, rows, R, 2 * N, N, false));
  PA_TRY(o.bcast_mul(rows, t2, R, 2 * N));
  PA_TRY(o.ntt(rows, rows, R, 2 * N, 0, true));
  PA_TRY(pa_cp(o, rows, d0, R, N, 2 * N, N, 2 * N, 0, 1, 0));  // D: the low N coefficients of each row
  E* leaves = nullptr;
  PA_TRY(pa_descend(o, tree, N, R, d0, d1, t1, t2, rows, hat, &leaves));
  return o.eval_combine(leaves, xs, m, N, C, batch, out);
}

// out[b][i] = sum_k coefs[b][k] x_i^k, canonical, for b < batch, i < m (n = 0: zeros)
template <class Ops, class E>
int pa_eval(Ops& o, const typename pa_id<E>::type* coefs, uint64_t n, uint64_t batch, const E* xs, uint64_t m, E* out, bool direct) {
  if (m == 0) return 0;
  if (n == 0) return pa_cp(o, nullptr, out, 1, batch * m, 0, 0, 0, 0, 1, 0);
  return direct ? pa_eval_direct(o, coefs, n, batch, xs, m, out) : pa_eval_tree(o, coefs, n, batch, xs, m, out);
}
