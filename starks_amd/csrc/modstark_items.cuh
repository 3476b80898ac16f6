// modstark_items.cuh -- the middle of STARK.mk_proof (stark.py:233-279) over any prime modulus below 2^256 (fpm.cuh): the per-item
// bodies of the boundary interpolant, X P'(X), the domain tables and their batch inversion, the quotients D and B, the packed Merkle
// leaves, the Fiat-Shamir scalars, the linear combination and the spot-check gather.  modstark.hip wraps them in kernels,
// api_modstark.hip drives them; tests/native/modstark_host.cpp walks the same functions on the host over the same grids.
//
// The algorithm is stark.hip's (its header has the derivation): D = C (x - r) / (x^s - 1) and B = (P - I) / ((x - 1)(x - r)) are
// evaluated on the n = steps * ext points x_i = G2^i; on the trace points, where the quotients are 0/0, the value is the formal
// derivative's (x C'(x) through Q = X P'(X) and the step polynomials' partial derivatives).  Only the arithmetic differs.
//
// Forms.  Every array between the kernels -- witness, inputs, P, Q, D, B, l -- holds PLAIN values, and all but the caller's witness
// and inputs are CANONICAL (below p): they are hashed and written as stored, a byte swap, never reduced modulo the MiMC prime.
// Multipliers are in Montgomery form, so that fpm_mul(plain, Montgomery) is plain and canonical: the term coefficients, the scalars,
// x_i, 1 / Z2(x_i).  The step polynomials are evaluated on Montgomery images of the point's P values (fpm_to_mont takes any 256-bit
// value, which is also where a witness value at or above p is reduced); their result meets the PLAIN table (x - r) / (x^s - 1) in the
// one product that leaves Montgomery form.  No address depends on a field value: a composite modulus gives unspecified bytes, in bounds.
#pragma once
#include "modfri_items.cuh"

constexpr uint32_t MS_WG = 256;         // threads per workgroup
constexpr uint32_t MS_MAX_WIDTH = 9;    // SHK_STARK_MAX_WIDTH
constexpr uint32_t MS_MAX_TERMS = 256;  // SHK_STARK_MAX_TERMS
constexpr uint32_t MS_INV_CHUNK = 32;   // values per batch-inversion item: one p - 2 power (~380 products) per chunk

struct MsArgs {
  const fpm* p_evals;  // [batch * width][n]      trace polynomials on the G2 domain
  fpm* d_work;         // [batch * width][n]      D
  fpm* b_work;         // [batch * width][n]      B
  const fpm* q_evals;  // [batch * width][steps]  Q_c = X P_c'(X) on G1
  const fpm* wit;      // [batch * width][steps]  the witness, any 256-bit values
  const fpm* inputs;   // [batch * width]         any 256-bit values
  fpm* iab;            // [batch * width][2]      boundary interpolant a + b X
  uint64_t n, steps;
  uint32_t ext, width, batch, log_n;
  const fpm* tw;       // G2^e, Montgomery form, e < n / 2 (the n-point transform's table)
  const fpm* inv_z2;   // [n] 1 / ((x_i - 1)(x_i - r)), Montgomery form, 0 at the two roots
  const fpm* fz;       // [n] (x_i - r) / (x_i^steps - 1), PLAIN, 0 on the trace points
  const fpm* xpow;     // [n] x_i, Montgomery form
  fpm x_last, g1, inv_last_m1, inv_1_m_last;  // r, 1 / r, 1 / (r - 1), 1 / (1 - r): Montgomery form
  fpm inv_steps;       // 1 / steps, plain
  uint32_t* bad;       // [batch] raised when a transition constraint of proof b fails on the trace
  // step polynomials: term t = coef[t] prod_v X_v^exps[t][v] (rows of `width` bytes), terms of dimension c: [term_begin[c], term_begin[c+1]);
  // d step_c / d X_v = derivative terms [dterm_begin[c width + v], dterm_begin[c width + v + 1]).  Coefficients in Montgomery form.
  const fpm* term_coef;
  const uint8_t* term_exps;
  uint32_t term_begin[MS_MAX_WIDTH + 1];
  const fpm* dterm_coef;
  const uint8_t* dterm_exps;
  const uint32_t* dterm_begin;
};

// the batch inversion of `count` Montgomery-form values: out[i] = in[i]^-1 (Montgomery form), 0 for in[i] = 0; in != out
struct MsInv {
  const fpm* in;
  fpm* out;
  uint64_t count, chunks;  // chunks = ceil(count / MS_INV_CHUNK); item g owns i = g + k chunks
  fpm pm2;                 // p - 2 as an integer
};

// the domain tables of (p, steps, ext): den / table are [2][n]; see ms_den_item and ms_tables_item
struct MsTables {
  fpm* den;    // scratch: (x_i - 1)(x_i - r) | x_i^steps - 1, Montgomery form
  fpm* table;  // inv_z2 | fz | xpow
  const fpm* tw;
  uint64_t n, steps;
  uint32_t ext, log_n;
  fpm x_last;  // Montgomery form
};

// a^e for a 256-bit exponent (a in Montgomery form, canonical)
FPM_HD fpm fpm_pow_limbs(fpm a, const uint32_t e[8], const fpm_mod& M) {
  fpm r = fpm_from_words(M.one);
  int top = 255;
  while (top >= 0 && !((e[top >> 5] >> (top & 31)) & 1)) --top;
  for (int i = 0; i <= top; ++i) {
    if ((e[i >> 5] >> (i & 31)) & 1) r = fpm_mul(r, a, M);
    a = fpm_mul(a, a, M);
  }
  return r;
}
FPM_HD bool fpm_is_zero(const fpm& a) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.v[i];
  return d == 0;
}
// G2^i in Montgomery form from the transform's half table (G2^(n/2) = -1)
FPM_HD fpm ms_x(const fpm* tw, uint32_t log_n, uint64_t i, const fpm_mod& M) {
  const uint64_t h = 1ull << (log_n - 1);
  const fpm t = mn_ld(tw + (i & (h - 1)));
  return i & h ? fpm_neg(t, M) : t;
}

// ---- host side of a call (no device): G2, p - 2, the term image ------------------------------------------------------------------------
// G2 = 7^((p - 1) // 2^lg) in Montgomery form (stark.py:205): p - 1 is p without its low bit, the division a shift (lg < 32)
inline fpm ms_g2(const fpm_mod& M, int lg) {
  uint32_t e[8];
  for (int i = 0; i < 8; ++i) {
    const uint32_t lo = i == 0 ? M.p[0] & ~1u : M.p[i], hi = i + 1 < 8 ? M.p[i + 1] : 0u;
    e[i] = lg ? (uint32_t)((((uint64_t)hi << 32) | lo) >> lg) : lo;
  }
  return fpm_pow_limbs(fpm_to_mont(fpm_from_u32(7u), M), e, M);
}
inline fpm ms_pm2(const fpm_mod& M) {  // p - 2 as an integer (p >= 3)
  fpm r;
  uint64_t borrow = 2;
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)M.p[i] - borrow;
    r.v[i] = (uint32_t)x;
    borrow = (x >> 32) & 1;
  }
  return r;
}
// MultivariatePolynomial.degree over every term (multivariate_polynomial.py:111-117)
inline uint32_t ms_terms_degree(const uint8_t* exps, uint32_t width, uint64_t total) {
  uint32_t degree = 0;
  for (uint64_t t = 0; t < total; ++t) {
    uint32_t sum = 0;
    for (uint32_t v = 0; v < width; ++v) sum += exps[t * width + v];
    if (sum > degree) degree = sum;
  }
  return degree;
}
// The terms and their partial derivatives as the kernels read them: cf[total], dcf / dex rows for up to total * width derivative terms,
// ex = the exponent rows, dbeg[width * width + 1], begin[width + 1].  Coefficients are field(v): any 256-bit value, modulo p.
// d/dX_v of coef * prod X^e = (coef * e_v) * X_v^(e_v - 1) * prod_{u != v} X_u^e_u
inline void ms_terms_build(const fpm_mod& M, uint32_t width, const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts, uint64_t total,
                           fpm* cf, fpm* dcf, uint8_t* ex, uint8_t* dex, uint32_t* dbeg, uint32_t* begin) {
  for (uint64_t t = 0; t < total; ++t) cf[t] = fpm_to_mont(fpm_from_wire_bytes(coefs + 32 * t), M);
  for (uint64_t k = 0; k < (uint64_t)width * total; ++k) ex[k] = exps[k];
  begin[0] = 0;
  for (uint32_t d = 0; d < width; ++d) begin[d + 1] = begin[d] + counts[d];
  uint32_t nd = 0;
  for (uint32_t d = 0; d < width; ++d) {
    for (uint32_t v = 0; v < width; ++v) {
      dbeg[d * width + v] = nd;
      for (uint32_t t = begin[d]; t < begin[d + 1]; ++t) {
        const uint32_t e = exps[(size_t)t * width + v];
        if (!e) continue;
        dcf[nd] = fpm_mul(cf[t], fpm_to_mont(fpm_from_u32(e), M), M);
        for (uint32_t u = 0; u < width; ++u) dex[(size_t)nd * width + u] = exps[(size_t)t * width + u];
        dex[(size_t)nd * width + v] = (uint8_t)(e - 1);
        ++nd;
      }
    }
  }
  dbeg[width * width] = nd;
}

// ---- batch inversion: Montgomery's trick per chunk, the chunk's elements a stride of `chunks` apart (coalesced) ------------------------
FPM_HD void ms_batch_inv_item(const MsInv& a, const fpm_mod& M, uint64_t g) {
  const fpm one = fpm_from_words(M.one);
  fpm acc = one;
  uint32_t k = 0;
  for (uint64_t i = g; i < a.count && k < MS_INV_CHUNK; i += a.chunks, ++k) {  // out[i] = the product of the chunk's values before i
    const fpm v = mn_ld(a.in + i);
    mn_st(a.out + i, acc);
    if (!fpm_is_zero(v)) acc = fpm_mul(acc, v, M);
  }
  fpm inv = fpm_pow_limbs(acc, a.pm2.v, M);
  while (k) {
    --k;
    const uint64_t i = g + (uint64_t)k * a.chunks;
    const fpm v = mn_ld(a.in + i);
    if (fpm_is_zero(v)) {
      mn_st(a.out + i, fpm_zero());
    } else {
      mn_st(a.out + i, fpm_mul(mn_ld(a.out + i), inv, M));
      inv = fpm_mul(inv, v, M);
    }
  }
}

// ---- the domain tables ---------------------------------------------------------------------------------------------------------------
// den[0][i] = (x_i - 1)(x_i - r), den[1][i] = x_i^steps - 1 = omega^(i mod ext) - 1, omega = G2^steps
FPM_HD void ms_den_item(const MsTables& t, const fpm_mod& M, uint64_t i) {
  const fpm one = fpm_from_words(M.one), x = ms_x(t.tw, t.log_n, i, M);
  mn_st(t.den + i, fpm_mul(fpm_sub(x, one, M), fpm_sub(x, t.x_last, M), M));
  const uint64_t j = i & (t.ext - 1);
  mn_st(t.den + t.n + i, fpm_sub(ms_x(t.tw, t.log_n, j * t.steps, M), one, M));
}
// after the batch inversion of den into table[0 .. 2n): table[1][i] becomes (x_i - r) / (x_i^steps - 1) in plain form, table[2][i] = x_i
FPM_HD void ms_tables_item(const MsTables& t, const fpm_mod& M, uint64_t i) {
  const fpm x = ms_x(t.tw, t.log_n, i, M);
  const fpm inv = fpm_from_mont(mn_ld(t.table + t.n + i), M);
  mn_st(t.table + t.n + i, fpm_mul(fpm_sub(x, t.x_last, M), inv, M));
  mn_st(t.table + 2 * t.n + i, x);
}

// ---- boundary interpolant (stark.py:81-96, poly_utils.py:397-410) ---------------------------------------------------------------------
// I_c(X) = a + b X through (1, input_c) and (r, output_c), output_c = witness[c][steps - 1]: b = (output - input) / (r - 1), a = input - b
FPM_HD void ms_interp_item(const MsArgs& a, const fpm_mod& M, uint64_t col) {
  const fpm in = fpm_canon(mn_ld(a.inputs + col), M);
  const fpm out = fpm_canon(mn_ld(a.wit + col * a.steps + (a.steps - 1)), M);
  const fpm b = fpm_mul(fpm_sub(out, in, M), a.inv_last_m1, M);
  mn_st(a.iab + 2 * col, fpm_sub(in, b, M));
  mn_st(a.iab + 2 * col + 1, b);
}

// q[c][k] = k p[c][k]: the coefficients of Q_c = X P_c'(X)
FPM_HD void ms_qprep_item(const fpm* pcoef, fpm* q, uint64_t steps, uint64_t g, const fpm_mod& M) {
  const uint64_t k = g & (steps - 1);
  mn_st(q + g, fpm_mul(mn_ld(pcoef + g), fpm_to_mont(fpm_from_u32((uint32_t)k), M), M));
}

// ---- step polynomials (multivariate_polynomial.py:329-338) on Montgomery images ------------------------------------------------------
template <int W>
FPM_HD fpm ms_eval_terms(const fpm* coef, const uint8_t* exps, uint32_t t0, uint32_t t1, const fpm (&P)[W], const fpm_mod& M) {
  fpm acc = fpm_zero();
  for (uint32_t t = t0; t < t1; ++t) {
    const uint8_t* ex = exps + (uint64_t)t * W;
    fpm prod = mn_ld(coef + t);
#pragma unroll
    for (int v = 0; v < W; ++v)
      for (uint32_t k = 0; k < ex[v]; ++k) prod = fpm_mul(prod, P[v], M);
    acc = fpm_add(acc, prod, M);
  }
  return acc;
}

// ---- the trace points x_k = g1^k (domain index k ext): D everywhere, B at x = 1 and x = r, and the constraint check ------------------
template <int W>
FPM_HD void ms_trace_item(const MsArgs& a, const fpm_mod& M, uint64_t g) {
  const uint64_t N = a.n, s = a.steps;
  const uint64_t b = g / s, k = g - b * s;
  const uint64_t i = k * a.ext, knext = (k + 1) & (s - 1);
  const fpm* we = a.wit + b * W * s;
  const fpm* qe = a.q_evals + b * W * s;
  fpm P[W];
#pragma unroll
  for (int v = 0; v < W; ++v) P[v] = fpm_to_mont(mn_ld(we + (uint64_t)v * s + k), M);
  const bool last = knext == 0;
  // D(x) = x C'(x) (x - r) / s off r, D(r) = C(r) r / s: the plain factor that takes the numerator out of Montgomery form
  const fpm scale = fpm_mul(a.inv_steps, last ? a.x_last : fpm_sub(mn_ld(a.xpow + i), a.x_last, M), M);
  for (int c = 0; c < W; ++c) {
    const uint64_t col = (b * W + c) * N;
    const fpm acc = ms_eval_terms<W>(a.term_coef, a.term_exps, a.term_begin[c], a.term_begin[c + 1], P, M);
    const fpm cval = fpm_sub(fpm_to_mont(mn_ld(we + (uint64_t)c * s + knext), M), acc, M);  // witness[c][k+1] - step_c(witness[.][k])
    fpm num;
    if (last) {
      num = cval;
    } else {
      if (!fpm_is_zero(cval)) {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(a.bad + b, 1u);
#else
        a.bad[b] |= 1u;
#endif
      }
      // x C'(x) = Q_c(g1 x) - sum_v (d step_c / d X_v)(P(x)) Q_v(x)
      fpm dsum = fpm_zero();
      for (int v = 0; v < W; ++v) {
        const uint32_t t0 = a.dterm_begin[c * W + v], t1 = a.dterm_begin[c * W + v + 1];
        if (t0 != t1)  // Montgomery times plain: the sum is plain
          dsum = fpm_add(dsum, fpm_mul(ms_eval_terms<W>(a.dterm_coef, a.dterm_exps, t0, t1, P, M), mn_ld(qe + (uint64_t)v * s + k), M), M);
      }
      num = fpm_to_mont(fpm_sub(mn_ld(qe + (uint64_t)c * s + knext), dsum, M), M);
    }
    mn_st(a.d_work + col + i, fpm_mul(num, scale, M));
    if (k == 0 || last) {
      // B(1) = (P'(1) - b) / (1 - r);  B(r) = (P'(r) - b) / (r - 1),  P'(x) = Q(x) / x,  1 / r = g1
      const fpm slope = mn_ld(a.iab + 2 * (b * W + c) + 1);
      const fpm qc = mn_ld(qe + (uint64_t)c * s + k);
      const fpm dp = last ? fpm_mul(qc, a.g1, M) : qc;
      const fpm v = fpm_mul(fpm_sub(dp, slope, M), a.inv_1_m_last, M);
      mn_st(a.b_work + col + i, last ? fpm_neg(v, M) : v);
    }
  }
}

// ---- D off the trace points, B everywhere but x = 1 and x = r: one item per domain point of one proof --------------------------------
template <int W>
FPM_HD void ms_quot_item(const MsArgs& a, const fpm_mod& M, uint64_t b, uint64_t i) {
  const uint64_t N = a.n;
  const fpm* pe = a.p_evals + b * W * N;
  const bool on_trace = (i & (a.ext - 1)) == 0;
  const uint64_t inext = (i + a.ext) & (N - 1);
  const bool special = on_trace && (i == 0 || inext == 0);
  fpm P[W];
#pragma unroll
  for (int v = 0; v < W; ++v) P[v] = fpm_to_mont(mn_ld(pe + (uint64_t)v * N + i), M);
  const fpm fz = mn_ld(a.fz + i), x = mn_ld(a.xpow + i), wz = mn_ld(a.inv_z2 + i);
  for (int c = 0; c < W; ++c) {
    const uint64_t col = (b * W + c) * N;
    if (!on_trace) {  // D = (P_c(g1 x) - step_c(P(x))) (x - r) / (x^s - 1)
      const fpm nxt = fpm_to_mont(mn_ld(pe + (uint64_t)c * N + inext), M);
      const fpm acc = ms_eval_terms<W>(a.term_coef, a.term_exps, a.term_begin[c], a.term_begin[c + 1], P, M);
      mn_st(a.d_work + col + i, fpm_mul(fpm_sub(nxt, acc, M), fz, M));
    }
    if (!special) {  // B = (P_c(x) - a - b x) / ((x - 1)(x - r))
      const fpm* ab = a.iab + 2 * (b * W + c);
      const fpm interp = fpm_add(mn_ld(ab), fpm_mul(mn_ld(ab + 1), x, M), M);
      mn_st(a.b_work + col + i, fpm_mul(fpm_sub(mn_ld(pe + (uint64_t)c * N + i), interp, M), wz, M));
    }
  }
}

// ---- packed Merkle leaves (merkle_tree.py:94-119) ----------------------------------------------------------------------------------
// Leaf x of proof b = P_1(x) .. P_W(x) | D_1(x) .. D_W(x) | B_1(x) .. B_W(x), each 32 bytes big-endian (stark.py:251-257); element e:
FPM_HD void ms_leaf_elem(const MsArgs& a, uint64_t b, uint32_t e, uint64_t x, uint32_t w[8]) {
  const uint32_t W = a.width;
  const fpm* base = e < W ? a.p_evals : e < 2 * W ? a.d_work : a.b_work;
  const uint32_t c = e < W ? e : e < 2 * W ? e - W : e - 2 * W;
  fpm_to_wire_words(mn_ld(base + (b * W + c) * a.n + x), w);
}
// row i of permute4 of tree b: the two leaf pairs (leaf A = point i + 2 s q, leaf B = point i + (2 s + 1) q, one message of 3 W BLAKE2s
// blocks) and their parent.  nodes: [batch][2n] x 32 B, only [0, n) is written: the leaves stay in the evaluation arrays.
template <bool ASM_ROUNDS>  // blake2s.cuh's throughput rounds, or the C++ rounds (the same function on the host)
FPM_HD void ms_leaf_row_item(const MsArgs& a, uint32_t* nodes, uint64_t b, uint64_t i) {
  const uint64_t N = a.n, q = N >> 2;
  const uint32_t k = 3 * a.width;
  uint32_t* tree = nodes + b * 2 * N * 8;
  b2digest d[2];
  for (int s = 0; s < 2; ++s) {
    const uint64_t la = i + (uint64_t)(2 * s) * q, lb = i + (uint64_t)(2 * s + 1) * q;
    b2_init(d[s].h);
    for (uint32_t blk = 0; blk < k; ++blk) {
      uint32_t m[16];
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const uint32_t e = 2 * blk + half;
        ms_leaf_elem(a, b, e < k ? e : e - k, e < k ? la : lb, m + 8 * half);
      }
      b2_compress<ASM_ROUNDS>(d[s].h, m, 64 * (blk + 1), blk + 1 == k);
    }
    mf_st8(tree + (N / 2 + 2 * i + s) * 8, d[s].h);
  }
  const b2digest top = b2_hash_pair<ASM_ROUNDS>(d[0].h, d[1].h);
  mf_st8(tree + (N / 4 + i) * 8, top.h);
  if (i == 0) {
    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    mf_st8(tree, z);  // nodes[0]: the reference keeps b'' there
  }
}

// ---- Fiat-Shamir scalars of the linear combination (stark.py:106-177) ----------------------------------------------------------------
// k_t = int(blake(m_root + b"0x0<t+1>")) mod p; with c = (G2^steps)^(n-1) -- `powers[i]` in the reference reads the loop variable left
// over from building the list, the last power --  l = sum_j (1 + lk_j c) (D_j + (k1 + k2 c) P_j + (k3 + k4 c) B_j),
// lk = get_pseudorandom_ks(m_root, width).  One item per proof writes alpha_j, alpha_j beta, alpha_j gamma in Montgomery form.
FPM_HD void ms_scalars_item(const uint32_t* mnodes, uint64_t tree_words, uint32_t width, const fpm& cpow, fpm* scal, uint64_t b,
                            const fpm_mod& M) {
  auto k_of = [&](uint32_t digit) {
    uint32_t m[16];
    mf_ld8(mnodes + b * tree_words + 8, m);
    for (int j = 9; j < 16; ++j) m[j] = 0;
    m[8] = 0x30u | (0x78u << 8) | (0x30u << 16) | ((0x30u + digit) << 24);  // "0x0<digit>"
    const b2digest d = b2_hash_short<false>(m, 36);
    return fpm_to_mont(fpm_from_wire_words(d.h), M);  // the 256-bit hash value modulo p
  };
  const fpm k1 = k_of(1), k2 = k_of(2), k3 = k_of(3), k4 = k_of(4);
  const fpm beta = fpm_add(k1, fpm_mul(k2, cpow, M), M), gamma = fpm_add(k3, fpm_mul(k4, cpow, M), M);
  for (uint32_t j = 0; j < width; ++j) {
    const fpm lk = k_of(width > 4 ? j : j + 1);  // stark.py:118-125: the series "0x01".. up to four, "0x00".. from five on
    const fpm alpha = fpm_add(fpm_from_words(M.one), fpm_mul(lk, cpow, M), M);
    fpm* o = scal + (b * width + j) * 3;
    mn_st(o, alpha);
    mn_st(o + 1, fpm_mul(alpha, beta, M));
    mn_st(o + 2, fpm_mul(alpha, gamma, M));
  }
}

// l[b][x] = sum_j alpha_j D_j[x] + (alpha_j beta) P_j[x] + (alpha_j gamma) B_j[x] (stark.py:128-177), plain and canonical
FPM_HD void ms_lincomb_item(const MsArgs& a, const fpm* scal, fpm* l, const fpm_mod& M, uint64_t b, uint64_t x) {
  fpm acc = fpm_zero();
  for (uint32_t j = 0; j < a.width; ++j) {
    const uint64_t col = (b * a.width + j) * a.n + x;
    const fpm* sc = scal + (b * a.width + j) * 3;
    const fpm v0 = mn_ld(a.d_work + col), v1 = mn_ld(a.p_evals + col), v2 = mn_ld(a.b_work + col);
    acc = fpm_add(acc, fpm_mul(v0, mn_ld(sc), M), M);
    acc = fpm_add(acc, fpm_mul(v1, mn_ld(sc + 1), M), M);
    acc = fpm_add(acc, fpm_mul(v2, mn_ld(sc + 2), M), M);
  }
  mn_st(l + b * a.n + x, acc);
}

// ---- spot checks (stark.py:390-402) ------------------------------------------------------------------------------------------------
// proof[b] = m_root | l_root | for each sampled pos: mk_branch(mtree, pos) | mk_branch(mtree, pos + ext) | mk_branch(ltree, pos).
// A packed branch = leaf (k values) | sibling leaf (k values) | log2(n) - 1 nodes; an l branch = log2(n) + 1 nodes.  One item per 32-byte slot.
struct MsGather {
  const uint32_t* mnodes;  // [batch][2n][8]
  const uint32_t* lnodes;  // [batch][2n][8]
  const fpm* lvals;        // [batch][n]
  const uint32_t* ys;      // [batch][samples]
  uint32_t samples, lg;
  uint8_t* proof;
  uint64_t stride;
};
FPM_HD uint64_t ms_gather_per_proof(uint32_t width, uint32_t samples, uint32_t lg) {
  return 2 + (uint64_t)samples * (2 * (6 * width + (lg - 1)) + (lg + 1));
}
FPM_HD void ms_gather_item(const MsArgs& a, const MsGather& ga, uint64_t g) {
  const uint32_t k = 3 * a.width, lg = ga.lg;
  const uint32_t pb = 2 * k + (lg - 1), lb = lg + 1, per_sample = 2 * pb + lb;
  const uint64_t per_proof = 2 + (uint64_t)ga.samples * per_sample;
  const uint64_t b = g / per_proof;
  uint64_t r = g - b * per_proof;
  uint32_t* out = reinterpret_cast<uint32_t*>(ga.proof + b * ga.stride) + 8 * r;
  const uint64_t n = a.n, q = n >> 2;
  const uint32_t* mt = ga.mnodes + b * 2 * n * 8;
  const uint32_t* lt = ga.lnodes + b * 2 * n * 8;
  uint32_t w[8];
  if (r < 2) {
    mf_ld8((r == 0 ? mt : lt) + 8, w);
    mf_st8(out, w);
    return;
  }
  r -= 2;
  const uint32_t s = (uint32_t)(r / per_sample);
  uint32_t slot = (uint32_t)(r - (uint64_t)s * per_sample);
  const uint64_t pos = ga.ys[b * ga.samples + s] & (n - 1);  // the sampler's values are below n; the mask keeps every address in bounds
  if (slot < 2 * pb) {
    const uint32_t which = slot / pb;
    slot -= which * pb;
    const uint64_t x = which ? ((pos + a.ext) & (n - 1)) : pos;
    const uint64_t idx = x / q + 4 * (x % q);  // get_index_in_permuted (merkle_tree.py:26-33)
    if (slot < 2 * k) {
      const uint64_t pi = slot < k ? idx : (idx ^ 1);  // the leaf, then its sibling leaf
      const uint64_t leaf = (pi & 3) * q + (pi >> 2);  // back to the natural position
      ms_leaf_elem(a, b, slot < k ? slot : slot - k, leaf, w);
    } else {
      const uint32_t lev = slot - 2 * k + 1;  // branch entry lev + 1: tree[((n + idx) >> lev) ^ 1]
      mf_ld8(mt + (((n + idx) >> lev) ^ 1) * 8, w);
    }
  } else {
    slot -= 2 * pb;
    const uint64_t pi = pos / q + 4 * (pos % q);
    if (slot <= 1) {  // the leaf and its sibling leaf: the l tree's leaf level is not materialised either
      const uint64_t ps = pi ^ slot;
      fpm_to_wire_words(mn_ld(ga.lvals + b * n + (ps & 3) * q + (ps >> 2)), w);
    } else {
      mf_ld8(lt + (((n + pi) >> (slot - 1)) ^ 1) * 8, w);
    }
  }
  mf_st8(out, w);
}
