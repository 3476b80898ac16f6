// mod64stark_items.cuh -- the middle of STARK.mk_proof (stark.py:233-279) over any prime modulus below 2^64 on packed 64-bit words
// (fp64m.cuh): the per-item bodies of the boundary interpolant, X P'(X), the domain tables and their batch inversion, the quotients D and
// B, the packed Merkle leaves, the Fiat-Shamir scalars, the linear combination and the spot-check gather.  mod64stark.hip wraps them in
// kernels, api_mod64stark.hip drives them; tests/native/mod64stark_host.cpp walks the same functions on the host over the same grids.
// The proof bytes are modstark_items.cuh's over the same modulus (its header has the algorithm): only the width of a stored value differs.
//
// Forms.  Every array between the kernels -- witness, inputs, P, Q, D, B, l -- holds PLAIN 8-byte words, and all but the caller's witness
// and inputs are CANONICAL (below p): an element is hashed and written as 24 zero bytes and the word big-endian (m6_wire_words), never
// reduced modulo anything but p.  Multipliers are in Montgomery form, so that f64_mul(plain, Montgomery) is plain and canonical: the term
// coefficients, the scalars, x_i, 1 / Z2(x_i).  The step polynomials are evaluated on Montgomery images of the point's P values
// (f64_to_mont takes any 64-bit word, which is also where a witness word at or above p is reduced); their result meets the PLAIN table
// (x - r) / (x^s - 1) in the one product that leaves Montgomery form.  f64_mul wants a canonical SECOND operand: every product below has
// a table entry, a scalar or an f64_* result there.  No address depends on a field value.
// x_i = G2^i comes from the n-point transform's own lo | hi table (one product), once per (p, steps, ext): the tables keep it as xpow.
#pragma once
#include "mod64fri_items.cuh"

constexpr uint32_t M6S_WG = 256;        // threads per workgroup
constexpr uint32_t M6S_MAX_WIDTH = 9;   // SHK_STARK_MAX_WIDTH
constexpr uint32_t M6S_MAX_TERMS = 256; // SHK_STARK_MAX_TERMS
// values per batch-inversion item: one a^(p-2) power (64 squarings + up to 64 products, ~96) per chunk, 6 products per value beside the
// trick's own 3 (the 256-bit path pays ~380 per 32 values, 12 per value), and twice the threads of a chunk of 32
constexpr uint32_t M6S_INV_CHUNK = 16;

struct M6sArgs {
  const uint64_t* p_evals;  // [batch * width][n]      trace polynomials on the G2 domain
  uint64_t* d_work;         // [batch * width][n]      D
  uint64_t* b_work;         // [batch * width][n]      B
  const uint64_t* q_evals;  // [batch * width][steps]  Q_c = X P_c'(X) on G1
  const uint64_t* wit;      // [batch * width][steps]  the witness, any 64-bit words
  const uint64_t* inputs;   // [batch * width]         any 64-bit words
  uint64_t* iab;            // [batch * width][2]      boundary interpolant a + b X
  uint64_t n, steps;
  uint32_t ext, width, batch;
  const uint64_t* inv_z2;   // [n] 1 / ((x_i - 1)(x_i - r)), Montgomery form, 0 at the two roots
  const uint64_t* fz;       // [n] (x_i - r) / (x_i^steps - 1), PLAIN, 0 on the trace points
  const uint64_t* xpow;     // [n] x_i, Montgomery form
  uint64_t x_last, g1, inv_last_m1, inv_1_m_last;  // r, 1 / r, 1 / (r - 1), 1 / (1 - r): Montgomery form
  uint64_t inv_steps;       // 1 / steps, plain
  uint32_t* bad;            // [batch] raised when a transition constraint of proof b fails on the trace
  // step polynomials: term t = coef[t] prod_v X_v^exps[t][v] (rows of `width` bytes), terms of dimension c: [term_begin[c], term_begin[c+1]);
  // d step_c / d X_v = derivative terms [dterm_begin[c width + v], dterm_begin[c width + v + 1]).  Coefficients in Montgomery form.
  const uint64_t* term_coef;
  const uint8_t* term_exps;
  uint32_t term_begin[M6S_MAX_WIDTH + 1];
  const uint64_t* dterm_coef;
  const uint8_t* dterm_exps;
  const uint32_t* dterm_begin;
};

// the batch inversion of `count` Montgomery-form words: out[i] = in[i]^-1 (Montgomery form), 0 for in[i] = 0; in != out
struct M6sInv {
  const uint64_t* in;
  uint64_t* out;
  uint64_t count, chunks;  // chunks = ceil(count / M6S_INV_CHUNK); item g owns i = g + k chunks
};

// the domain tables of (p, steps, ext): den is [2][n], table [3][n]; see m6s_den_item and m6s_tables_item
struct M6sTables {
  uint64_t* den;            // scratch: (x_i - 1)(x_i - r) | x_i^steps - 1, Montgomery form
  uint64_t* table;          // inv_z2 | fz | xpow
  const uint64_t *lo, *hi;  // the n-point transform's tables: G2^e = hi[e >> log_h] lo[e & (2^log_h - 1)], Montgomery form
  uint64_t n, steps;
  uint32_t ext, log_h;
  uint64_t x_last;          // Montgomery form
};

// G2^e in Montgomery form, e < n
F64_HD uint64_t m6s_x(const M6sTables& t, const f64_mod& M, uint64_t e) {
  return f64_mul(t.hi[e >> t.log_h], t.lo[e & ((1ull << t.log_h) - 1)], M);
}

// ---- host side of a call (no device): G2, the term image -----------------------------------------------------------------------------
// G2 = 7^((p - 1) // 2^lg) in Montgomery form (stark.py:205)
inline uint64_t m6s_g2(const f64_mod& M, int lg) { return f64_pow(f64_to_mont(7u, M), (M.p - 1) >> lg, M); }
// a 32-byte wire value (big-endian) modulo p, canonical
inline uint64_t m6s_from_wire(const uint8_t b[32], const f64_mod& M) {
  uint32_t limbs[8];
  for (int i = 0; i < 8; ++i) {
    const uint8_t* s = b + 4 * (7 - i);
    limbs[i] = ((uint32_t)s[0] << 24) | ((uint32_t)s[1] << 16) | ((uint32_t)s[2] << 8) | s[3];
  }
  return f64_from_limbs(limbs, M);
}
// MultivariatePolynomial.degree over every term (multivariate_polynomial.py:111-117)
inline uint32_t m6s_terms_degree(const uint8_t* exps, uint32_t width, uint64_t total) {
  uint32_t degree = 0;
  for (uint64_t t = 0; t < total; ++t) {
    uint32_t sum = 0;
    for (uint32_t v = 0; v < width; ++v) sum += exps[t * width + v];
    if (sum > degree) degree = sum;
  }
  return degree;
}
// The terms and their partial derivatives as the kernels read them (ms_terms_build on words): cf[total], dcf / dex rows for up to
// total * width derivative terms, ex = the exponent rows, dbeg[width * width + 1], begin[width + 1].  Coefficients are 32-byte wire
// values, reduced modulo p here.
inline void m6s_terms_build(const f64_mod& M, uint32_t width, const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts,
                            uint64_t total, uint64_t* cf, uint64_t* dcf, uint8_t* ex, uint8_t* dex, uint32_t* dbeg, uint32_t* begin) {
  for (uint64_t t = 0; t < total; ++t) cf[t] = f64_to_mont(m6s_from_wire(coefs + 32 * t, M), M);
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
        dcf[nd] = f64_mul(cf[t], f64_to_mont(e, M), M);
        for (uint32_t u = 0; u < width; ++u) dex[(size_t)nd * width + u] = exps[(size_t)t * width + u];
        dex[(size_t)nd * width + v] = (uint8_t)(e - 1);
        ++nd;
      }
    }
  }
  dbeg[width * width] = nd;
}

// ---- batch inversion: Montgomery's trick per chunk, the chunk's elements a stride of `chunks` apart (coalesced) ------------------------
F64_HD void m6s_batch_inv_item(const M6sInv& a, const f64_mod& M, uint64_t g) {
  uint64_t acc = M.one;
  uint32_t k = 0;
  for (uint64_t i = g; i < a.count && k < M6S_INV_CHUNK; i += a.chunks, ++k) {  // out[i] = the product of the chunk's values before i
    const uint64_t v = a.in[i];
    a.out[i] = acc;
    if (v) acc = f64_mul(acc, v, M);
  }
  uint64_t inv = f64_pow(acc, M.p - 2, M);  // Fermat: the modulus is prime by contract
  while (k) {
    --k;
    const uint64_t i = g + (uint64_t)k * a.chunks;
    const uint64_t v = a.in[i];
    if (!v) {
      a.out[i] = 0;
    } else {
      a.out[i] = f64_mul(a.out[i], inv, M);
      inv = f64_mul(inv, v, M);
    }
  }
}

// ---- the domain tables ---------------------------------------------------------------------------------------------------------------
// den[0][i] = (x_i - 1)(x_i - r), den[1][i] = x_i^steps - 1 = omega^(i mod ext) - 1, omega = G2^steps
F64_HD void m6s_den_item(const M6sTables& t, const f64_mod& M, uint64_t i) {
  const uint64_t x = m6s_x(t, M, i);
  t.den[i] = f64_mul(f64_sub(x, M.one, M), f64_sub(x, t.x_last, M), M);
  const uint64_t j = i & (t.ext - 1);
  t.den[t.n + i] = f64_sub(m6s_x(t, M, j * t.steps), M.one, M);
}
// after the batch inversion of den into table[0 .. 2n): table[1][i] becomes (x_i - r) / (x_i^steps - 1) in plain form, table[2][i] = x_i
F64_HD void m6s_tables_item(const M6sTables& t, const f64_mod& M, uint64_t i) {
  const uint64_t x = m6s_x(t, M, i);
  const uint64_t inv = f64_from_mont(t.table[t.n + i], M);
  t.table[t.n + i] = f64_mul(f64_sub(x, t.x_last, M), inv, M);
  t.table[2 * t.n + i] = x;
}

// ---- boundary interpolant (stark.py:81-96, poly_utils.py:397-410) ---------------------------------------------------------------------
// I_c(X) = a + b X through (1, input_c) and (r, output_c), output_c = witness[c][steps - 1]: b = (output - input) / (r - 1), a = input - b
F64_HD void m6s_interp_item(const M6sArgs& a, const f64_mod& M, uint64_t col) {
  const uint64_t in = f64_canon(a.inputs[col], M);
  const uint64_t out = f64_canon(a.wit[col * a.steps + (a.steps - 1)], M);
  const uint64_t b = f64_mul(f64_sub(out, in, M), a.inv_last_m1, M);
  a.iab[2 * col] = f64_sub(in, b, M);
  a.iab[2 * col + 1] = b;
}

// q[c][k] = k p[c][k]: the coefficients of Q_c = X P_c'(X)
F64_HD void m6s_qprep_item(const uint64_t* pcoef, uint64_t* q, uint64_t steps, uint64_t g, const f64_mod& M) {
  q[g] = f64_mul(pcoef[g], f64_to_mont(g & (steps - 1), M), M);
}

// ---- step polynomials (multivariate_polynomial.py:329-338) on Montgomery images ------------------------------------------------------
template <int W>
F64_HD uint64_t m6s_eval_terms(const uint64_t* coef, const uint8_t* exps, uint32_t t0, uint32_t t1, const uint64_t (&P)[W],
                               const f64_mod& M) {
  uint64_t acc = 0;
  for (uint32_t t = t0; t < t1; ++t) {
    const uint8_t* ex = exps + (uint64_t)t * W;
    uint64_t prod = coef[t];
#pragma unroll
    for (int v = 0; v < W; ++v)
      for (uint32_t k = 0; k < ex[v]; ++k) prod = f64_mul(prod, P[v], M);
    acc = f64_add(acc, prod, M);
  }
  return acc;
}

// ---- the trace points x_k = g1^k (domain index k ext): D everywhere, B at x = 1 and x = r, and the constraint check ------------------
template <int W>
F64_HD void m6s_trace_item(const M6sArgs& a, const f64_mod& M, uint64_t g) {
  const uint64_t N = a.n, s = a.steps;
  const uint64_t b = g / s, k = g - b * s;
  const uint64_t i = k * a.ext, knext = (k + 1) & (s - 1);
  const uint64_t* we = a.wit + b * W * s;
  const uint64_t* qe = a.q_evals + b * W * s;
  uint64_t P[W];
#pragma unroll
  for (int v = 0; v < W; ++v) P[v] = f64_to_mont(we[(uint64_t)v * s + k], M);
  const bool last = knext == 0;
  // D(x) = x C'(x) (x - r) / s off r, D(r) = C(r) r / s: the plain factor that takes the numerator out of Montgomery form
  const uint64_t scale = f64_mul(a.inv_steps, last ? a.x_last : f64_sub(a.xpow[i], a.x_last, M), M);
  for (int c = 0; c < W; ++c) {
    const uint64_t col = (b * W + c) * N;
    const uint64_t acc = m6s_eval_terms<W>(a.term_coef, a.term_exps, a.term_begin[c], a.term_begin[c + 1], P, M);
    const uint64_t cval = f64_sub(f64_to_mont(we[(uint64_t)c * s + knext], M), acc, M);  // witness[c][k+1] - step_c(witness[.][k])
    uint64_t num;
    if (last) {
      num = cval;
    } else {
      if (cval) {
#if defined(__HIP_DEVICE_COMPILE__)
        atomicOr(a.bad + b, 1u);
#else
        a.bad[b] |= 1u;
#endif
      }
      // x C'(x) = Q_c(g1 x) - sum_v (d step_c / d X_v)(P(x)) Q_v(x)
      uint64_t dsum = 0;
      for (int v = 0; v < W; ++v) {
        const uint32_t t0 = a.dterm_begin[c * W + v], t1 = a.dterm_begin[c * W + v + 1];
        if (t0 != t1)  // Montgomery times plain: the sum is plain
          dsum = f64_add(dsum, f64_mul(m6s_eval_terms<W>(a.dterm_coef, a.dterm_exps, t0, t1, P, M), qe[(uint64_t)v * s + k], M), M);
      }
      num = f64_to_mont(f64_sub(qe[(uint64_t)c * s + knext], dsum, M), M);
    }
    a.d_work[col + i] = f64_mul(num, scale, M);
    if (k == 0 || last) {
      // B(1) = (P'(1) - b) / (1 - r);  B(r) = (P'(r) - b) / (r - 1),  P'(x) = Q(x) / x,  1 / r = g1
      const uint64_t slope = a.iab[2 * (b * W + c) + 1];
      const uint64_t qc = qe[(uint64_t)c * s + k];
      const uint64_t dp = last ? f64_mul(qc, a.g1, M) : qc;
      const uint64_t v = f64_mul(f64_sub(dp, slope, M), a.inv_1_m_last, M);
      a.b_work[col + i] = last ? f64_neg(v, M) : v;
    }
  }
}

// ---- D off the trace points, B everywhere but x = 1 and x = r: one item per domain point of one proof --------------------------------
// lanes walk i: every load and store below is one 8-byte word per lane at consecutive addresses (the i + ext read a shifted run)
template <int W>
F64_HD void m6s_quot_item(const M6sArgs& a, const f64_mod& M, uint64_t b, uint64_t i) {
  const uint64_t N = a.n;
  const uint64_t* pe = a.p_evals + b * W * N;
  const bool on_trace = (i & (a.ext - 1)) == 0;
  const uint64_t inext = (i + a.ext) & (N - 1);
  const bool special = on_trace && (i == 0 || inext == 0);
  uint64_t P[W];
#pragma unroll
  for (int v = 0; v < W; ++v) P[v] = f64_to_mont(pe[(uint64_t)v * N + i], M);
  const uint64_t fz = a.fz[i], x = a.xpow[i], wz = a.inv_z2[i];
  for (int c = 0; c < W; ++c) {
    const uint64_t col = (b * W + c) * N;
    if (!on_trace) {  // D = (P_c(g1 x) - step_c(P(x))) (x - r) / (x^s - 1)
      const uint64_t nxt = f64_to_mont(pe[(uint64_t)c * N + inext], M);
      const uint64_t acc = m6s_eval_terms<W>(a.term_coef, a.term_exps, a.term_begin[c], a.term_begin[c + 1], P, M);
      a.d_work[col + i] = f64_mul(f64_sub(nxt, acc, M), fz, M);
    }
    if (!special) {  // B = (P_c(x) - a - b x) / ((x - 1)(x - r))
      const uint64_t* ab = a.iab + 2 * (b * W + c);
      const uint64_t interp = f64_add(ab[0], f64_mul(ab[1], x, M), M);
      a.b_work[col + i] = f64_mul(f64_sub(pe[(uint64_t)c * N + i], interp, M), wz, M);
    }
  }
}

// ---- packed Merkle leaves (merkle_tree.py:94-119) ----------------------------------------------------------------------------------
// Leaf x of proof b = P_1(x) .. P_W(x) | D_1(x) .. D_W(x) | B_1(x) .. B_W(x), each 24 zero bytes and the word big-endian; element e:
F64_HD void m6s_leaf_elem(const M6sArgs& a, uint64_t b, uint32_t e, uint64_t x, uint32_t w[8]) {
  const uint32_t W = a.width;
  const uint64_t* base = e < W ? a.p_evals : e < 2 * W ? a.d_work : a.b_work;
  const uint32_t c = e < W ? e : e < 2 * W ? e - W : e - 2 * W;
  m6_wire_words(base[(b * W + c) * a.n + x], w);
}
// row i of permute4 of tree b: the two leaf pairs (leaf A = point i + 2 s q, leaf B = point i + (2 s + 1) q, one message of 3 W BLAKE2s
// blocks) and their parent.  nodes: [batch][2n] x 32 B, only [0, n) is written: the leaves stay in the evaluation arrays.  Lanes walk i:
// each of the four strided leaf reads is a run of consecutive words across the lanes.
template <bool ASM_ROUNDS>  // blake2s.cuh's throughput rounds, or the C++ rounds (the same function on the host)
F64_HD void m6s_leaf_row_item(const M6sArgs& a, uint32_t* nodes, uint64_t b, uint64_t i) {
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
        m6s_leaf_elem(a, b, e < k ? e : e - k, e < k ? la : lb, m + 8 * half);
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
// k_t = int(blake(m_root + b"0x0<t+1>")) mod p: the 256-bit hash is byte-swapped into limbs and reduced by f64_from_limbs, as the packed
// fold reduces its challenge.  With c = (G2^steps)^(n-1), l = sum_j (1 + lk_j c) (D_j + (k1 + k2 c) P_j + (k3 + k4 c) B_j),
// lk = get_pseudorandom_ks(m_root, width).  One item per proof writes alpha_j, alpha_j beta, alpha_j gamma in Montgomery form.
F64_HD void m6s_scalars_item(const uint32_t* mnodes, uint64_t tree_words, uint32_t width, uint64_t cpow, uint64_t* scal, uint64_t b,
                             const f64_mod& M) {
  auto k_of = [&](uint32_t digit) {
    uint32_t m[16];
    mf_ld8(mnodes + b * tree_words + 8, m);
    for (int j = 9; j < 16; ++j) m[j] = 0;
    m[8] = 0x30u | (0x78u << 8) | (0x30u << 16) | ((0x30u + digit) << 24);  // "0x0<digit>"
    const b2digest d = b2_hash_short<false>(m, 36);
    uint32_t limbs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) limbs[i] = __builtin_bswap32(d.h[7 - i]);
    return f64_to_mont(f64_from_limbs(limbs, M), M);
  };
  const uint64_t k1 = k_of(1), k2 = k_of(2), k3 = k_of(3), k4 = k_of(4);
  const uint64_t beta = f64_add(k1, f64_mul(k2, cpow, M), M), gamma = f64_add(k3, f64_mul(k4, cpow, M), M);
  for (uint32_t j = 0; j < width; ++j) {
    const uint64_t lk = k_of(width > 4 ? j : j + 1);  // stark.py:118-125: the series "0x01".. up to four, "0x00".. from five on
    const uint64_t alpha = f64_add(M.one, f64_mul(lk, cpow, M), M);
    uint64_t* o = scal + (b * width + j) * 3;
    o[0] = alpha;
    o[1] = f64_mul(alpha, beta, M);
    o[2] = f64_mul(alpha, gamma, M);
  }
}

// l[b][x] = sum_j alpha_j D_j[x] + (alpha_j beta) P_j[x] + (alpha_j gamma) B_j[x] (stark.py:128-177), plain and canonical
F64_HD void m6s_lincomb_item(const M6sArgs& a, const uint64_t* scal, uint64_t* l, const f64_mod& M, uint64_t b, uint64_t x) {
  uint64_t acc = 0;
  for (uint32_t j = 0; j < a.width; ++j) {
    const uint64_t col = (b * a.width + j) * a.n + x;
    const uint64_t* sc = scal + (b * a.width + j) * 3;
    acc = f64_add(acc, f64_mul(a.d_work[col], sc[0], M), M);
    acc = f64_add(acc, f64_mul(a.p_evals[col], sc[1], M), M);
    acc = f64_add(acc, f64_mul(a.b_work[col], sc[2], M), M);
  }
  l[b * a.n + x] = acc;
}

// ---- spot checks (stark.py:390-402) ------------------------------------------------------------------------------------------------
// proof[b] = m_root | l_root | for each sampled pos: mk_branch(mtree, pos) | mk_branch(mtree, pos + ext) | mk_branch(ltree, pos).
// A packed branch = leaf (k values) | sibling leaf (k values) | log2(n) - 1 nodes; an l branch = log2(n) + 1 nodes.  One item per 32-byte
// slot: leaf slots are expanded from words to wire values, node slots are copied.
struct M6sGather {
  const uint32_t* mnodes;  // [batch][2n][8]
  const uint32_t* lnodes;  // [batch][2n][8]
  const uint64_t* lvals;   // [batch][n]
  const uint32_t* ys;      // [batch][samples]
  uint32_t samples, lg;
  uint8_t* proof;
  uint64_t stride;
};
F64_HD uint64_t m6s_gather_per_proof(uint32_t width, uint32_t samples, uint32_t lg) {
  return 2 + (uint64_t)samples * (2 * (6 * width + (lg - 1)) + (lg + 1));
}
F64_HD void m6s_gather_item(const M6sArgs& a, const M6sGather& ga, uint64_t g) {
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
      m6s_leaf_elem(a, b, slot < k ? slot : slot - k, leaf, w);
    } else {
      const uint32_t lev = slot - 2 * k + 1;  // branch entry lev + 1: tree[((n + idx) >> lev) ^ 1]
      mf_ld8(mt + (((n + idx) >> lev) ^ 1) * 8, w);
    }
  } else {
    slot -= 2 * pb;
    const uint64_t pi = pos / q + 4 * (pos % q);
    if (slot <= 1) {  // the leaf and its sibling leaf: the l tree's leaf level is not materialised either
      const uint64_t ps = pi ^ slot;
      m6_wire_words(ga.lvals[b * n + (ps & 3) * q + (ps >> 2)], w);
    } else {
      mf_ld8(lt + (((n + pi) >> (slot - 1)) ^ 1) * 8, w);
    }
  }
  mf_st8(out, w);
}
