// mod64witness_items.cuh -- the per-lane step of the witness generator over any odd modulus 3 <= p < 2^64 on packed 64-bit words
// (mod64witness.hip): modwitness_items.cuh on the one-word Montgomery arithmetic of fp64m.cuh.  A trace needs only ring operations -- no
// root of unity, no inverse -- so composite moduli (15, 2^64 - 1) and the moduli the provers refuse (BabyBear, KoalaBear) are fine here.
//
// The decomposition is witness_items.cuh's, unchanged: WiRow, wi_pack_row, WiPlan, wi_split and wi_plan do not depend on the field and
// are used as they are; only the arithmetic bodies have m6w_* forms, with the modulus block passed down by reference from the kernel
// argument.  Semantics are the reference's (multivariate_polynomial.py:329-338): X^0 = 1 also at X = 0 (a factor with exponent 0 is
// never in a row's factor queue), a term without factors is its coefficient, a dimension without terms is 0.
//
// Forms.  The state P[] lives in registers in Montgomery form, canonical: row 0 is f64_to_mont(input word), which reduces ANY 64-bit
// input, at or above p included, and the coefficients arrive in Montgomery form, canonical (Mod64TermLayout::coef).  d_witness ends PLAIN
// and canonical: what sh_dev_mod64_stark_prove reads.
// Operand order.  f64_mul wants a canonical SECOND operand: every product below has an f64_* result (the state, a power, a running term),
// a coefficient or a constant of the modulus block there, never a raw input word -- the one raw word of the path, the input, is the FIRST
// operand of f64_to_mont's product with R^2.  tests/native/mod64witness_host.cpp runs inputs of 2^64 - 1 and x + p over p = 3.
// Between the state and d_witness there are two store forms (M6wStore, the twins of MwiStore):
//   M6W_PASS   (default) the sequential kernel stores its rows as they are, Montgomery form, and one element-wise grid-wide pass
//              (m6w_finish) converts [batch][width][steps] in place after the last slice; a resumed slice reads Montgomery values.
//   M6W_INLINE the kernel converts on the store path (one f64_from_mont per stored column per step, shared by the group's lanes) and a
//              resumed slice converts its starting row back (f64_to_mont); there is no pass.
// STARKHIP_WITNESS_STORE=inline selects M6W_INLINE, as for the generic path.  A lone wave is bound by its own instruction stream, so
// M6W_INLINE's products are paid in full; tools/mod64_witness_time.py times both (profiles/r20_mod64_witness.json, EXPERIMENTS.md); the
// numbers are quoted at M6W_SLICE_PRODUCTS below.
// Every function is __host__ __device__: tests/native/mod64witness_host.cpp runs the same decomposition serially.
#pragma once
#include <stdint.h>

#include "fp64m.cuh"
#include "witness_items.cuh"

// Sequential products per dispatch of the packed-word kernel (the budget of this path; WI_SLICE_PRODUCTS and MWI_SLICE_PRODUCTS are the
// other two).  mod64_witness_kernel measures (tools/mod64_witness_time.py, profiles/r20_mod64_witness.json; Goldilocks, and
// 2^64 - 1835007 within 0.2 % of it) 0.57 us per counted product on MiMC (2 per step, 75 ms per 65535 steps at 64 units; 0.61 us for a
// single unit) and 0.62 us on the 256-term width-9 system at G = 16 (56 per step, 35 us per step), against 1.9 and 3.8 us for
// mod_witness_kernel plus the two sh_dev_mod64_from_limbs passes in the same run: 3.3x and 6.2x.  2^14 products are 9.4 - 10.1 ms per
// dispatch: both systems lie inside the 9 - 14 ms band the other two budgets aim at (2^13: 4.7 - 5.0 ms, 2^15: 18.7 - 20.2 ms).
// M6W_INLINE in the same run: 0.62 us per product on MiMC (81 ms, + 7.6 %: its two conversion products per step beside the step's two
// are paid in full) and 0.62 us on the 256-term system (143.0 against 141.3 ms: 9 conversions shared by 16 lanes beside 56 products, a
// difference inside the 141.1 - 143.7 ms spread of the forced G = 16 runs of the two forms).  M6W_PASS is the default: it is faster
// where the forms differ, and its closing pass is inside the 75 ms.
constexpr uint64_t M6W_SLICE_PRODUCTS = 1u << 14;

enum M6wStore { M6W_PASS = 0, M6W_INLINE = 1 };

// Mod64TermLayout has no "coefficient == 1" flag: a coefficient is canonical Montgomery form (f64_to_mont of the wire value reduced
// modulo p, so a stored 1 + p counts as 1), and 1 is M.one
WI_HD bool m6w_unit(uint64_t coef, const f64_mod& M) { return coef == M.one; }

// P[v] / Q[c] for a lane-dependent index without indexing the register array (witness_items.cuh: wi_blend)
WI_HD void m6w_blend(uint64_t& r, uint64_t x, bool take) {
  const uint64_t m = 0ull - (uint64_t)take;
  r = (x & m) | (r & ~m);
}
template <int W>
WI_HD uint64_t m6w_select(const uint64_t (&P)[W], uint32_t v) {
  uint64_t r = P[0];
#pragma unroll
  for (int u = 1; u < W; ++u) m6w_blend(r, P[u], v == (uint32_t)u);
  return r;
}
template <int W>
WI_HD void m6w_put(uint64_t (&Q)[W], uint32_t c, uint64_t x) {
#pragma unroll
  for (int u = 0; u < W; ++u) m6w_blend(Q[u], x, c == (uint32_t)u);
}

// x^e, e >= 1, square-and-multiply from the top bit: the products wi_term_products counts.  x is canonical (a state value)
WI_HD uint64_t m6w_pow(uint64_t x, uint32_t e, const f64_mod& M) {
  uint64_t r = x;
#pragma unroll 1
  for (int i = 30 - __builtin_clz(e); i >= 0; --i) {
    r = f64_mul(r, r, M);
    if ((e >> i) & 1u) r = f64_mul(r, x, M);
  }
  return r;
}

// coef * prod_v P[v]^e_v; a coefficient of 1 is not multiplied in (and is the value of a term without factors)
template <int W>
WI_HD uint64_t m6w_term(const WiRow& row, uint64_t coef, const uint64_t (&P)[W], const f64_mod& M) {
  bool have = ((row.lo >> 4) & 1u) == 0;
  uint32_t nf = (uint32_t)(row.lo >> 5) & 15u;
  uint64_t lo = (row.lo >> 9) | (row.hi << 55), hi = row.hi >> 9;  // the factor queue, 12 bits each
  uint64_t t = coef;
#pragma unroll 1
  for (; nf; --nf) {
    const uint32_t f = (uint32_t)lo & 0xfffu;
    lo = (lo >> 12) | (hi << 52);
    hi >>= 12;
    const uint64_t x = m6w_pow(m6w_select<W>(P, f & 15u), f >> 4, M);
    t = have ? f64_mul(t, x, M) : x;
    have = true;
  }
  return t;
}

// One lane's share of one step: Q[c] = the sum of its terms of dimension c, 0 for the dimensions it has none of (wi_lane)
template <int W>
WI_HD void m6w_lane(const WiRow* rows, const uint64_t* coefs, uint32_t t0, uint32_t t1, const uint64_t (&P)[W], uint64_t (&Q)[W],
                    const f64_mod& M) {
#pragma unroll
  for (int c = 0; c < W; ++c) Q[c] = 0;
  if (t0 >= t1) return;
  uint32_t cur = wi_dim(rows[t0]);
  uint64_t run = 0;
#pragma unroll 1
  for (uint32_t t = t0; t < t1; ++t) {
    const WiRow row = rows[t];
    const uint32_t d = wi_dim(row);
    if (d != cur) {
      m6w_put<W>(Q, cur, run);
      run = 0;
      cur = d;
    }
    run = f64_add(run, m6w_term<W>(row, coefs[t], P, M), M);
  }
  m6w_put<W>(Q, cur, run);
}

// The new state from the group's partial sums: slots[j * W + c] = lane j's Q[c] (wi_gather)
template <int W>
WI_HD void m6w_gather(const uint64_t* slots, const WiPlan& p, uint64_t (&P)[W], const f64_mod& M) {
#pragma unroll
  for (int c = 0; c < W; ++c) {
    uint64_t s = 0;
#pragma unroll 1
    for (uint32_t j = p.first[c]; j < p.first[c] + p.nl[c]; ++j) s = j == p.first[c] ? slots[j * W + c] : f64_add(s, slots[j * W + c], M);
    P[c] = s;
  }
}

// What a row holds in d_witness between dispatches, and the state a resumed dispatch makes of it
template <int STORE>
WI_HD uint64_t m6w_stored(uint64_t x, const f64_mod& M) {
  return STORE == M6W_INLINE ? f64_from_mont(x, M) : x;
}
template <int STORE>
WI_HD uint64_t m6w_resumed(uint64_t x, const f64_mod& M) {
  return STORE == M6W_INLINE ? f64_to_mont(x, M) : x;
}
// M6W_PASS's closing pass, one element: Montgomery -> plain canonical
WI_HD uint64_t m6w_finish(uint64_t x, const f64_mod& M) { return f64_from_mont(x, M); }

// One dispatch of mod64witness.hip
struct Mod64WitnessArgs {
  const uint64_t* inputs;  // [batch][W], any 64-bit words, plain (read when k0 == 0)
  uint64_t* wit;           // [batch][W][steps]
  uint64_t steps;
  uint64_t k0, k1;         // rows of this dispatch
  uint32_t batch;
  uint32_t nterms;
  const uint64_t* coef;    // Mod64TermLayout::coef: Montgomery form, canonical
  const uint8_t* exps;     // Mod64TermLayout::exps: rows of W bytes
  uint32_t begin[SHK_STARK_MAX_WIDTH + 1];  // terms of dimension c: [begin[c], begin[c + 1])
  WiPlan plan;
};

// ---- host: the plan -------------------------------------------------------------------------------------------------------------
// wi_plan's group choice with the packed path's own slice budget.  group / slice: 0 = choose.  A step over budget is still a dispatch
// of its own.
inline void m6w_plan(const WiRow* rows, uint32_t T, uint32_t width, uint32_t group, uint64_t slice, WiPlan* out) {
  wi_plan(rows, T, width, group, slice, out);
  if (slice) return;
  const uint64_t fit = M6W_SLICE_PRODUCTS / (out->cost ? out->cost : 1);
  out->slice = fit ? fit : 1;
}
