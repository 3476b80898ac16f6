// modwitness_items.cuh -- the per-lane step of the witness generator over ANY odd modulus 3 <= p < 2^256 (modwitness.hip): the twin of
// witness_items.cuh on the Montgomery arithmetic of fpm.cuh.  A trace needs only ring operations -- no root of unity, no inverse -- so
// composite moduli are as good as primes here.
//
// The decomposition is witness_items.cuh's, unchanged: WiRow, wi_pack_row, WiPlan, wi_split and wi_plan do not depend on the field and
// are used as they are; only the arithmetic bodies have mwi_* forms, with the modulus block passed down by reference from the kernel
// argument.  Semantics are the reference's (multivariate_polynomial.py:329-338): X^0 = 1 also at X = 0 (a factor with exponent 0 is
// never in a row's factor queue), a term without factors is its coefficient, a dimension without terms is 0.
//
// Forms.  The state P[] lives in registers in Montgomery form: row 0 is fpm_to_mont(input), which also reduces an input >= p, and the
// coefficients arrive in Montgomery form (ModTermLayout).  d_witness ends PLAIN and canonical.  Between the two there are two store
// forms (MwiStore):
//   MWI_PASS   (default) the sequential kernel stores its rows as they are, Montgomery form, and one element-wise grid-wide pass
//              (mwi_finish) converts [batch][width][steps] in place after the last slice; a resumed slice reads Montgomery values.
//   MWI_INLINE the kernel converts on the store path (one fpm_from_mont per stored column per step, shared by the group's lanes) and a
//              resumed slice converts its starting row back (fpm_to_mont); there is no pass.
// A lone wave is bound by its own instruction stream, so MWI_INLINE's products are paid in full: on the 2-product MiMC step they are two
// more.  tools/mod_witness_time.py times both (profiles/r17_mod_witness.json, EXPERIMENTS.md); the numbers are quoted at
// MWI_SLICE_PRODUCTS below.
// Every function is __host__ __device__: tests/native/modwitness_host.cpp runs the same decomposition serially.
#pragma once
#include <stdint.h>

#include "fpm.cuh"
#include "witness_items.cuh"

// Sequential products per dispatch of the generic kernel.  mod_witness_kernel measures (tools/mod_witness_time.py,
// profiles/r17_mod_witness.json; BN254, Goldilocks and the MiMC prime within 0.1 % of each other) 1.9 us per counted product on MiMC
// (2 per step, 247 ms per 65535 steps at 64 units; 2.15 us for a single unit) and 4.05 us on the 256-term width-9 system at G = 16
// (56 per step, 227 us per step), against 1.13 and 1.78 us for witness_kernel in the same run: 1.68x and 2.27x.  2^12 products are
// 7.8 - 16.6 ms per dispatch.  The two systems are a factor 2.1 apart, more than the 9 - 14 ms band is wide, so no power of two
// puts both inside it: 2^12 centres them on it (2^11: 3.9 - 8.3 ms, 2^13: 15.6 - 33 ms).
// MWI_INLINE in the same run: 2.47 us per product on MiMC (324 ms, + 31 %: its two conversion products per step on top of the step's
// two are paid in full) and 4.05 us on the 256-term system (9 conversions shared by 16 lanes beside 56 products: no difference).
// MWI_PASS is the default: its closing pass is inside the 247 ms.
constexpr uint64_t MWI_SLICE_PRODUCTS = 1u << 12;

enum MwiStore { MWI_PASS = 0, MWI_INLINE = 1 };

// ModTermLayout has no "coefficient == 1" flag: a coefficient is canonical Montgomery form (fpm_to_mont of any 256-bit value, so 1 + p
// counts as 1), and 1 is M.one
WI_HD bool mwi_unit(const fpm& coef, const fpm_mod& M) { return fpm_eq(coef, fpm_from_words(M.one)); }

// P[v] / Q[c] for a lane-dependent index without indexing the register array (witness_items.cuh: wi_blend)
WI_HD void mwi_blend(fpm& r, const fpm& x, bool take) {
  const uint32_t m = 0u - (uint32_t)take;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (x.v[i] & m) | (r.v[i] & ~m);
}
template <int W>
WI_HD fpm mwi_select(const fpm (&P)[W], uint32_t v) {
  fpm r = P[0];
#pragma unroll
  for (int u = 1; u < W; ++u) mwi_blend(r, P[u], v == (uint32_t)u);
  return r;
}
template <int W>
WI_HD void mwi_put(fpm (&Q)[W], uint32_t c, const fpm& x) {
#pragma unroll
  for (int u = 0; u < W; ++u) mwi_blend(Q[u], x, c == (uint32_t)u);
}

// x^e, e >= 1, square-and-multiply from the top bit: the products wi_term_products counts
WI_HD fpm mwi_pow(const fpm& x, uint32_t e, const fpm_mod& M) {
  fpm r = x;
#pragma unroll 1
  for (int i = 30 - __builtin_clz(e); i >= 0; --i) {
    r = fpm_mul(r, r, M);
    if ((e >> i) & 1u) r = fpm_mul(r, x, M);
  }
  return r;
}

// coef * prod_v P[v]^e_v; a coefficient of 1 is not multiplied in (and is the value of a term without factors)
template <int W>
WI_HD fpm mwi_term(const WiRow& row, const fpm& coef, const fpm (&P)[W], const fpm_mod& M) {
  bool have = ((row.lo >> 4) & 1u) == 0;
  uint32_t nf = (uint32_t)(row.lo >> 5) & 15u;
  uint64_t lo = (row.lo >> 9) | (row.hi << 55), hi = row.hi >> 9;  // the factor queue, 12 bits each
  fpm t = coef;
#pragma unroll 1
  for (; nf; --nf) {
    const uint32_t f = (uint32_t)lo & 0xfffu;
    lo = (lo >> 12) | (hi << 52);
    hi >>= 12;
    const fpm x = mwi_pow(mwi_select<W>(P, f & 15u), f >> 4, M);
    t = have ? fpm_mul(t, x, M) : x;
    have = true;
  }
  return t;
}

// One lane's share of one step: Q[c] = the sum of its terms of dimension c, 0 for the dimensions it has none of (wi_lane)
template <int W>
WI_HD void mwi_lane(const WiRow* rows, const fpm* coefs, uint32_t t0, uint32_t t1, const fpm (&P)[W], fpm (&Q)[W], const fpm_mod& M) {
#pragma unroll
  for (int c = 0; c < W; ++c) Q[c] = fpm_zero();
  if (t0 >= t1) return;
  uint32_t cur = wi_dim(rows[t0]);
  fpm run = fpm_zero();
#pragma unroll 1
  for (uint32_t t = t0; t < t1; ++t) {
    const WiRow row = rows[t];
    const uint32_t d = wi_dim(row);
    if (d != cur) {
      mwi_put<W>(Q, cur, run);
      run = fpm_zero();
      cur = d;
    }
    run = fpm_add(run, mwi_term<W>(row, coefs[t], P, M), M);
  }
  mwi_put<W>(Q, cur, run);
}

// The new state from the group's partial sums: slots[j * W + c] = lane j's Q[c] (wi_gather)
template <int W>
WI_HD void mwi_gather(const fpm* slots, const WiPlan& p, fpm (&P)[W], const fpm_mod& M) {
#pragma unroll
  for (int c = 0; c < W; ++c) {
    fpm s = fpm_zero();
#pragma unroll 1
    for (uint32_t j = p.first[c]; j < p.first[c] + p.nl[c]; ++j) s = j == p.first[c] ? slots[j * W + c] : fpm_add(s, slots[j * W + c], M);
    P[c] = s;
  }
}

// What a row holds in d_witness between dispatches, and the state a resumed dispatch makes of it
template <int STORE>
WI_HD fpm mwi_stored(const fpm& x, const fpm_mod& M) {
  return STORE == MWI_INLINE ? fpm_from_mont(x, M) : x;
}
template <int STORE>
WI_HD fpm mwi_resumed(const fpm& x, const fpm_mod& M) {
  return STORE == MWI_INLINE ? fpm_to_mont(x, M) : x;
}
// MWI_PASS's closing pass, one element: Montgomery -> plain canonical
WI_HD fpm mwi_finish(const fpm& x, const fpm_mod& M) { return fpm_from_mont(x, M); }

// One dispatch of modwitness.hip
struct ModWitnessArgs {
  const fpm* inputs;    // [batch][W], any 256-bit values, plain (read when k0 == 0)
  fpm* wit;             // [batch][W][steps]
  uint64_t steps;
  uint64_t k0, k1;      // rows of this dispatch
  uint32_t batch;
  uint32_t nterms;
  const fpm* coef;      // ModTermLayout::coef: Montgomery form, canonical
  const uint8_t* exps;  // ModTermLayout::exps: rows of W bytes
  uint32_t begin[SHK_STARK_MAX_WIDTH + 1];  // terms of dimension c: [begin[c], begin[c + 1])
  WiPlan plan;
};

// ---- host: the plan -------------------------------------------------------------------------------------------------------------
// wi_plan's group choice (the split weighs products against LDS reads and additions, whose ratio the field changes little) with the
// generic path's own slice budget.  group / slice: 0 = choose.  A step over budget is still a dispatch of its own.
inline void mwi_plan(const WiRow* rows, uint32_t T, uint32_t width, uint32_t group, uint64_t slice, WiPlan* out) {
  wi_plan(rows, T, width, group, slice, out);
  if (slice) return;
  const uint64_t fit = MWI_SLICE_PRODUCTS / (out->cost ? out->cost : 1);
  out->slice = fit ? fit : 1;
}
