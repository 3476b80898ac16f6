// witness_items.cuh -- the per-lane step of the device witness generator (witness.hip) and the host plan it runs by.
//
// AIR.generate_witness / get_computational_trace (starks/air.py:32-52, 121-123): witness[c][0] = inputs[c] mod p and
// witness[c][k + 1] = step_c(witness[0][k], ..., witness[W - 1][k]) mod p, step_c the sum of its sparse terms coef * prod_v X_v^e_v
// (multivariate_polynomial.py:329-338; X^0 = 1 even at X = 0).  The recurrence is sequential in k, so one unit's step is split over a
// GROUP of G lanes of one wave (G = 1, 2, 4, 8, 16): lane j evaluates a contiguous run [t0_j, t1_j) of the term list (terms are in
// dimension order) and leaves one partial sum per dimension; the new state of dimension c is the sum of the partial sums of the lanes
// first[c] .. first[c] + nl[c] - 1.  Every function here is __host__ __device__, so tests/native/witness_host.cpp runs the same
// decomposition serially and compares it with the reference's traces.
#pragma once
#include <stdint.h>

#include "fp256.cuh"
#include "internal.hpp"  // SHK_STARK_MAX_WIDTH, SHK_STARK_MAX_TERMS

#define WI_HD __host__ __device__ __forceinline__

constexpr uint32_t WI_MAX_GROUP = 16;
// Sequential products per dispatch.  witness_kernel measures 1.1 us per counted product on MiMC (2 per step, 18.5 ms per 8192 steps) and
// 1.7 us on the 256-term width-9 system at G = 16 (56 per step, 97 us per step): 2^13 products are 9 - 14 ms per dispatch.
constexpr uint64_t WI_SLICE_PRODUCTS = 1u << 13;

// One term as the lanes read it: 16 bytes, one LDS read per term.  Bits 0-3 dimension, bit 4 coefficient == 1, bits 5-8 the number of
// factors with a non-zero exponent, then 12 bits per such factor: variable (4 bits) | exponent (8 bits).  9 + 9 * 12 = 117 bits.
struct alignas(16) WiRow {
  uint64_t lo, hi;
};

// ex = the term's exponent row (width bytes), unit = its coefficient is 1
WI_HD WiRow wi_pack_row(uint32_t dim, bool unit, const uint8_t* ex, uint32_t width) {
  WiRow r;
  r.lo = dim | (unit ? 16u : 0u);
  r.hi = 0;
  uint32_t nf = 0;
  for (uint32_t v = 0; v < width; ++v) {
    if (!ex[v]) continue;
    const uint64_t f = v | ((uint64_t)ex[v] << 4);
    const uint32_t pos = 9 + 12 * nf++;
    if (pos < 64) {
      r.lo |= f << pos;
      if (pos > 52) r.hi |= f >> (64 - pos);
    } else {
      r.hi |= f << (pos - 64);
    }
  }
  r.lo |= (uint64_t)nf << 5;
  return r;
}
WI_HD uint32_t wi_dim(const WiRow& r) { return (uint32_t)r.lo & 15u; }

// P[v] for a lane-dependent v without indexing the register array (an indexed array lives in scratch).  Masks rather than branches:
// the compiler folds `if (v == u) r = P[u]` back into an indexed load.
WI_HD void wi_blend(fp& r, const fp& x, bool take) {
  const uint32_t m = 0u - (uint32_t)take;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (x.v[i] & m) | (r.v[i] & ~m);
}
template <int W>
WI_HD fp wi_select(const fp (&P)[W], uint32_t v) {
  fp r = P[0];
#pragma unroll
  for (int u = 1; u < W; ++u) wi_blend(r, P[u], v == (uint32_t)u);
  return r;
}
template <int W>
WI_HD void wi_put(fp (&Q)[W], uint32_t c, const fp& x) {
#pragma unroll
  for (int u = 0; u < W; ++u) wi_blend(Q[u], x, c == (uint32_t)u);
}

// x^e, e >= 1, square-and-multiply from the top bit: (bit length - 1) squares and (popcount - 1) products
WI_HD fp wi_pow(const fp& x, uint32_t e) {
  fp r = x;
#pragma unroll 1
  for (int i = 30 - __builtin_clz(e); i >= 0; --i) {
    r = fp_sqr(r);
    if ((e >> i) & 1u) r = fp_mul(r, x);
  }
  return r;
}

// coef * prod_v P[v]^e_v; a coefficient of 1 is not multiplied in (and is the value of a term without factors)
template <int W>
WI_HD fp wi_term(const WiRow& row, const fp& coef, const fp (&P)[W]) {
  bool have = ((row.lo >> 4) & 1u) == 0;
  uint32_t nf = (uint32_t)(row.lo >> 5) & 15u;
  uint64_t lo = (row.lo >> 9) | (row.hi << 55), hi = row.hi >> 9;  // the factor queue, 12 bits each
  fp t = coef;
#pragma unroll 1
  for (; nf; --nf) {
    const uint32_t f = (uint32_t)lo & 0xfffu;
    lo = (lo >> 12) | (hi << 52);
    hi >>= 12;
    const fp x = wi_pow(wi_select<W>(P, f & 15u), f >> 4);
    t = have ? fp_mul(t, x) : x;
    have = true;
  }
  return t;
}

// One lane's share of one step: Q[c] = the sum of its terms of dimension c, 0 for the dimensions it has none of.  Terms [t0, t1) are in
// dimension order, so each dimension's run is summed in `run` and put into Q once.
template <int W>
WI_HD void wi_lane(const WiRow* rows, const fp* coefs, uint32_t t0, uint32_t t1, const fp (&P)[W], fp (&Q)[W]) {
#pragma unroll
  for (int c = 0; c < W; ++c) Q[c] = fp_zero();
  if (t0 >= t1) return;
  uint32_t cur = wi_dim(rows[t0]);
  fp run = fp_zero();
#pragma unroll 1
  for (uint32_t t = t0; t < t1; ++t) {
    const WiRow row = rows[t];
    const uint32_t d = wi_dim(row);
    if (d != cur) {
      wi_put<W>(Q, cur, run);
      run = fp_zero();
      cur = d;
    }
    run = fp_add(run, wi_term<W>(row, coefs[t], P));
  }
  wi_put<W>(Q, cur, run);
}

// How a unit's step is split over its group (kernel argument; built on the host by wi_plan)
struct WiPlan {
  uint32_t group;                            // G lanes per unit
  uint32_t t0[WI_MAX_GROUP], t1[WI_MAX_GROUP];  // lane j evaluates terms [t0[j], t1[j])
  uint32_t first[SHK_STARK_MAX_WIDTH];       // dimension c's partial sums sit in lanes first[c] .. first[c] + nl[c] - 1
  uint32_t nl[SHK_STARK_MAX_WIDTH];
  uint32_t cost;                             // products per step on the longest lane (plus one for the exchange when G > 1)
  uint64_t slice;                            // steps per dispatch
};

// One dispatch of witness.hip
struct WitnessArgs {
  const fp* inputs;     // [batch][W], lazily reduced (read when k0 == 0)
  fp* wit;              // [batch][W][steps], canonical
  uint64_t steps;
  uint64_t k0, k1;      // rows of this dispatch
  uint32_t batch;
  uint32_t nterms;
  const fp* coef;       // TermLayout::coef (ctx.hpp)
  const uint8_t* exps;  // TermLayout::exps: rows of W + 1 bytes, the last one flags coef == 1
  uint32_t begin[SHK_STARK_MAX_WIDTH + 1];  // terms of dimension c: [begin[c], begin[c + 1])
  WiPlan plan;
};

// The new state from the group's partial sums: slots[j * W + c] = lane j's Q[c]
template <int W>
WI_HD void wi_gather(const fp* slots, const WiPlan& p, fp (&P)[W]) {
#pragma unroll
  for (int c = 0; c < W; ++c) {
    fp s = fp_zero();
#pragma unroll 1
    for (uint32_t j = p.first[c]; j < p.first[c] + p.nl[c]; ++j) s = j == p.first[c] ? slots[j * W + c] : fp_add(s, slots[j * W + c]);
    P[c] = s;
  }
}

// ---- host: the plan -------------------------------------------------------------------------------------------------------------
// products of one term: (bit length - 1) + (popcount - 1) per factor, plus one per factor beyond the first and one for a coefficient
// other than 1
inline uint32_t wi_term_products(const WiRow& r) {
  uint32_t nf = (uint32_t)(r.lo >> 5) & 15u, prod = 0, mults = ((r.lo >> 4) & 1u) ? 0u : 1u;
  uint64_t lo = (r.lo >> 9) | (r.hi << 55), hi = r.hi >> 9;
  for (; nf; --nf) {
    const uint32_t e = ((uint32_t)lo & 0xfffu) >> 4;
    lo = (lo >> 12) | (hi << 52);
    hi >>= 12;
    prod += (31 - __builtin_clz(e)) + (__builtin_popcount(e) - 1);
    ++mults;
  }
  return prod + (mults ? mults - 1 : 0);
}

// Contiguous split of the T terms over at most G lanes with the smallest largest lane weight (weight = 4 x products + 1: a term without
// a product still costs a quarter product of LDS reads and an addition).  Returns that weight.
inline uint32_t wi_split(const WiRow* rows, uint32_t T, uint32_t G, WiPlan* p) {
  uint32_t w[SHK_STARK_MAX_TERMS], lo = 0, hi = 0;
  for (uint32_t t = 0; t < T; ++t) {
    w[t] = 4 * wi_term_products(rows[t]) + 1;
    lo = w[t] > lo ? w[t] : lo;
    hi += w[t];
  }
  auto parts = [&](uint32_t bound) {
    uint32_t n = 1, s = 0;
    for (uint32_t t = 0; t < T; ++t) {
      if (s + w[t] > bound) {
        ++n;
        s = 0;
      }
      s += w[t];
    }
    return n;
  };
  while (lo < hi) {  // smallest bound that G lanes can keep
    const uint32_t mid = lo + (hi - lo) / 2;
    if (parts(mid) <= G) hi = mid;
    else lo = mid + 1;
  }
  uint32_t j = 0, s = 0, worst = 0;
  p->t0[0] = 0;
  for (uint32_t t = 0; t < T; ++t) {
    if (s + w[t] > lo) {
      p->t1[j++] = t;
      p->t0[j] = t;
      s = 0;
    }
    s += w[t];
    worst = s > worst ? s : worst;
  }
  p->t1[j++] = T;
  for (; j < WI_MAX_GROUP; ++j) p->t0[j] = p->t1[j] = T;  // idle lanes
  p->group = G;
  return worst;
}

// The plan for one system: rows = the packed terms (in dimension order), width W.  group / slice: 0 = choose (knobs.hpp passes
// STARKHIP_WITNESS_GROUP / STARKHIP_WITNESS_SLICE here).  The default group is the one with the shortest estimated step: the longest
// lane's weight, plus for G > 1 the exchange (about a product, and an eighth of one per partial sum read back).
inline void wi_plan(const WiRow* rows, uint32_t T, uint32_t width, uint32_t group, uint64_t slice, WiPlan* out) {
  WiPlan best{};
  uint32_t best_est = 0xffffffffu, best_w = 0;
  for (uint32_t G = 1; G <= WI_MAX_GROUP; G *= 2) {
    if (group && G != group) continue;
    WiPlan p{};
    const uint32_t wt = wi_split(rows, T, G, &p);
    uint32_t reads = 0;
    for (uint32_t c = 0; c < width; ++c) {
      p.first[c] = 0;
      p.nl[c] = 0;
      for (uint32_t j = 0; j < G; ++j) {
        bool touches = false;
        for (uint32_t t = p.t0[j]; t < p.t1[j]; ++t) touches = touches || wi_dim(rows[t]) == c;
        if (!touches) continue;
        if (!p.nl[c]) p.first[c] = j;
        ++p.nl[c];
      }
      reads += p.nl[c];
    }
    const uint32_t est = wt + (G > 1 ? 4 + reads / 2 : 0);
    if (est < best_est) {
      best_est = est;
      best_w = wt;
      best = p;
    }
  }
  best.cost = best_w / 4 + (best.group > 1 ? 1 : 0);
  // at least one step: a step of more than WI_SLICE_PRODUCTS products (e.g. 256 terms of exponent 255 at G = 1) is a dispatch of its own
  const uint64_t fit = WI_SLICE_PRODUCTS / (best.cost ? best.cost : 1);
  best.slice = slice ? slice : (fit ? fit : 1);
  *out = best;
}
