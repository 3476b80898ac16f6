// modntt_items.cuh -- the generic transform over any odd modulus below 2^256 (fpm.cuh): the plan, the pass descriptors and the
// per-workgroup bodies as functions of (workgroup index, thread index, LDS pointer).  modntt.hip wraps them in kernels with a
// barrier between the phases; tests/native/modntt_host.cpp walks the same functions on the host over the same grid.
//
// A transform of n = 2^L points, natural order in and out, is m = ceil(L / t) passes of LDS tiles of 2^t elements (t =
// STARKHIP_MODNTT_TILE_LOG, default 10: 32 KiB of LDS, 2^24 points in three passes of radix 2^8), radices R_0 .. R_{m-1} as equal as
// L allows.  With P_d = R_0 .. R_{d-1}, N_d = n / P_d and S_d = N_d / R_d, pass d sees the vector as batch P_d blocks of N_d
// elements; inside a block, column j2 < S_d holds the R_d elements j1 S_d + j2.  The pass takes the R_d-point DFT of every column
// (root w^(n / R_d)), multiplies output k by w^(P_d j2 k) and stores it at k S_d + j2: in place, position for position.  The last
// pass (S = 1) has no twiddle; its block number is (k_0 .. k_{m-2}) with k_0 most significant and output k goes to
// k_0 + R_0 k_1 + .. + P_{m-1} k, which is natural order.  Because that store scatters over the whole vector, a plan of several
// passes runs source -> work buffer -> .. -> destination, so the source may be the destination.
//
// A tile is T = 2^t / R adjacent columns (numbered through blocks and vectors alike, so short columns share a tile).  Phases:
//   load   element j1 of column c to LDS row bitrev(j1), converted to Montgomery form on the first pass (one product with R^2);
//          the first pass also reads wire form when asked and takes everything from index n_in on as zero (fft_1d's padding);
//   stage  s = 1 .. log R: radix-2 decimation-in-time butterflies on rows (i, i + 2^(s-1)), twiddle tw[(i mod 2^(s-1)) n / 2^s];
//   store  row k times the pass twiddle, or on the last pass times `scale` in PLAIN form -- 1, or n^-1 for an inverse -- which is
//          the conversion out of Montgomery form in the same product.  No pass over memory exists only to convert.
// tw holds w^e in Montgomery form for e < n / 2 (w^(e + n/2) = -w^e): mn_tw_item builds it on the device from w^(2^i).
#pragma once
#include "fpm.cuh"

constexpr uint32_t MN_WG = 256;           // threads per workgroup
constexpr int MN_MAX_LOG_N = 26;          // n <= 2^26 and batch n <= 2^26
constexpr int MN_MAX_PASSES = 13;         // 26 / 2

struct MnPass {
  const void* src;   // fpm limbs, or 32-byte wire values when wire_in
  void* dst;
  const fpm* tw;     // n / 2 entries, null for n = 1
  uint64_t total;    // columns of the launch: batch n / R
  uint64_t n_in;     // first pass: elements per source vector (<= n)
  uint32_t log_n, log_R, log_S, log_T;
  uint32_t first, last, wire_in, wire_out;
  uint32_t ndig;     // last pass: the earlier passes' radix logs, k_0 first
  uint8_t dig_log[MN_MAX_PASSES];
  fpm scale;         // last pass: plain-form factor of every output
};

struct MnTw {
  fpm pw[MN_MAX_LOG_N];  // w^(2^i), Montgomery form
  fpm* tw;
  uint64_t count;        // n / 2
};

// ---- plan (host) -------------------------------------------------------------------------------------------------------------------
inline int mn_plan(int log_n, int tile_log, int radix[MN_MAX_PASSES]) {
  if (log_n == 0) {
    radix[0] = 0;
    return 1;
  }
  const int m = (log_n + tile_log - 1) / tile_log, base = log_n / m, rem = log_n % m;
  for (int d = 0; d < m; ++d) radix[d] = base + (d < rem ? 1 : 0);
  return m;
}
// pass d of the plan for `batch` vectors; src / dst / tw, n_in, the wire flags and scale are the caller's to fill
inline MnPass mn_pass(int log_n, int tile_log, const int* radix, int m, int d, uint64_t batch) {
  MnPass a = {};
  int log_P = 0;
  for (int e = 0; e < d; ++e) log_P += radix[e];
  a.log_n = (uint32_t)log_n;
  a.log_R = (uint32_t)radix[d];
  a.log_S = (uint32_t)(log_n - log_P - radix[d]);
  a.log_T = (uint32_t)(tile_log - radix[d]);
  a.total = batch << (log_n - radix[d]);
  a.n_in = 1ull << log_n;
  a.first = d == 0;
  a.last = d + 1 == m;
  if (a.last) {
    a.ndig = (uint32_t)d;
    for (int e = 0; e < d; ++e) a.dig_log[e] = (uint8_t)radix[e];
  }
  a.scale = fpm_from_u32(1u);
  return a;
}
inline uint64_t mn_tiles(const MnPass& a) { return (a.total + ((1ull << a.log_T) - 1)) >> a.log_T; }

// root < p and of order exactly n: 1 for n = 1, else root^(n/2) = -1 -- the condition under which the transform is invertible
inline bool mn_check_root(const fpm& root, uint64_t n, const fpm_mod& M) {
  if (!fpm_below_p(root, M)) return false;
  const fpm one = fpm_from_words(M.one), r = fpm_to_mont(root, M);
  if (n == 1) return fpm_eq(r, one);
  return fpm_eq(fpm_pow(r, n / 2, M), fpm_neg(one, M));
}
// n^-1 = ((p + 1) / 2)^log_n in plain form: no inversion, no primality
inline fpm mn_inv_n(int log_n, const fpm_mod& M) {
  fpm h;
  for (int i = 0; i < 8; ++i) h.v[i] = (M.p[i] >> 1) | (i < 7 ? M.p[i + 1] << 31 : 0u);
  uint64_t carry = 1;
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)h.v[i] + carry;
    h.v[i] = (uint32_t)x;
    carry = x >> 32;
  }
  return fpm_from_mont(fpm_pow(fpm_to_mont(h, M), (uint64_t)log_n, M), M);
}
// the squarings of the root (Montgomery form) that mn_tw_item multiplies up
inline void mn_tw_args(const fpm& root_mont, int log_n, const fpm_mod& M, MnTw* t) {
  fpm g = root_mont;
  for (int i = 0; i < MN_MAX_LOG_N; ++i) {
    t->pw[i] = g;
    g = fpm_mul(g, g, M);
  }
  t->count = log_n >= 1 ? 1ull << (log_n - 1) : 0;
}

// ---- element access ----------------------------------------------------------------------------------------------------------------
FPM_HD fpm mn_ld(const fpm* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  fpm r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
#else
  return *p;
#endif
}
FPM_HD void mn_st(fpm* p, const fpm& r) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  q[1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
#else
  *p = r;
#endif
}
FPM_HD uint32_t mn_bitrev(uint32_t x, uint32_t bits) { return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0u; }

// ---- the table ---------------------------------------------------------------------------------------------------------------------
FPM_HD void mn_tw_item(const MnTw& t, const fpm_mod& M, uint64_t e) {
  fpm acc = fpm_from_words(M.one);
  for (int i = 0; (e >> i) != 0; ++i)
    if ((e >> i) & 1) acc = fpm_mul(acc, t.pw[i], M);
  mn_st(t.tw + e, acc);
}

// ---- the phases of workgroup wg, thread tid (each loops over its share of the tile) -------------------------------------------------
FPM_HD void mn_load_item(const MnPass& a, const fpm_mod& M, uint64_t wg, uint32_t tid, fpm* lds) {
  const uint32_t T = 1u << a.log_T, elems = 1u << (a.log_T + a.log_R);
  const uint32_t log_N = a.log_R + a.log_S;
  for (uint32_t x = tid; x < elems; x += MN_WG) {
    const uint32_t tc = x & (T - 1), j1 = x >> a.log_T;
    const uint64_t c = (wg << a.log_T) + tc;
    if (c >= a.total) continue;
    const uint64_t q = c >> a.log_S, j2 = c & ((1ull << a.log_S) - 1);
    fpm v;
    if (a.first) {  // q is the vector: P_0 = 1
      const uint64_t idx = ((uint64_t)j1 << a.log_S) + j2;
      if (idx < a.n_in) {
        const fpm* s = reinterpret_cast<const fpm*>(a.src) + q * a.n_in + idx;
        v = mn_ld(s);
        if (a.wire_in) v = fpm_from_wire_words(v.v);
        v = fpm_to_mont(v, M);
      } else {
        v = fpm_zero();
      }
    } else {
      v = mn_ld(reinterpret_cast<const fpm*>(a.src) + (q << log_N) + ((uint64_t)j1 << a.log_S) + j2);
    }
    lds[(mn_bitrev(j1, a.log_R) << a.log_T) + tc] = v;
  }
}

FPM_HD void mn_stage_item(const MnPass& a, const fpm_mod& M, uint32_t s, uint64_t wg, uint32_t tid, fpm* lds) {
  const uint32_t T = 1u << a.log_T, bfs = 1u << (a.log_T + a.log_R - 1), half = 1u << (s - 1);
  for (uint32_t x = tid; x < bfs; x += MN_WG) {
    const uint32_t tc = x & (T - 1), pi = x >> a.log_T;
    if ((wg << a.log_T) + tc >= a.total) continue;
    const uint32_t lo = pi & (half - 1), i = ((pi >> (s - 1)) << s) | lo;
    fpm* u = lds + ((uint64_t)i << a.log_T) + tc;
    fpm* w = lds + ((uint64_t)(i + half) << a.log_T) + tc;
    const fpm y = *u;
    fpm z = *w;
    if (s > 1) z = fpm_mul(z, mn_ld(a.tw + ((uint64_t)lo << (a.log_n - s))), M);
    *u = fpm_add(y, z, M);
    *w = fpm_sub(y, z, M);
  }
}

FPM_HD void mn_store_item(const MnPass& a, const fpm_mod& M, uint64_t wg, uint32_t tid, const fpm* lds) {
  const uint32_t T = 1u << a.log_T, elems = 1u << (a.log_T + a.log_R);
  const uint32_t log_N = a.log_R + a.log_S, log_P = a.log_n - log_N;
  for (uint32_t x = tid; x < elems; x += MN_WG) {
    const uint32_t tc = x & (T - 1), k = x >> a.log_T;
    const uint64_t c = (wg << a.log_T) + tc;
    if (c >= a.total) continue;
    const uint64_t q = c >> a.log_S, j2 = c & ((1ull << a.log_S) - 1);
    fpm v = lds[x];
    if (!a.last) {
      const uint64_t e = (j2 * k) << log_P, h = 1ull << (a.log_n - 1);  // below n
      if (e) {
        const fpm t = mn_ld(a.tw + (e & (h - 1)));
        v = fpm_mul(v, e & h ? fpm_neg(t, M) : t, M);
      }
      mn_st(reinterpret_cast<fpm*>(a.dst) + (q << log_N) + ((uint64_t)k << a.log_S) + j2, v);
    } else {  // S = 1: q = vector P + block number
      uint64_t rho = q & ((1ull << log_P) - 1), out = 0;
      uint32_t sh = log_P;
      for (uint32_t d = 0; d < a.ndig; ++d) {  // k_0 is the most significant digit of the block number, the least of the output
        sh -= a.dig_log[d];
        out |= ((rho >> sh) & ((1ull << a.dig_log[d]) - 1)) << (log_P - sh - a.dig_log[d]);
      }
      out |= (uint64_t)k << log_P;
      v = fpm_mul(v, a.scale, M);
      if (a.wire_out) {
        fpm w;
        fpm_to_wire_words(v, w.v);
        v = w;
      }
      mn_st(reinterpret_cast<fpm*>(a.dst) + ((q >> log_P) << a.log_n) + out, v);
    }
  }
}

// c[i] = a[i] b[i] mod p, plain form in and out (a, b any 256-bit values): sh_mod_mul_polys' pointwise product
FPM_HD fpm mn_pointwise_item(const fpm& x, const fpm& y, const fpm_mod& M) {
  return fpm_mul(x, fpm_to_mont(y, M), M);
}
