// ntt64_items.cuh -- the transform over any odd modulus below 2^64 on packed 64-bit words (fp64m.cuh): the plan, the pass descriptors,
// the index maps and the per-workgroup bodies as functions of (workgroup index, thread index, LDS pointer).  ntt64.hip wraps them in
// kernels with a barrier between the phases; tests/native/ntt64_host.cpp walks the same functions on the host over the same grid, and
// enumerates the same index maps lane by lane (its `runs` and `banks` modes).
//
// The decomposition is modntt_items.cuh's.  A transform of n = 2^L points, natural order in and out, is m passes over LDS tiles of
// 2^t elements (t = STARKHIP_MOD64_TILE_LOG in 2 .. 13, default 12: 32 KiB of LDS), radices R_0 >= .. >= R_{m-1} as equal as L allows.
// With P_d = R_0 .. R_{d-1}, N_d = n / P_d and S_d = N_d / R_d, pass d sees the vector as batch P_d blocks of N_d elements; inside a
// block, column j2 < S_d holds the R_d elements j1 S_d + j2.  The pass takes the R_d-point DFT of every column (root w^(n / R_d)),
// multiplies output k by w^(P_d j2 k) and stores it at k S_d + j2: in place, position for position.  The last pass (S = 1) has no
// twiddle; its block number is (k_0 .. k_{m-2}) with k_0 most significant and output k goes to u + P k, u = k_0 + R_0 k_1 + ..,
// which is natural order.  A plan of several passes runs source -> work buffer -> .. -> destination, so the source may be the
// destination.
//
// What an 8-byte element changes against the 32-byte one:
//  PLAN RULE   the largest radix log is t - min(4, floor(t / 2)), so that a tile holds at least 16 columns (for t >= 8);
//              m = ceil(L / that), radix logs floor(L / m) or one more, the larger ones first; L = 0 is one pass of radix 1.
//              t = 12: 2^16 = (8, 8), 2^24 = (8, 8, 8), 2^28 = (7, 7, 7, 7).  A tile is T = 2^(t - log R) columns, fewer when the
//              whole launch has fewer.
//  RUNS        every global access of a pass walks runs of T >= 16 consecutive elements per 16 adjacent lanes (n >= 2^16):
//              passes 0 .. m-2 take T adjacent columns, lanes along the columns, both ways.  The last pass takes the T blocks whose
//              outputs are adjacent -- column c = vector P + u holds the block whose digits spell u -- and loads them with the lanes
//              along j1 (a block is R consecutive elements), then stores with the lanes along u.
//  TWIDDLES    w^e = hi[e >> h] lo[e & (2^h - 1)], h = ceil(L / 2): one product instead of a gather from an n / 2-entry table.  The
//              stage twiddles of a tile are stw[e] = w^(e n / R_0), e < R_0 / 2 (pass d reads every (R_0 / R_d)-th).  A plan owns
//              lo | hi | stw, at most 8 (2^(h+1) + 2^(t-1)) bytes (n64_table_bytes is the exact figure).
//  STAGES      decimation in frequency on natural-order rows, the stages in groups of up to three: a thread holds the 2^q rows of a
//              column that differ in bits b .. b+q-1, runs q stages in registers, and writes them back -- one LDS exchange and one
//              barrier per group.  The leftover group (log R mod 3 stages) runs first, so that the last group has three stages.  The
//              DFT leaves output k in row bitrev(k); the store phase walks the rows in order.
//  LDS IMAGE   element (row, column) lives at word row T + ((column ^ row) mod T), and for T = 16 word-address bit 4 is flipped by
//              row bit 3 (n64_lds_at): 16 lanes along the columns or along the rows hit 16 different 8-byte slots, and the two
//              rows that 32 lanes read at once lie in different halves of the 64 banks.
// Phases of workgroup wg:  load (conversion into Montgomery form on the first pass, zeros from index n_in on);  the groups;  store
// (times the pass twiddle, or on the last pass times `scale` in PLAIN form -- 1, or n^-1 -- which is the conversion out).
#pragma once
#include "fp64m.cuh"

constexpr uint32_t N64_WG = 256;           // threads per workgroup
constexpr int N64_MAX_LOG_N = 28;          // n <= 2^28 and batch n <= 2^28
constexpr int N64_MAX_PASSES = 28;         // tile log 2: radix 2
constexpr int N64_MIN_TILE_LOG = 2, N64_MAX_TILE_LOG = 13, N64_DEFAULT_TILE_LOG = 12;

struct N64Pass {
  const uint64_t* src;
  uint64_t* dst;
  const uint64_t *lo, *hi, *stw;  // Montgomery form; null for n = 1
  uint64_t total;                 // columns of the launch: batch n / R
  uint64_t n_in;                  // first pass: elements per source vector (<= n)
  uint64_t scale;                 // last pass: plain-form factor of every output
  uint32_t log_n, log_R, log_S, log_T, log_h;
  uint32_t stw_shift;             // log(R_0 / R): stage twiddle e of this pass is stw[e << stw_shift]
  uint32_t first, last;
  uint32_t ndig;                  // last pass: the earlier passes' radix logs, k_0 first
  uint8_t dig_log[N64_MAX_PASSES];
};

struct N64Tw {
  uint64_t pw[N64_MAX_LOG_N];  // w^(2^i), Montgomery form
  uint64_t* tab;               // lo | hi | stw
  uint32_t n_lo, n_hi, n_stw;  // 2^h, 2^(L - h), R_0 / 2
  uint32_t log_h, stw_log;     // exponent of stw[e]: e << stw_log = e n / R_0
};

// ---- plan (host) ---------------------------------------------------------------------------------------------------------------------
inline int n64_max_radix_log(int tile_log) { return tile_log - (tile_log / 2 < 4 ? tile_log / 2 : 4); }
inline int n64_plan(int log_n, int tile_log, int radix[N64_MAX_PASSES]) {
  if (log_n == 0) {
    radix[0] = 0;
    return 1;
  }
  const int rm = n64_max_radix_log(tile_log), m = (log_n + rm - 1) / rm, base = log_n / m, rem = log_n % m;
  for (int d = 0; d < m; ++d) radix[d] = base + (d < rem ? 1 : 0);
  return m;
}
inline int n64_log_h(int log_n) { return (log_n + 1) / 2; }
// pass d of the plan for `batch` vectors; src / dst / the tables, n_in and scale are the caller's to fill
inline N64Pass n64_pass(int log_n, int tile_log, const int* radix, int m, int d, uint64_t batch) {
  N64Pass a = {};
  int log_P = 0;
  for (int e = 0; e < d; ++e) log_P += radix[e];
  a.log_n = (uint32_t)log_n;
  a.log_R = (uint32_t)radix[d];
  a.log_S = (uint32_t)(log_n - log_P - radix[d]);
  a.total = batch << (log_n - radix[d]);
  a.log_T = (uint32_t)(tile_log - radix[d]);
  while (a.log_T > 0 && (1ull << (a.log_T - 1)) >= a.total) --a.log_T;  // no wider than the launch
  a.log_h = (uint32_t)n64_log_h(log_n);
  a.stw_shift = (uint32_t)(radix[0] - radix[d]);
  a.n_in = 1ull << log_n;
  a.first = d == 0;
  a.last = d + 1 == m;
  if (a.last) {
    a.ndig = (uint32_t)d;
    for (int e = 0; e < d; ++e) a.dig_log[e] = (uint8_t)radix[e];
  }
  a.scale = 1;
  return a;
}
inline uint64_t n64_tiles(const N64Pass& a) { return (a.total + ((1ull << a.log_T) - 1)) >> a.log_T; }
inline uint32_t n64_tile_elems(const N64Pass& a) { return 1u << (a.log_T + a.log_R); }

// root < p and of order exactly n: 1 for n = 1, else root^(n/2) = -1 -- the condition under which the transform is invertible
inline bool n64_check_root(uint64_t root, uint64_t n, const f64_mod& M) {
  if (root >= M.p) return false;
  const uint64_t r = f64_to_mont(root, M);
  if (n == 1) return r == M.one;
  return f64_pow(r, n / 2, M) == f64_neg(M.one, M);
}
// n^-1 = ((p + 1) / 2)^log_n in plain form: no inversion, no primality
inline uint64_t n64_inv_n(int log_n, const f64_mod& M) {
  return f64_from_mont(f64_pow(f64_to_mont((M.p >> 1) + 1, M), (uint64_t)log_n, M), M);
}
// the tables of (root, n) under a plan whose first radix log is r0 (log_n >= 1); t->tab is the caller's to fill
inline void n64_tw_args(uint64_t root_mont, int log_n, int r0, const f64_mod& M, N64Tw* t) {
  uint64_t g = root_mont;
  for (int i = 0; i < N64_MAX_LOG_N; ++i) {
    t->pw[i] = g;
    g = f64_mul(g, g, M);
  }
  t->log_h = (uint32_t)n64_log_h(log_n);
  t->n_lo = 1u << t->log_h;
  t->n_hi = 1u << (log_n - (int)t->log_h);
  t->n_stw = 1u << (r0 - 1);
  t->stw_log = (uint32_t)(log_n - r0);
  t->tab = nullptr;
}
inline uint64_t n64_table_entries(const N64Tw& t) { return (uint64_t)t.n_lo + t.n_hi + t.n_stw; }
inline uint64_t n64_table_bytes(const N64Tw& t) { return 8 * n64_table_entries(t); }
// the documented bound of a plan's bytes
inline uint64_t n64_table_bound(int log_n, int tile_log) { return 8 * ((2ull << n64_log_h(log_n)) + (1ull << (tile_log - 1))); }

F64_HD uint32_t n64_bitrev(uint32_t x, uint32_t bits) { return bits ? __builtin_bitreverse32(x) >> (32 - bits) : 0u; }

// ---- the tables ----------------------------------------------------------------------------------------------------------------------
F64_HD void n64_tw_item(const N64Tw& t, const f64_mod& M, uint64_t i) {
  uint64_t e = i < t.n_lo ? i : i < (uint64_t)t.n_lo + t.n_hi ? (i - t.n_lo) << t.log_h : (i - t.n_lo - t.n_hi) << t.stw_log;
  uint64_t acc = M.one;
  for (int b = 0; e != 0; ++b, e >>= 1)
    if (e & 1) acc = f64_mul(acc, t.pw[b], M);
  t.tab[i] = acc;
}

// ---- index maps: what lane x of a phase touches.  The phases below call these and nothing else to form an address --------------------
// word address of element (row, column tc) of the tile's LDS image
F64_HD uint32_t n64_lds_at(const N64Pass& a, uint32_t row, uint32_t tc) {
  uint32_t x = (row << a.log_T) | ((tc ^ row) & ((1u << a.log_T) - 1));
  if (a.log_T == 4) x ^= (row & 8u) << 1;
  return x;
}
// column c of the launch -> the element offset of its first element and the element stride along j1 is S (passes before the last) or
// 1 (last pass); vec = the vector (first pass: the source has n_in elements per vector)
struct N64Col {
  uint64_t vec, at;  // at: offset of (j1 = 0 / k = 0) inside the vector's n elements
};
F64_HD N64Col n64_col(const N64Pass& a, uint64_t c) {
  N64Col r;
  const uint32_t log_N = a.log_R + a.log_S, log_P = a.log_n - log_N;
  if (!a.last) {
    const uint64_t q = c >> a.log_S, j2 = c & ((1ull << a.log_S) - 1);  // q = vector P + block
    r.vec = q >> log_P;
    r.at = ((q & ((1ull << log_P) - 1)) << log_N) + j2;
  } else {
    r.vec = c >> log_P;
    r.at = c & ((1ull << log_P) - 1);  // u: the low part of every output index of this column
  }
  return r;
}
// last pass: the block whose outputs are u + P k -- the digits of u, k_0 least significant, spell the block number k_0 first
F64_HD uint64_t n64_block_of(const N64Pass& a, uint64_t u) {
  uint64_t blk = 0;
  for (uint32_t d = 0; d < a.ndig; ++d) {
    blk = (blk << a.dig_log[d]) | (u & ((1ull << a.dig_log[d]) - 1));
    u >>= a.dig_log[d];
  }
  return blk;
}
// load slot x < tile elements of workgroup wg: false = nothing of this launch; *zero = padding (no load); *src = element index from
// a.src; *lds = word address of the LDS store
F64_HD bool n64_load_map(const N64Pass& a, uint64_t wg, uint32_t x, uint64_t* src, bool* zero, uint32_t* lds) {
  uint32_t tc, j1;
  if (!a.last) {
    tc = x & ((1u << a.log_T) - 1);
    j1 = x >> a.log_T;
  } else {
    j1 = x & ((1u << a.log_R) - 1);
    tc = x >> a.log_R;
  }
  const uint64_t c = (wg << a.log_T) + tc;
  if (c >= a.total) return false;
  const N64Col col = n64_col(a, c);
  const uint64_t idx = a.last ? (n64_block_of(a, col.at) << a.log_R) + j1 : col.at + ((uint64_t)j1 << a.log_S);
  *zero = a.first && idx >= a.n_in;
  *src = a.first ? col.vec * a.n_in + idx : (col.vec << a.log_n) + idx;
  *lds = n64_lds_at(a, j1, tc);
  return true;
}
// item x < tile elements / 2^q of the group of q stages on row bits b .. b+q-1: false = nothing of this launch; lds[j] for j < 2^q;
// *low = the rows' bits below b
F64_HD bool n64_group_map(const N64Pass& a, uint32_t b, uint32_t q, uint64_t wg, uint32_t x, uint32_t* lds, uint32_t* low) {
  const uint32_t tc = x & ((1u << a.log_T) - 1), g = x >> a.log_T;
  if ((wg << a.log_T) + tc >= a.total) return false;
  *low = g & ((1u << b) - 1);
  const uint32_t base = ((g >> b) << (b + q)) | *low;
  for (uint32_t j = 0; j < (1u << q); ++j) lds[j] = n64_lds_at(a, base + (j << b), tc);
  return true;
}
// store slot x < tile elements: *dst = element index into a.dst, *lds = word address of the LDS load, *e = the exponent of the
// pass twiddle (0 on the last pass)
F64_HD bool n64_store_map(const N64Pass& a, uint64_t wg, uint32_t x, uint64_t* dst, uint32_t* lds, uint64_t* e) {
  const uint32_t tc = x & ((1u << a.log_T) - 1), row = x >> a.log_T, k = n64_bitrev(row, a.log_R);
  const uint64_t c = (wg << a.log_T) + tc;
  if (c >= a.total) return false;
  const N64Col col = n64_col(a, c);
  const uint32_t log_P = a.log_n - a.log_R - a.log_S;
  if (!a.last) {
    *dst = (col.vec << a.log_n) + col.at + ((uint64_t)k << a.log_S);
    *e = ((c & ((1ull << a.log_S) - 1)) * k) << log_P;  // P j2 k, below n
  } else {
    *dst = (col.vec << a.log_n) + col.at + ((uint64_t)k << log_P);
    *e = 0;
  }
  *lds = n64_lds_at(a, row, tc);
  return true;
}

// ---- the phases of workgroup wg, thread tid (each loops over its share of the tile) ---------------------------------------------------
F64_HD void n64_load_item(const N64Pass& a, const f64_mod& M, uint64_t wg, uint32_t tid, uint64_t* lds) {
  const uint32_t elems = 1u << (a.log_T + a.log_R);
#pragma unroll 4
  for (uint32_t x = tid; x < elems; x += N64_WG) {
    uint64_t src;
    uint32_t at;
    bool zero;
    if (!n64_load_map(a, wg, x, &src, &zero, &at)) continue;
    uint64_t v = 0;
    if (!zero) {
      v = a.src[src];
      if (a.first) v = f64_to_mont(v, M);
    }
    lds[at] = v;
  }
}

// q = Q stages of decimation in frequency on the rows base + j 2^b, j < 2^Q: stage s pairs j with j + 2^s (rows 2^(b+s) apart)
template <int Q>
F64_HD void n64_group_item(const N64Pass& a, const f64_mod& M, uint32_t b, uint64_t wg, uint32_t tid, uint64_t* lds) {
  constexpr uint32_t E = 1u << Q;
  const uint32_t items = 1u << (a.log_T + a.log_R - Q);
  for (uint32_t x = tid; x < items; x += N64_WG) {
    uint32_t at[E], low;
    if (!n64_group_map(a, b, Q, wg, x, at, &low)) continue;
    uint64_t v[E];
#pragma unroll
    for (uint32_t j = 0; j < E; ++j) v[j] = lds[at[j]];
#pragma unroll
    for (int s = Q - 1; s >= 0; --s) {
#pragma unroll
      for (uint32_t j = 0; j < E; ++j) {
        if (j & (1u << s)) continue;
        // row mod 2^(b+s) of the pair, as an exponent of the 2^(b+s+1)-th root w_R^(R / 2^(b+s+1))
        const uint32_t ex = (low + ((j & ((1u << s) - 1)) << b)) << (a.log_R - (b + s + 1));
        const uint64_t y = v[j], z = v[j | (1u << s)];
        v[j] = f64_add(y, z, M);
        uint64_t d = f64_sub(y, z, M);
        if (ex) d = f64_mul(d, a.stw[(uint64_t)ex << a.stw_shift], M);
        v[j | (1u << s)] = d;
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < E; ++j) lds[at[j]] = v[j];
  }
}

// the groups of a radix-2^log_R pass, leftover first: their number, and group g's stage count *q and lowest row bit *b
F64_HD uint32_t n64_groups(uint32_t log_R) { return log_R / 3 + (log_R % 3 ? 1u : 0u); }
F64_HD void n64_group_shape(uint32_t log_R, uint32_t g, uint32_t* q, uint32_t* b) {
  const uint32_t rem = log_R % 3, first = rem ? 1u : 0u;
  if (g < first) {
    *q = rem;
    *b = log_R - rem;
  } else {
    *q = 3;
    *b = log_R - rem - 3 * (g - first + 1);
  }
}
F64_HD void n64_group_any(const N64Pass& a, const f64_mod& M, uint32_t g, uint64_t wg, uint32_t tid, uint64_t* lds) {
  uint32_t q, b;
  n64_group_shape(a.log_R, g, &q, &b);
  if (q == 3) n64_group_item<3>(a, M, b, wg, tid, lds);
  else if (q == 2) n64_group_item<2>(a, M, b, wg, tid, lds);
  else n64_group_item<1>(a, M, b, wg, tid, lds);
}

F64_HD void n64_store_item(const N64Pass& a, const f64_mod& M, uint64_t wg, uint32_t tid, const uint64_t* lds) {
  const uint32_t elems = 1u << (a.log_T + a.log_R);
#pragma unroll 4
  for (uint32_t x = tid; x < elems; x += N64_WG) {
    uint64_t dst, e;
    uint32_t at;
    if (!n64_store_map(a, wg, x, &dst, &at, &e)) continue;
    uint64_t v = lds[at];
    if (a.last) {
      v = f64_mul(v, a.scale, M);
    } else if (e) {
      v = f64_mul(v, f64_mul(a.hi[e >> a.log_h], a.lo[e & ((1ull << a.log_h) - 1)], M), M);
    }
    a.dst[dst] = v;
  }
}

// c[i] = a[i] b[i] mod p, plain form in and out (any 64-bit x, y): sh_mod64_mul_polys' pointwise product
F64_HD uint64_t n64_pointwise_item(uint64_t x, uint64_t y, const f64_mod& M) {
  return f64_mul(x, f64_to_mont(y, M), M);
}
