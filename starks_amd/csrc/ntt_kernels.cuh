// ntt_kernels.cuh -- radix-2^r tile passes of the large NTT over Z/p (replaces the recursive
// _fft/_simple_ft of starks/fft.py:287-314; same outputs, natural order in and out).
//
// Decomposition.  n = R_1 * R_2 * ... * R_m, one kernel launch ("pass") per factor:
//   pass d < m ("column pass", LAST=false): the array is viewed as [P_d][R_d][S_d] (S_d = n / (P_d R_d));
//       every column (p, j2) gets an R_d-point NTT along the middle axis, in place, followed by the
//       inter-pass twiddle  g_d^(j2*k1),  g_d = w^(P_d)  (order R_d*S_d).
//   pass m ("row pass", LAST=true): contiguous rows of R_m points; the result is scattered to natural
//       order  out[drev(p) + P*k]  (drev = mixed-radix digit reversal of the row number).
// A workgroup owns a tile of R x T elements (2048 elements = 64 KiB of LDS -> 2 workgroups per CU):
// T adjacent columns (T*32 B contiguous per row: coalesced segments) or T rows.  Each thread keeps 4
// elements in registers and does two butterfly levels (radix-4) between LDS exchanges; the R-point
// transform is decimation-in-frequency, so the tile's own twiddles come from one table of R/2 powers of
// w^(n/R) shared by every pass that uses radix R; the bit-reversed order DIF leaves is undone by the
// store addresses.  The last two levels of each tile transform have twiddles 1 / w^(R/4) only.
#pragma once
#include <stdlib.h>

#include <atomic>
#include <type_traits>

#include "internal.hpp"
#include "knobs.hpp"


// LDS image of a tile: 32-byte elements, 8 to a 256-byte bank row; the slot inside the row is XOR-ed with
// the higher index bits so that any power-of-two stride between lanes spreads over all 8 slots.
__host__ __device__ constexpr uint32_t lds_slot(uint32_t e) {
  uint32_t s = (e ^ (e >> 3) ^ (e >> 6) ^ (e >> 9)) & 7u;
  return (((e >> 3) << 3) | s) * 2u;  // in uint4 units
}
// lds_slot is linear over GF(2) (shifts, XOR, disjoint masks), so lds_slot(e ^ d) == lds_slot(e) ^ lds_slot(d): a
// thread computes the slot of its first element once and reaches the other three with one XOR by a constant.
__device__ __forceinline__ void lds_put_at(uint4* lds, uint32_t o, const fp& r) {
  lds[o] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  lds[o + 1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}
__device__ __forceinline__ fp lds_get_at(const uint4* lds, uint32_t o) {
  uint4 a = lds[o], b = lds[o + 1];
  fp r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
}
__device__ __forceinline__ void lds_put(uint4* lds, uint32_t e, const fp& r) {
  uint32_t o = lds_slot(e);
  lds[o] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
  lds[o + 1] = make_uint4(r.v[4], r.v[5], r.v[6], r.v[7]);
}
__device__ __forceinline__ fp lds_get(const uint4* lds, uint32_t e) {
  uint32_t o = lds_slot(e);
  uint4 a = lds[o], b = lds[o + 1];
  fp r;
  r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
  r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
  return r;
}

__device__ __forceinline__ fp tw_lookup(const NttPassArgs& a, uint64_t e) {
  if (a.tw_direct) return fp_load(a.tw_lo + e);
  fp lo = fp_load(a.tw_lo + (e & ((1ull << a.tw_lb) - 1)));
  fp hi = fp_load(a.tw_hi + (e >> a.tw_lb));
  return fp_mul(lo, hi);
}

template <class F>
__device__ __forceinline__ void static_for4(F&& f) {
  f(std::integral_constant<int, 0>{});
  f(std::integral_constant<int, 1>{});
  f(std::integral_constant<int, 2>{});
  f(std::integral_constant<int, 3>{});
}

// Per-thread state carried across the register groups of one tile pass.
struct TileThread {
  fp x[4];
  uint32_t t, ibase;
  bool active;
  uint64_t gbase;  // global element offset of (this thread's column/row, i = 0)
  uint64_t j2;     // column pass: column index inside the prefix block
  uint64_t obase;  // row pass: output offset of k = 0
  uint64_t sbase;  // zero-padded source (a.src_n != 0): element offset of (this column/row, i = 0) in the short source
};

// ---- which thread holds which elements ---------------------------------------------------------------------------------
// In group g a thread holds the four elements whose row index i differs in the bits (beta, beta + 1) of the group's two
// levels; the other LOG_R - 2 bits of i (and the column t) name the thread.  WAVE-LOCAL EXCHANGES: the groups fall into
// two phases.  Phase 0 (the first GA groups, whose level bits are the top 2 GA bits of i) takes the wave number from i
// bits BELOW its level bits, phase 1 (the rest) from the TOP bits of i, which its levels never touch.  Inside a phase an
// element therefore stays in the same wave from group to group: the hand-over through LDS needs no workgroup barrier (the
// LDS unit serves a wave's requests in order), only the phase change does -- one __syncthreads() per tile instead of one
// per group, and waves that drift apart instead of marching in step.  (SHK_WAVE_LOCAL=0: the plain mapping, a barrier per
// exchange.)
#ifndef SHK_WAVE_LOCAL
#define SHK_WAVE_LOCAL 1
#endif
template <int LOG_R, int LOG_T>
__host__ __device__ constexpr bool tile_wave_local() {
  constexpr int LOG_W = LOG_R + LOG_T - 8;  // log2 of the waves per workgroup
  if (!SHK_WAVE_LOCAL || LOG_W < 0 || LOG_T > 5 || LOG_R < 4) return false;
  constexpr int GA = (LOG_W + 1) / 2;
  return LOG_W <= LOG_R - 2 * GA;
}
// phase of group g: -1 = the row pass's first group (its own lane mapping), 0 / 1 as above
template <int LOG_R, int LOG_T, bool LAST>
__host__ __device__ constexpr int tile_phase(int g) {
  if (LAST && g == 0) return -1;
  if (!tile_wave_local<LOG_R, LOG_T>()) return 2 + g;  // every exchange crosses waves
  constexpr int LOG_W = LOG_R + LOG_T - 8;
  return g < (LOG_W + 1) / 2 ? 0 : 1;
}
// row index (with the group's two level bits clear) of the elements of thread tid in group g (not the row pass's group 0)
template <int LOG_R, int LOG_T, int g>
__host__ __device__ __forceinline__ uint32_t tile_ibase(uint32_t tid) {
  constexpr int beta = (LOG_R - 2 * (g + 1)) > 0 ? (LOG_R - 2 * (g + 1)) : 0;
  if constexpr (!tile_wave_local<LOG_R, LOG_T>()) {
    const uint32_t rest = tid >> LOG_T;
    return ((rest >> beta) << (beta + 2)) | (rest & ((1u << beta) - 1u));
  } else {
    constexpr int LOG_W = LOG_R + LOG_T - 8;
    constexpr int GA = (LOG_W + 1) / 2;
    constexpr int wlo = g < GA ? (LOG_R - 2 * GA) - LOG_W : LOG_R - LOG_W;  // the wave number sits at i bits [wlo, wlo + LOG_W)
    const uint32_t lane_i = (tid & 63u) >> LOG_T, wave = tid >> 6;
    uint32_t i = 0;
    int nl = 0, nw = 0;
#pragma unroll
    for (int p = 0; p < LOG_R; ++p) {
      if (p == beta || p == beta + 1) continue;
      if (p >= wlo && p < wlo + LOG_W) {
        i |= ((wave >> nw) & 1u) << p;
        ++nw;
      } else {
        i |= ((lane_i >> nl) & 1u) << p;
        ++nl;
      }
    }
    return i;
  }
}

// Column t and row base (the group's two level bits clear) of thread tid in group g of a tile pass: its four elements are the rows
// ibase | (h << beta), h = 0..3, beta = max(LOG_R - 2 (g + 1), 0).  The row pass's first group has its own mapping (lanes run along
// the contiguous row).  (Also what tests/native/tile_map_host.cpp enumerates on the host to check the wave-local exchanges.)
template <int LOG_R, int LOG_T, bool LAST, int g>
__host__ __device__ __forceinline__ void tile_thread_coords(uint32_t tid, uint32_t* t, uint32_t* ibase) {
  constexpr int beta = (LOG_R - 2 * (g + 1)) > 0 ? (LOG_R - 2 * (g + 1)) : 0;
  if constexpr (LAST && g == 0) {
    const uint32_t rest = tid & ((1u << LOG_R) / 4 - 1);
    *t = tid >> (LOG_R - 2);
    *ibase = ((rest >> beta) << (beta + 2)) | (rest & ((1u << beta) - 1u));
  } else {
    *t = tid & ((1u << LOG_T) - 1);
    *ibase = tile_ibase<LOG_R, LOG_T, g>(tid);
  }
}

// ---- the tile's own twiddles ---------------------------------------------------------------------------------------------
// Group g does the levels q = qhi and qhi - 1 (qhi = LOG_R - 1 - 2 g), two butterflies b = 2 lv + pr each; level q multiplies by
// w_R^((i mod 2^q) * 2^(LOG_R - 1 - q)), an entry of a.wR (R / 2 pairs).  Which of the four products exist is known at compile time.
template <int LOG_R, int g>
__host__ __device__ constexpr bool tile_tw_needed(int b) {
  constexpr int beta = (LOG_R - 2 * (g + 1)) > 0 ? (LOG_R - 2 * (g + 1)) : 0;
  constexpr int qhi = LOG_R - 1 - 2 * g;
  const int q = qhi - (b >> 1), pr = b & 1;
  if (q <= 0) return false;                        // level absent, or twiddle 1
  const int lb = q - beta;
  const int hl = lb == 1 ? pr : 2 * pr;
  if (q == 1 && beta == 0) return (hl & 1) != 0;   // 1 or w^(R/4)
  return true;
}
// index into a.wR of butterfly b's twiddle for the thread whose row base is ibase
template <int LOG_R, int g>
__host__ __device__ constexpr uint32_t tile_tw_exponent(int b, uint32_t ibase) {
  constexpr int beta = (LOG_R - 2 * (g + 1)) > 0 ? (LOG_R - 2 * (g + 1)) : 0;
  constexpr int qhi = LOG_R - 1 - 2 * g;
  const int q = qhi - (b >> 1), pr = b & 1;
  const int lb = q - beta;
  const int hl = lb == 1 ? pr : 2 * pr;
  if (q == 1 && beta == 0) return (1u << LOG_R) / 4;  // w^(R/4), the 4th root of unity
  const uint32_t il = ibase | ((uint32_t)hl << beta);
  return (il & ((1u << q) - 1u)) << (LOG_R - 1 - q);
}

// TWIDDLES IN LDS.  Every thread of a tile needs up to 13 of the R / 2 pairs, and which ones depends on its row base alone: read
// from global memory that is 4 global_load_dwordx4 per pair and thread for a table of 32 R bytes that never leaves the L1.  Cells
// with room for it copy the table into LDS behind the tile image once per tile (1 or 2 loads per thread, one workgroup barrier in
// front of the first product; read-only afterwards, so the barrier-free exchanges of the image are untouched) and take the pairs
// from there: four ds_read_b128 that wait on lgkmcnt and leave vmcnt to the elements and the inter-pass twiddles.
// A cell qualifies when image + table, times the workgroups per CU its thread count allows, still fit the 160 KiB of a CU -- the
// table must never cost a workgroup -- and the radix is at most 2^9 (the 2^10 and 2^11 tables do not fit beside any tile that
// leaves two workgroups per CU).  Workgroups per CU: at 5 waves per SIMD (20 per CU), which a kernel of at most 96 registers may
// run, the 512- and 1024-element tiles fill the CU with images alone (10 x 16 KiB, 5 x 32 KiB) and no table fits: the radices
// below 2^8 are counted that way and keep the global loads on those tiles.  Radix 2^8 and 2^9 are counted at 4 waves per SIMD
// (16 per CU).  That matters for <8,2,*> alone (4 x 40 KiB) and rests on its 98 and 100 registers; on the 2048- and 4096-element
// tiles 16 and 20 waves are the same 2 and 1 workgroups (<8,3,true> and <8,4,true> do fit 96 registers).  The compiler's register
// count is not visible here, so tests/native/ntt_occupancy.hip asks the runtime: with and without the table, every qualifying cell.
// SHK_TW_LDS=0: every cell reads global memory.
#ifndef SHK_TW_LDS
#define SHK_TW_LDS 1
#endif
template <int LOG_R, int LOG_T>
__host__ __device__ constexpr bool tile_tw_in_lds() {
  constexpr int TILE_LOG = LOG_R + LOG_T;
  if (!SHK_TW_LDS || LOG_R > 9 || TILE_LOG < 8 || TILE_LOG > 12) return false;
  constexpr long wgs = (LOG_R >= 8 ? 16 : 20) >> (TILE_LOG - 8);  // 2^(TILE_LOG - 8) waves each
  return ((32L << TILE_LOG) + (32L << LOG_R)) * wgs <= 160L * 1024;
}
// bytes of dynamic LDS of a cell
template <int LOG_R, int LOG_T>
__host__ __device__ constexpr size_t tile_lds_bytes() {
  return ((size_t)32 << (LOG_R + LOG_T)) + (tile_tw_in_lds<LOG_R, LOG_T>() ? (size_t)32 << LOG_R : 0);
}
// Where 16-byte chunk c (0..3) of the pair with exponent ex lives in the table region, in uint4 units.  A pair is 64 bytes = 16 of
// the 64 banks, and one ds_read_b128 serves 16 lanes at a time, each lane 4 banks wide: it is conflict-free when the distinct
// pairs of those 16 lanes differ in the 4-bit key (pair slot mod 4, chunk rotation).  A level reads exponents a power-of-two
// stride apart (at most 4 distinct per 16 lanes in the column mapping, 16 consecutive or every second one in the row pass's first
// group, and with bits 0 and 4 or 0, 1 and 5 apart where wave or level bits split a thread's row index), so the key is
// ex ^ (ex >> 3) ^ (ex >> 4): no XOR of two exponents that one lane group reads together, in any cell, folds to zero.  The key's
// low half moves the pair inside its aligned group of four, its high half rotates the chunks inside the pair.  A bijection of
// [0, R/2) x [0, 4) onto [0, 2 R) for every R >= 4; tests/native/tw_lds_map_host.cpp enumerates it.
__host__ __device__ constexpr uint32_t tw_lds_key(uint32_t ex) { return (ex ^ (ex >> 3) ^ (ex >> 4)) & 15u; }
__host__ __device__ constexpr uint32_t tw_lds_slot(uint32_t ex, uint32_t c) {
  const uint32_t k = tw_lds_key(ex);
  return ((((ex & ~3u) | (k & 3u)) << 2) | (c ^ (k >> 2)));
}
// THE ADDRESS OF A PAIR, in bytes from the start of the table region.  tw_lds_slot is linear over GF(2) in the exponent (the key is
// XORs of shifts under a mask, and the ORs join disjoint bits), and so is the exponent in the row index.  The two butterflies of a
// level differ in one level bit of the row index, which the row base has clear: the second pair's address is the first's XOR a
// compile-time constant (zero where the level's mask drops that bit), and the chunks of a pair are its address XOR 16, 32, 48.  A
// thread forms one address per level; every other read is one XOR by a constant, or an immediate offset where the bit is clear.
template <int LOG_R, int g>
__host__ __device__ constexpr uint32_t tile_tw_pair_xor(int b) {
  return 16u * tw_lds_slot(tile_tw_exponent<LOG_R, g>(b, 0) ^ tile_tw_exponent<LOG_R, g>(b & ~1, 0), 0);
}
template <int LOG_R, int g>
__host__ __device__ constexpr uint32_t tile_tw_byte(int b, uint32_t ibase, uint32_t c) {
  return (16u * tw_lds_slot(tile_tw_exponent<LOG_R, g>(b & ~1, ibase), 0)) ^ tile_tw_pair_xor<LOG_R, g>(b) ^ (16u * c);
}
// What the kernel computes for butterfly b (compile-time).  The pair constant's bits above the key (8 and up) fall on bits the level's
// address has clear: they are added, and end up in the read's immediate offset.  Its key bits 4, 5 only rotate the chunks: the second
// pair reads the first pair's four addresses in another order, and the read is tile_tw_byte as it stands.  Key bits 6, 7 cost one XOR
// for the pair: tile_tw_level folds the key bits into the level's address once, and tile_tw_read adds the rest per chunk.
template <int LOG_R, int g, int b>
__host__ __device__ constexpr bool tile_tw_keyed() { return (tile_tw_pair_xor<LOG_R, g>(b) & 0xc0u) != 0; }
template <int LOG_R, int g, int b>
__host__ __device__ constexpr uint32_t tile_tw_level(uint32_t ibase) {
  const uint32_t at = tile_tw_byte<LOG_R, g>(b & ~1, ibase, 0);
  return tile_tw_keyed<LOG_R, g, b>() ? at ^ (tile_tw_pair_xor<LOG_R, g>(b) & 0xf0u) : at;
}
template <int LOG_R, int g, int b>
__host__ __device__ constexpr uint32_t tile_tw_read(uint32_t level, uint32_t ibase, uint32_t c) {
  if constexpr (tile_tw_keyed<LOG_R, g, b>()) return (level ^ (16u * c)) + (tile_tw_pair_xor<LOG_R, g>(b) & ~0xffu);
  else return tile_tw_byte<LOG_R, g>(b, ibase, c);
}
// the copy: thread tid of `threads` moves the chunks j = tid, tid + threads, ... < 2 R of a.wR (chunk j = pair j / 4, part j % 4)
template <int LOG_R, int LOG_T>
__host__ __device__ constexpr int tile_tw_fill_chunks() {  // steps per thread (rounded up)
  constexpr int chunks = 2 << LOG_R, threads = 1 << (LOG_R + LOG_T - 2);
  return (chunks + threads - 1) / threads;
}
// the chunk thread tid moves in step k, or -1 (the bound is checked at run time only in a step that not every thread takes)
template <int LOG_R, int LOG_T>
__host__ __device__ constexpr int tile_tw_fill_chunk(uint32_t tid, int k) {
  constexpr uint32_t chunks = 2u << LOG_R, threads = 1u << (LOG_R + LOG_T - 2);
  const uint32_t j = tid + (uint32_t)k * threads;
  return ((uint32_t)(k + 1) * threads <= chunks || j < chunks) ? (int)j : -1;
}

// WHERE THE OUTPUTS GO.  Position i of the DIF output holds frequency k = bitrev(i).  The last group's elements are i = ibase | h
// with bits 0 and 1 of ibase clear, and bit reversal carries those two bits to the top: k_h = k_0 + tile_out_k_step(h), k_0 the
// frequency of h = 0.  A thread reverses one index; the other three rows lie a wave-uniform distance behind it, which the scalar unit
// scales by the launch's row stride once.
template <int LOG_R>
__host__ __device__ constexpr uint32_t tile_out_k_step(int h) {
  return ((uint32_t)(h & 1) << (LOG_R - 1)) | ((uint32_t)(h >> 1) << (LOG_R - 2));
}

// Register group g: fetch 4 elements (global memory for g == 0, LDS otherwise), do its butterfly levels,
// and hand the elements to the next group through LDS.
template <int LOG_R, int LOG_T, bool LAST, int g>
__device__ __forceinline__ void ntt_group(const NttPassArgs& a, uint4* lds, TileThread& th, uint32_t tid, uint64_t tile0) {
  constexpr int R = 1 << LOG_R;
  constexpr int G = (LOG_R + 1) / 2;
  constexpr int beta = (LOG_R - 2 * (g + 1)) > 0 ? (LOG_R - 2 * (g + 1)) : 0;  // position of local bit 0
  tile_thread_coords<LOG_R, LOG_T, LAST, g>(tid, &th.t, &th.ibase);

  if (g == 0 || (LAST && g == 1)) {
    // (re)derive the global coordinates of this thread's column/row: t changes between the
    // rfast mapping of the row pass's first group and the t-fast mapping of the later ones.
    // Threads past the end (partial last tile) work on a copy of the last valid column / row and store nothing: every
    // load is unconditional and in bounds, so the four loads of a thread are requested back to back.
    const uint64_t col_raw = tile0 + th.t;
    th.active = col_raw < a.total;
    const uint64_t col = th.active ? col_raw : a.total - 1;
    if (LAST) {
      const uint64_t b = col >> a.log_P;
      const uint32_t pp = (uint32_t)(col & ((1ull << a.log_P) - 1));
      // tiles enumerate rows with the FIRST pass's digit fastest, so that a tile's T rows land on
      // T adjacent output addresses
      const uint32_t lr1 = a.ndig ? a.dig_log[0] : 0;
      const uint32_t k1 = pp & ((1u << lr1) - 1u);
      const uint32_t rst = pp >> lr1;
      const uint32_t p = (k1 << (a.log_P - lr1)) | rst;
      uint32_t sh = a.log_P, wl = 0, acc = 0;
#pragma unroll
      for (uint32_t d = 0; d < 3; ++d) {
        if (d < a.ndig) {
          sh -= a.dig_log[d];
          acc |= ((p >> sh) & ((1u << a.dig_log[d]) - 1u)) << wl;
          wl += a.dig_log[d];
        }
      }
      th.gbase = (b << a.log_n) + ((uint64_t)p << LOG_R);
      th.obase = (b << a.log_n) + acc;
      th.sbase = b * a.src_n;  // used by one-pass transforms only (p = 0)
    } else {
      th.j2 = col & ((1ull << a.log_S) - 1);
      th.gbase = ((col >> a.log_S) << (LOG_R + a.log_S)) + th.j2;
      th.sbase = (col >> a.log_S) * a.src_n;  // first pass: P = 1, col >> log_S is the vector index
    }
  }

  // ---- the twiddles of this group's (up to) four butterflies b = 2 lv + pr: which exist is known at compile time ---------
  constexpr int qhi = LOG_R - 1 - 2 * g;
  constexpr bool TWL = tile_tw_in_lds<LOG_R, LOG_T>();
  auto tw_needed = [](int b) constexpr { return tile_tw_needed<LOG_R, g>(b); };
  auto tw_load = [&](auto bc) {  // butterfly b as an integral_constant: which form its address takes is known at compile time
    constexpr int b = decltype(bc)::value;
    if constexpr (TWL) {
      const char* tw = reinterpret_cast<const char*>(lds + (2u << (LOG_R + LOG_T)));  // the table region behind the tile image
      // tile_tw_byte(b, ibase, c) from the level's one address (tile_tw_level, tile_tw_read).  The empty asm keeps the compiler from
      // merging the pair's key XOR into each chunk's address anew (four instructions instead of one).
      uint32_t at = tile_tw_level<LOG_R, g, b>(th.ibase);
      if constexpr (tile_tw_keyed<LOG_R, g, b>()) asm("" : "+v"(at));
      auto chunk = [&](uint32_t c) { return *reinterpret_cast<const uint4*>(tw + tile_tw_read<LOG_R, g, b>(at, th.ibase, c)); };
      const uint4 c0 = chunk(0), c1 = chunk(1), c2 = chunk(2), c3 = chunk(3);
      fp2 r;
      r.w.v[0] = c0.x; r.w.v[1] = c0.y; r.w.v[2] = c0.z; r.w.v[3] = c0.w;
      r.w.v[4] = c1.x; r.w.v[5] = c1.y; r.w.v[6] = c1.z; r.w.v[7] = c1.w;
      r.w128.v[0] = c2.x; r.w128.v[1] = c2.y; r.w128.v[2] = c2.z; r.w128.v[3] = c2.w;
      r.w128.v[4] = c3.x; r.w128.v[5] = c3.y; r.w128.v[6] = c3.z; r.w128.v[7] = c3.w;
      return r;
    } else {
      return fp2_load(a.wR + tile_tw_exponent<LOG_R, g>(b, th.ibase));
    }
  };
  // one twiddle is always in flight: the first is requested before the elements are fetched, the next before the current
  // product (the product's inline asm keeps the compiler from moving loads across it, so source order is issue order)
  constexpr int first_tw = tw_needed(0) ? 0 : tw_needed(1) ? 1 : tw_needed(2) ? 2 : tw_needed(3) ? 3 : 4;
  fp2 tw_cur, tw_nxt;
  // Twiddles in LDS, first group: this thread's share of the table is requested first and the elements right behind it, so that
  // the copy waits for the table alone (vmcnt counts in order) while the elements are in flight; the workgroup barrier and the
  // first twiddle read follow the element loads (tw_fill_finish), in front of the group's first product.
  constexpr int FILL = tile_tw_fill_chunks<LOG_R, LOG_T>();  // 1 or 2 in every qualifying cell (LOG_T >= 2)
  static_assert(!TWL || FILL == 1 || FILL == 2, "twiddle copy: one or two chunks per thread");
  uint4 tw_fill0 = make_uint4(0, 0, 0, 0), tw_fill1 = tw_fill0;
  if constexpr (TWL && g == 0) {
    const uint4* src = reinterpret_cast<const uint4*>(a.wR);
    const int j0 = tile_tw_fill_chunk<LOG_R, LOG_T>(tid, 0), j1 = tile_tw_fill_chunk<LOG_R, LOG_T>(tid, 1);
    tw_fill0 = src[j0 < 0 ? 0 : j0];
    if constexpr (FILL == 2) tw_fill1 = src[j1 < 0 ? 0 : j1];
    // no instruction of its own: keeps the compiler from sinking the requests to the copy below, behind the element loads
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "singlethread");
  }
  auto tw_fill_finish = [&]() {
    uint4* tw = lds + (2u << (LOG_R + LOG_T));
    const int j0 = tile_tw_fill_chunk<LOG_R, LOG_T>(tid, 0), j1 = tile_tw_fill_chunk<LOG_R, LOG_T>(tid, 1);
    if (j0 >= 0) tw[tw_lds_slot((uint32_t)j0 >> 2, (uint32_t)j0 & 3u)] = tw_fill0;
    if constexpr (FILL == 2) {
      if (j1 >= 0) tw[tw_lds_slot((uint32_t)j1 >> 2, (uint32_t)j1 & 3u)] = tw_fill1;
    }
    __syncthreads();
    if constexpr (first_tw < 4) tw_cur = tw_load(std::integral_constant<int, first_tw>{});
  };
  if constexpr (first_tw < 4 && !(TWL && g == 0)) tw_cur = tw_load(std::integral_constant<int, first_tw>{});

  // ---- zero-padded source whose non-zero part ends inside the first quarter of the rows (the 8x low-degree extension:
  // rows i >= R / 8 of every column are zero): this thread's elements 1..3 are zero, so the group's two levels are
  //   x2 = x0 w_a,  x1 = x0 w_b,  x3 = x2 w_c   -- three products, no addition, nothing at all where x0 is zero too
  bool sparse_done = false;
  if constexpr (g == 0 && !LAST && LOG_R >= 4) {
    if (a.src_n && a.src_n <= ((uint64_t)(R / 4) << a.log_S)) {
      sparse_done = true;
      const uint64_t off = ((uint64_t)th.ibase << a.log_S) + th.j2;  // element h = 0
      const bool in = off < a.src_n;
      th.x[0] = th.x[1] = th.x[2] = th.x[3] = fp_zero();
      fp x0 = fp_zero();
      if constexpr (TWL) {
        if (FP_ANY(in)) x0 = fp_load(a.src + th.sbase + (in ? off : 0));
        tw_fill_finish();  // src_n is the launch's: every thread of the workgroup comes this way
      }
      if (FP_ANY(in)) {  // wave-uniform
        if constexpr (!TWL) x0 = fp_load(a.src + th.sbase + (in ? off : 0));
        const fp2 tw_b = tw_load(std::integral_constant<int, 2>{}), tw_c = tw_load(std::integral_constant<int, 3>{});  // tw_cur holds butterfly 0's
#pragma unroll
        for (int w = 0; w < 8; ++w) x0.v[w] = in ? x0.v[w] : 0u;
        th.x[0] = x0;
        th.x[2] = fp_mul2(x0, tw_cur);
        th.x[1] = fp_mul2(x0, tw_b);
        th.x[3] = fp_mul2(th.x[2], tw_c);
      }
    }
  }

  // ---- fetch this group's four elements ---------------------------------------------------------
  if (sparse_done) {
    // nothing left to do before the exchange
  } else if (g == 0) {
    if (a.src_n) {  // zero-padded source (first pass only): points at or beyond src_n are zero and are not read
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const uint32_t i = th.ibase | ((uint32_t)h << beta);
        const uint64_t off = LAST ? (uint64_t)i : (((uint64_t)i << a.log_S) + th.j2);
        const bool in = off < a.src_n;
        fp v = fp_load(a.src + th.sbase + (in ? off : 0));
#pragma unroll
        for (int w = 0; w < 8; ++w) v.v[w] = in ? v.v[w] : 0u;
        th.x[h] = v;
      }
      if constexpr (TWL) tw_fill_finish();
    } else {
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        // the rows of h = 1..3 lie a wave-uniform (h << beta) << log_S behind the thread's first
        th.x[h] = LAST ? fp_load(a.src + th.gbase + (th.ibase | ((uint32_t)h << beta)))
                       : fp_load(a.src + th.gbase + ((uint64_t)th.ibase << a.log_S) + ((uint64_t)((uint32_t)h << beta) << a.log_S));
      }
      // in the block of the element loads: the copy's wait then counts exactly these eight requests behind the table's
      if constexpr (TWL) tw_fill_finish();
    }
  } else {
#pragma unroll
    for (int h = 0; h < 4; ++h)
      th.x[h] = lds_get_at(lds, lds_slot((th.ibase << LOG_T) | th.t) ^ lds_slot((uint32_t)h << (beta + LOG_T)));
  }

  // ---- butterfly levels (DIF: a' = a + b, b' = (a - b) * w^((i mod half) * 2^s)) ---------------------
  if (!sparse_done) static_for4([&](auto bc) {
    constexpr int b = decltype(bc)::value;
    constexpr int q = qhi - (b >> 1), pr = b & 1;
    if constexpr (q >= 0) {
      constexpr int lb = q - beta;  // local bit
      constexpr int hl = lb == 1 ? pr : 2 * pr;  // lower element of the pair
      constexpr int hh = hl | (1 << lb);
      constexpr int nxt = (b < 1 && tw_needed(1)) ? 1 : (b < 2 && tw_needed(2)) ? 2 : (b < 3 && tw_needed(3)) ? 3 : 4;
      if constexpr (tw_needed(b) && nxt < 4) tw_nxt = tw_load(std::integral_constant<int, nxt>{});
      const fp s = fp_add(th.x[hl], th.x[hh]);
      fp d = fp_sub(th.x[hl], th.x[hh]);
      if constexpr (tw_needed(b)) {
        d = fp_mul2(d, tw_cur);
        if constexpr (nxt < 4) tw_cur = tw_nxt;
      }
      th.x[hl] = s;
      th.x[hh] = d;
    }
  });

  // ---- hand the elements to the next group through LDS ---------------------------------------------
  if (g < G - 1) {
    // in place: for g > 0 these are exactly the slots this thread read at the top of the group (element (i, t) always lives
    // at the same slot), and no other thread touches them before the barrier below -- one barrier per exchange
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      lds_put_at(lds, lds_slot((th.ibase << LOG_T) | th.t) ^ lds_slot((uint32_t)h << (beta + LOG_T)), th.x[h]);
    }
    if constexpr (tile_phase<LOG_R, LOG_T, LAST>(g) == tile_phase<LOG_R, LOG_T, LAST>(g + 1)) {
      // the next group's elements were written by lanes of this wave: order the wave's own LDS traffic, nothing more
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
      __syncthreads();
    }
  }
}

#ifndef SHK_NTT_MIN_WAVES
#define SHK_NTT_MIN_WAVES 4
#endif
template <int LOG_R, int LOG_T, bool LAST>
__device__ __forceinline__ void ntt_pass_body(const NttPassArgs& a) {
  static_assert(LOG_R >= 2 && LOG_R <= 11 && LOG_T >= 0 && LOG_R + LOG_T >= 8 && LOG_R + LOG_T <= 12, "unsupported tile");
  constexpr int G = (LOG_R + 1) / 2;  // register groups (two levels each, the last may have one)
  extern __shared__ __attribute__((aligned(16))) uint4 lds[];
  const uint32_t tid = threadIdx.x;
  uint64_t tile = blockIdx.x;
  if (a.xcd_per) {
    tile = (uint64_t)(blockIdx.x & 7u) * a.xcd_per + (blockIdx.x >> 3);
    if ((tile << LOG_T) >= a.total) return;  // grid padding (whole workgroup, before any barrier)
  }
  const uint64_t tile0 = tile << LOG_T;
  TileThread th;
  th.t = 0; th.ibase = 0; th.active = false; th.gbase = 0; th.j2 = 0; th.obase = 0; th.sbase = 0;
  // Column passes: the inter-pass twiddles g^(j2 k) of this thread's outputs are requested ahead of their use -- before the
  // LAST group's butterflies (whose own twiddles are 1 and w^(R/4) only) -- so that their latency (HBM, or L2 when another
  // vector has just read the same rows) is hidden behind arithmetic instead of being paid four times in the store loop.
  // One is kept in flight (the first before the last group, the others one product ahead in the store loop): all four at
  // once, or two, cost a wave per SIMD (106 / 102 VGPRs) and measured slower on single vectors and on 2^24.
  fp itw[4];
  auto itw_load = [&](int h) {
    const uint32_t k0 = __brev(tile_ibase<LOG_R, LOG_T, G - 1>(tid)) >> (32 - LOG_R);  // the last group's h = 0 (beta = 0)
    return fp_load(a.tw2 + ((uint64_t)k0 << a.log_S) + th.j2 + ((uint64_t)tile_out_k_step<LOG_R>(h) << a.log_S));
  };
  auto itw_request = [&]() {
    if (!LAST && a.tw2) itw[0] = itw_load(0);
  };
  if constexpr (G == 1) {
    ntt_group<LOG_R, LOG_T, LAST, 0>(a, lds, th, tid, tile0);
    itw_request();
  } else {
    ntt_group<LOG_R, LOG_T, LAST, 0>(a, lds, th, tid, tile0);
    if constexpr (G == 2) itw_request();
    ntt_group<LOG_R, LOG_T, LAST, 1>(a, lds, th, tid, tile0);
    if constexpr (G > 2) {
      if constexpr (G == 3) itw_request();
      ntt_group<LOG_R, LOG_T, LAST, 2>(a, lds, th, tid, tile0);
    }
    if constexpr (G > 3) {
      if constexpr (G == 4) itw_request();
      ntt_group<LOG_R, LOG_T, LAST, 3>(a, lds, th, tid, tile0);
    }
    if constexpr (G > 4) {
      if constexpr (G == 5) itw_request();
      ntt_group<LOG_R, LOG_T, LAST, 4>(a, lds, th, tid, tile0);
    }
    if constexpr (G > 5) {
      if constexpr (G == 6) itw_request();
      ntt_group<LOG_R, LOG_T, LAST, 5>(a, lds, th, tid, tile0);
    }
  }

  // ---- store: position i of the DIF output holds frequency k = bitrev(i) ----------------------------
  if (!th.active) return;
  const uint32_t k0 = __brev(th.ibase) >> (32 - LOG_R);  // the last group's local bits sit at position 0: k of h is k0 + step(h)
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const uint32_t step = tile_out_k_step<LOG_R>(h);
    if (LAST) {
      fp v = th.x[h];
      if (a.scale) v = fp_mul(v, fp_load(a.scale));
      fp_store(a.dst + th.obase + ((uint64_t)k0 << a.log_P) + ((uint64_t)step << a.log_P), v);
    } else {
      if (a.tw2 && h + 1 < 4) itw[h + 1] = itw_load(h + 1);
      const fp tw = a.tw2 ? itw[h] : tw_lookup(a, th.j2 * (k0 + step));
      fp v = fp_mul(th.x[h], tw);
      fp_store(a.dst + th.gbase + ((uint64_t)k0 << a.log_S) + ((uint64_t)step << a.log_S), v);
    }
  }
}

template <int LOG_R, int LOG_T, bool LAST>
__global__ void __launch_bounds__(1 << (LOG_R + LOG_T - 2), SHK_NTT_MIN_WAVES) ntt_pass_kernel(NttPassArgs a) {
  ntt_pass_body<LOG_R, LOG_T, LAST>(a);
}

// ---- narrow launches -----------------------------------------------------------------------------------------------------
// A pass over fewer tiles than the chip has CUs is a latency chain, not a throughput problem: every workgroup is alone on its CU, a
// lone wave issues an instruction every ~2 ns whatever it does, and ntt_pass_body gives a thread 2 butterflies per level (4
// elements, 14-20 butterflies and 4 inter-pass products per pass = 11-20 us for a radix 2^7..2^9 pass).  Here a thread owns ONE
// butterfly per level (twice the threads per tile, 512 for 1024 elements): the pair (i, i + half) of level q = log2(half) is read from
// the tile's LDS image, combined, and written back in place; one workgroup barrier per level; the first level reads global memory,
// the last one writes it (same addresses, twiddles and results as ntt_pass_body: DIF, position i holds frequency bitrev(i)).
// Used below STARKHIP_NTT_NARROW_TILES tiles per launch (knobs.hpp; small transforms: the commits and proofs of 2^14..2^16-step traces).
template <int LOG_R, int LOG_T, bool LAST>
__global__ void __launch_bounds__(1 << (LOG_R + LOG_T - 1)) ntt_narrow_pass_kernel(NttPassArgs a) {
  static_assert(LOG_R >= 2 && LOG_R <= 10 && LOG_T >= 0 && (LOG_R + LOG_T == 10 || LOG_R + LOG_T == 9), "1024- or 512-element tiles");
  __shared__ __attribute__((aligned(16))) uint4 lds[2 << (LOG_R + LOG_T)];
  constexpr int R = 1 << LOG_R;
  const uint32_t tid = threadIdx.x;
  // Which butterfly (column / row t, pair index p) a thread takes may change from level to level: everything goes through the LDS
  // image behind a workgroup barrier.  Column pass: adjacent lanes take adjacent columns throughout (32 contiguous bytes each, in
  // the loads and in the stores).  Row pass: adjacent lanes run along the contiguous row for the loads of the first level and take
  // adjacent rows afterwards, so that the T outputs of one frequency land on T adjacent addresses (as in ntt_pass_body).
  const uint32_t t_in = LAST ? tid >> (LOG_R - 1) : tid & ((1u << LOG_T) - 1u);
  const uint32_t p_in = LAST ? tid & (R / 2 - 1) : tid >> LOG_T;
  const uint32_t t = tid & ((1u << LOG_T) - 1u), p = tid >> LOG_T;
  const uint64_t tile0 = (uint64_t)blockIdx.x << LOG_T;
  // threads past the end work on a copy of the last column / row and store nothing
  const uint64_t col_in = tile0 + t_in < a.total ? tile0 + t_in : a.total - 1;
  const bool active = tile0 + t < a.total;
  const uint64_t col = active ? tile0 + t : a.total - 1;
  uint64_t gbase_in, gbase = 0, obase = 0, sbase_in, j2 = 0;
  if (LAST) {
    auto row_of = [&](uint64_t c, uint64_t* bb) {  // rows enumerated with the first pass's digit fastest, as in ntt_pass_body
      *bb = c >> a.log_P;
      const uint32_t pp = (uint32_t)(c & ((1ull << a.log_P) - 1));
      const uint32_t lr1 = a.ndig ? a.dig_log[0] : 0;
      const uint32_t k1 = pp & ((1u << lr1) - 1u), rst = pp >> lr1;
      return (k1 << (a.log_P - lr1)) | rst;
    };
    uint64_t b_in, b_out;
    const uint32_t row_in = row_of(col_in, &b_in), row = row_of(col, &b_out);
    uint32_t sh = a.log_P, wl = 0, acc = 0;
#pragma unroll
    for (uint32_t d = 0; d < 3; ++d) {
      if (d < a.ndig) {
        sh -= a.dig_log[d];
        acc |= ((row >> sh) & ((1u << a.dig_log[d]) - 1u)) << wl;
        wl += a.dig_log[d];
      }
    }
    gbase_in = (b_in << a.log_n) + ((uint64_t)row_in << LOG_R);
    obase = (b_out << a.log_n) + acc;
    sbase_in = b_in * a.src_n;
  } else {
    j2 = col & ((1ull << a.log_S) - 1);
    gbase = ((col >> a.log_S) << (LOG_R + a.log_S)) + j2;
    gbase_in = gbase;
    sbase_in = (col >> a.log_S) * a.src_n;
  }
  auto fetch = [&](uint32_t i) {
    if (a.src_n) {  // zero-padded source (first pass): points at or beyond src_n are zero and are not read
      const uint64_t off = LAST ? (uint64_t)i : (((uint64_t)i << a.log_S) + j2);
      const bool in = off < a.src_n;
      fp v = fp_load(a.src + sbase_in + (in ? off : 0));
#pragma unroll
      for (int w = 0; w < 8; ++w) v.v[w] = in ? v.v[w] : 0u;
      return v;
    }
    return LAST ? fp_load(a.src + gbase_in + i) : fp_load(a.src + gbase_in + ((uint64_t)i << a.log_S));
  };
  fp x0, x1;
  uint32_t i_lo = 0;
  // the twiddle pair of a level, w_R^((i mod half) * R / (2 half)), depends on the thread alone: it is requested one level ahead (the
  // product's inline asm pins a load where the source has it, and a load right in front of its product is ~0.5 us of every level)
  auto tw_of = [&](int q) {
    const uint32_t half = 1u << q, pq = q == LOG_R - 1 ? p_in : p;
    const uint32_t il = ((pq >> q) << (q + 1)) | (pq & (half - 1u));
    return fp2_load(a.wR + ((il & (half - 1u)) << (LOG_R - 1 - q)));
  };
  fp2 tw_cur, tw_nxt;
  if constexpr (LOG_R >= 2) tw_cur = tw_of(LOG_R - 1);
#pragma unroll
  for (int q = LOG_R - 1; q >= 0; --q) {
    const uint32_t half = 1u << q;
    const uint32_t tq = q == LOG_R - 1 ? t_in : t, pq = q == LOG_R - 1 ? p_in : p;
    i_lo = ((pq >> q) << (q + 1)) | (pq & (half - 1u));
    const uint32_t i_hi = i_lo | half;
    const uint32_t s_lo = lds_slot((i_lo << LOG_T) | tq), s_hi = lds_slot((i_hi << LOG_T) | tq);
    fp u, v;
    if (q == LOG_R - 1) {
      u = fetch(i_lo);
      v = fetch(i_hi);
    } else {
      u = lds_get_at(lds, s_lo);
      v = lds_get_at(lds, s_hi);
    }
    if (q > 1) tw_nxt = tw_of(q - 1);
    x0 = fp_add(u, v);
    x1 = fp_sub(u, v);
    if (q > 0) {
      x1 = fp_mul2(x1, tw_cur);
      if (q > 1) tw_cur = tw_nxt;
      lds_put_at(lds, s_lo, x0);
      lds_put_at(lds, s_hi, x1);
      __syncthreads();
    }
  }
  if (!active) return;
  // position i of the DIF output holds frequency k = bitrev(i); this thread ends with positions i_lo (even) and i_lo + 1
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t k = __brev(i_lo | (uint32_t)h) >> (32 - LOG_R);
    fp v = h ? x1 : x0;
    if (LAST) {
      if (a.scale) v = fp_mul(v, fp_load(a.scale));
      fp_store(a.dst + obase + ((uint64_t)k << a.log_P), v);
    } else {
      const fp tw = a.tw2 ? fp_load(a.tw2 + ((uint64_t)k << a.log_S) + j2) : tw_lookup(a, j2 * k);
      fp_store(a.dst + gbase + ((uint64_t)k << a.log_S), fp_mul(v, tw));
    }
  }
}

// ---- launching a tile pass (any kernel built on ntt_pass_body) --------------------------------------------------------------
// Tiles narrower than 128 bytes (T < 4: the big-radix passes) share their cache lines with the neighbouring tile; workgroups
// are dealt to the 8 XCDs round-robin, so neighbours would sit behind different L2s and every line would be fetched (or
// written back partially) twice.  Default (1): such launches map adjacent tiles to the same XCD (measured on the T = 1
// variant: 8.6 -> 10.2 G elements/s).  STARKHIP_XCD_SWZ (knobs.hpp): 0 = never, 2 = every tile pass (measured level for
// T >= 4).  The caller decides (xcd; knobs.hpp: shk_ntt_choose_cell); the grid is then padded to a multiple of 8 workgroups.

// attr_done: one bit per device ordinal, per kernel instantiation (contexts on several devices, and on several host threads,
// share the launcher)
inline hipError_t shk_launch_tile_kernel(void (*k)(NttPassArgs), std::atomic<uint64_t>& attr_done, int log_t, unsigned threads,
                                         size_t lds_bytes, const NttPassArgs& a, bool xcd, hipStream_t st) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (!(attr_done.load(std::memory_order_acquire) & bit)) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    attr_done.fetch_or(bit, std::memory_order_release);
  }
  const uint64_t tiles = (a.total + ((1ull << log_t) - 1)) >> log_t;
  if (tiles == 0) return hipSuccess;
  if (tiles > 0x7ffffff0ull) return hipErrorInvalidValue;
  NttPassArgs b = a;
  uint64_t grid = tiles;
  b.xcd_per = 0;
  if (xcd) {  // knobs.hpp: shk_ntt_choose_cell
    b.xcd_per = (uint32_t)((tiles + 7) / 8);
    grid = 8ull * b.xcd_per;
  }
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(threads), lds_bytes, st, b);
  return hipGetLastError();
}

// n <= 2: the reference's naive base case (_simple_ft, fft.py:287-300) is the whole transform.
static __global__ void ntt_tiny_kernel(const fp* src, fp* dst, uint32_t n, uint32_t batch, const fp* scale) {
  uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  if (n == 1) {
    fp_store(dst + b, fp_load(src + b));
    return;
  }
  fp x0 = fp_load(src + 2ull * b), x1 = fp_load(src + 2ull * b + 1);
  fp s = fp_add(x0, x1), d = fp_sub(x0, x1);
  if (scale) {
    fp sc = fp_load(scale);
    s = fp_mul(s, sc);
    d = fp_mul(d, sc);
  }
  fp_store(dst + 2ull * b, s);
  fp_store(dst + 2ull * b + 1, d);
}
