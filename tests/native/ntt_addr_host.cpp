// Host-side check of the addresses the NTT tile passes form from one value per thread (csrc/ntt_kernels.cuh: tile_tw_byte,
// tile_tw_pair_xor, tile_out_k_step), compiled with hipcc and run on the CPU.  The helpers are the header's own, nothing is restated.
//   * Twiddle pairs in LDS.  For every cell that tile_tw_in_lds admits, both pass kinds, every register group, thread and butterfly
//     (the sparse first group's second and third included), the byte address of each of the four reads -- the level's one address, XOR
//     the pair constant, XOR 16 c -- is 16 * tw_lds_slot(tile_tw_exponent<LOG_R, g>(b, ibase), c), inside the table region; and the pair
//     constant is what one level bit of the row index adds to the slot.
//   * Output rows.  For LOG_R = 2 .. 11 and every row base with bits 0 and 1 clear, the frequency of element h,
//     bitrev(ibase | h) >> (32 - LOG_R), is that of h = 0 plus tile_out_k_step<LOG_R>(h) = {0, R/2, R/4, 3R/4}[h].
#include <cstdio>

#include "ntt_kernels.cuh"

static int failures = 0, cells = 0;
static long reads = 0, rows = 0;

static void fail(const char* what, int log_r, int log_t, int last, int g, unsigned tid, int b) {
  if (!failures++) printf("R=2^%d T=2^%d last=%d group %d thread %u butterfly %d: %s\n", log_r, log_t, last, g, tid, b, what);
}

static uint32_t bitrev32(uint32_t x) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
  return r;
}

template <int LOG_R, int LOG_T, bool LAST, int g, int b>
static void check_butterfly() {
  constexpr uint32_t threads = 1u << (LOG_R + LOG_T - 2), region_bytes = 32u << LOG_R;
  constexpr bool sparse_extra = g == 0 && !LAST && LOG_R >= 4 && (b == 2 || b == 3);
  if constexpr (tile_tw_needed<LOG_R, g>(b) || sparse_extra) {  // the products the kernel has: nothing else is instantiated there
    const uint32_t px = tile_tw_pair_xor<LOG_R, g>(b);
    // the constant's bits above the key (8 and up) are added, not XOR-ed (they go into the read's immediate offset): they must be clear
    const uint32_t added = px & ~0xffu;
    if ((b & 1) == 0 && px != 0) fail("the first butterfly of a level has a pair constant", LOG_R, LOG_T, LAST, g, 0, b);
    for (uint32_t tid = 0; tid < threads; ++tid) {
      uint32_t t = 0, ibase = 0;
      tile_thread_coords<LOG_R, LOG_T, LAST, g>(tid, &t, &ibase);
      const uint32_t ex = tile_tw_exponent<LOG_R, g>(b, ibase);
      const uint32_t level = tile_tw_byte<LOG_R, g>(b & ~1, ibase, 0);  // the one address a thread forms for the level
      for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t addr = tile_tw_byte<LOG_R, g>(b, ibase, c);
        ++reads;
        // the kernel's own expression: the address it forms for the level, then the read of chunk c
        if (tile_tw_read<LOG_R, g, b>(tile_tw_level<LOG_R, g, b>(ibase), ibase, c) != addr)
          fail("the kernel's read (tile_tw_level, tile_tw_read) is not tile_tw_byte", LOG_R, LOG_T, LAST, g, tid, b);
        if (!tile_tw_keyed<LOG_R, g, b>() && tile_tw_level<LOG_R, g, b>(ibase) != level)
          fail("a pair without key bits 6, 7 changes the level's address", LOG_R, LOG_T, LAST, g, tid, b);
        if ((level ^ (16u * c)) & added) fail("an added pair constant meets a set bit", LOG_R, LOG_T, LAST, g, tid, b);
        if (addr != (level ^ px ^ (16u * c))) fail("the read is not the level's address XOR the constants", LOG_R, LOG_T, LAST, g, tid, b);
        if (addr != 16u * tw_lds_slot(ex, c)) fail("address differs from 16 * tw_lds_slot(exponent, c)", LOG_R, LOG_T, LAST, g, tid, b);
        if (addr >= region_bytes) fail("address outside the table region", LOG_R, LOG_T, LAST, g, tid, b);
      }
    }
  }
}

template <int LOG_R, int LOG_T, bool LAST, int g>
static void check_group() {
  constexpr int G = (LOG_R + 1) / 2;
  check_butterfly<LOG_R, LOG_T, LAST, g, 0>();
  check_butterfly<LOG_R, LOG_T, LAST, g, 1>();
  check_butterfly<LOG_R, LOG_T, LAST, g, 2>();
  check_butterfly<LOG_R, LOG_T, LAST, g, 3>();
  if constexpr (g + 1 < G) check_group<LOG_R, LOG_T, LAST, g + 1>();
}

template <int LOG_R, int TILE_LOG>
static void check_cell() {
  if constexpr (shk_ntt_cell_exists(SHK_NTT_TILE, TILE_LOG, LOG_R)) {
    constexpr int LOG_T = TILE_LOG - LOG_R;
    if constexpr (tile_tw_in_lds<LOG_R, LOG_T>()) {
      ++cells;
      check_group<LOG_R, LOG_T, false, 0>();
      check_group<LOG_R, LOG_T, true, 0>();
    }
  }
}

template <int LOG_R>
static void check_radix() {
  check_cell<LOG_R, 9>();
  check_cell<LOG_R, 10>();
  check_cell<LOG_R, 11>();
  check_cell<LOG_R, 12>();
  // output rows: every row base of the last group (bits 0 and 1 clear)
  static const uint32_t want[4] = {0u, (1u << LOG_R) / 2, (1u << LOG_R) / 4, 3 * ((1u << LOG_R) / 4)};
  for (uint32_t ibase = 0; ibase < (1u << LOG_R); ibase += 4) {
    const uint32_t k0 = bitrev32(ibase) >> (32 - LOG_R);
    for (int h = 0; h < 4; ++h) {
      ++rows;
      const uint32_t k = bitrev32(ibase | (uint32_t)h) >> (32 - LOG_R);
      if (tile_out_k_step<LOG_R>(h) != want[h] || k != k0 + tile_out_k_step<LOG_R>(h) || k >= (1u << LOG_R))
        fail("frequency of element h is not k_0 + step(h)", LOG_R, 0, 0, -1, ibase, h);
    }
  }
}

int main() {
  check_radix<2>();
  check_radix<3>();
  check_radix<4>();
  check_radix<5>();
  check_radix<6>();
  check_radix<7>();
  check_radix<8>();
  check_radix<9>();
  check_radix<10>();
  check_radix<11>();
  printf("%d cells with twiddles in LDS, %ld chunk reads, %ld output rows, %d failures\n", cells, reads, rows, failures);
  return failures ? 1 : 0;
}
