// Host-side check of the NTT tile passes' twiddle table in LDS (csrc/ntt_kernels.cuh: tile_tw_in_lds, tw_lds_slot, tile_tw_fill_chunk,
// tile_tw_exponent, tile_tw_needed), compiled with hipcc and run on the CPU.  For every cell the library instantiates:
//   * the qualification rule admits exactly the cells written out below, and the LDS size of a cell is image (+ table);
// and for every qualifying (LOG_R, LOG_T, LAST):
//   * the copy writes every 16-byte slot of the table region exactly once, and no slot outside it;
//   * for every register group, thread and twiddle product (the w^(R/4) product and the sparse first group's second and third twiddle
//     included) the four slots the kernel reads lie inside the region and hold the four chunks of the pair whose exponent the
//     global-memory path reads (the exponent is derived here from the rows a thread holds and a plain radix-2 DIF loop: ref_exponent);
//   * banking: a ds_read_b128 is served in four groups of 16 lanes (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32),
//     each lane four of the 64 banks wide, identical addresses broadcast; counted per wave, read and lane group,
//       - no bank sees more than ONE distinct address (the layout is conflict-free: every read costs its 4 LDS cycles), and
//       - wherever a lane group reads at most 8 distinct pairs -- every group but the row pass's first, whose lanes run along the row
//         and read 16 distinct pairs -- no bank quarter (16 banks, one pair wide) holds more than 2 of them.
//         A group of 16 distinct pairs has 4 to a quarter whatever the layout; the chunk rotation keeps those on different banks.
// Not enumerated: the banks of the copy's own ds_write_b128 (8 lanes at a time, 32-bank model) -- one or two stores per thread and tile
// against 52 reads.  What holds the arithmetic is the exact-residue GPU suite; this file holds the map.
#include <cstdio>
#include <map>
#include <set>
#include <vector>

#include "ntt_kernels.cuh"

static int failures = 0, cells = 0, qualifying = 0, reads = 0;
static int max_bank_ways = 0, max_quarter_small = 0, max_quarter_any = 0;

static void fail(const char* what, int log_r, int log_t, int last, int g, unsigned tid, int b) {
  if (!failures++) printf("R=2^%d T=2^%d last=%d group %d thread %u butterfly %d: %s\n", log_r, log_t, last, g, tid, b, what);
}

// The exponent the global path reads, from a plain radix-2 decimation-in-frequency transform of R points:
//   for q = LOG_R - 1 .. 0:  for every i with bit q clear:  (x[i], x[i + 2^q]) <- (x[i] + x[i + 2^q], (x[i] - x[i + 2^q]) * w_R^((i mod 2^q) * R / 2^(q + 1)))
// A thread of group g holds the rows ibase | (h << beta), h = 0..3; level lv of the group is q = LOG_R - 1 - 2 g - lv, and its two
// butterflies are the two pairs among those four rows that differ in bit q, pr = 0 for the pair with the lower rows.  Nothing of the
// kernel's own selection (tile_tw_exponent's local-bit arithmetic) is used: rows, pairs and the DIF formula only.  -1: no such level.
static long ref_exponent(int log_r, int g, int b, uint32_t ibase) {
  const int beta = (log_r - 2 * (g + 1)) > 0 ? (log_r - 2 * (g + 1)) : 0;
  const int q = (log_r - 1 - 2 * g) - (b >> 1);
  if (q < 0) return -1;
  uint32_t lower[4];
  int pairs = 0;
  for (uint32_t h = 0; h < 4; ++h) {
    const uint32_t i = ibase | (h << beta);
    if (i & (1u << q)) continue;  // the upper row of its pair
    bool partner = false;
    for (uint32_t h2 = 0; h2 < 4; ++h2) partner |= (ibase | (h2 << beta)) == (i | (1u << q));
    if (partner) lower[pairs++] = i;
  }
  if (pairs != 2) return -2;  // the group would not hold whole butterflies of this level
  const uint32_t i = (b & 1) ? (lower[0] > lower[1] ? lower[0] : lower[1]) : (lower[0] < lower[1] ? lower[0] : lower[1]);
  return (long)((i & ((1u << q) - 1u)) * ((1u << log_r) >> (q + 1)));
}

static const int kLaneGroup[64] = {0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1,
                                   2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 2, 2, 2, 2, 3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3};

template <int LOG_R, int LOG_T, bool LAST, int g>
static void check_group(const std::vector<int>& table) {
  constexpr int G = (LOG_R + 1) / 2;
  constexpr uint32_t threads = 1u << (LOG_R + LOG_T - 2), region = 2u << LOG_R;
  for (int b = 0; b < 4; ++b) {
    const bool sparse_extra = g == 0 && !LAST && LOG_R >= 4 && (b == 2 || b == 3);
    if (!tile_tw_needed<LOG_R, g>(b) && !sparse_extra) {
      for (uint32_t tid = 0; tid < threads; ++tid) {  // a product the kernel leaves out must be one by w^0, in every thread
        uint32_t t = 0, ibase = 0;
        tile_thread_coords<LOG_R, LOG_T, LAST, g>(tid, &t, &ibase);
        const long want = ref_exponent(LOG_R, g, b, ibase);
        if (want > 0 || want == -2) fail("a twiddle other than 1 is skipped", LOG_R, LOG_T, LAST, g, tid, b);
      }
      continue;
    }
    for (uint32_t wave0 = 0; wave0 < threads; wave0 += 64) {
      // [lane group][chunk read c] -> bank column -> distinct addresses, and bank quarter -> distinct pairs
      std::map<uint32_t, std::set<uint32_t>> by_bank[4][4], by_quarter[4][4];
      std::set<uint32_t> pairs[4];
      for (uint32_t tid = wave0; tid < wave0 + 64 && tid < threads; ++tid) {
        uint32_t t = 0, ibase = 0;
        tile_thread_coords<LOG_R, LOG_T, LAST, g>(tid, &t, &ibase);
        const long want = ref_exponent(LOG_R, g, b, ibase);
        if (want < 0) fail("reference: the level does not exist", LOG_R, LOG_T, LAST, g, tid, b);
        const uint32_t ex = tile_tw_exponent<LOG_R, g>(b, ibase);
        if ((long)ex != want || ex >= (1u << LOG_R) / 2) fail("exponent differs from the butterfly formula", LOG_R, LOG_T, LAST, g, tid, b);
        const uint32_t o = tw_lds_slot(ex, 0);
        const int lg = kLaneGroup[tid & 63u];
        pairs[lg].insert(ex);
        for (uint32_t c = 0; c < 4; ++c) {
          const uint32_t pos = o ^ c;  // what ntt_group's tw_load reads as chunk c
          ++reads;
          if (pos != tw_lds_slot(ex, c)) fail("o ^ c is not tw_lds_slot(ex, c)", LOG_R, LOG_T, LAST, g, tid, b);
          if (pos >= region) {
            fail("slot outside the table region", LOG_R, LOG_T, LAST, g, tid, b);
            continue;
          }
          if (table[pos] != (int)(4 * ex + c)) fail("slot holds another chunk than the global path reads", LOG_R, LOG_T, LAST, g, tid, b);
          by_bank[lg][c][pos & 15u].insert(pos);          // 16 bytes = banks 4 (pos mod 16) .. + 3
          by_quarter[lg][c][(pos >> 2) & 3u].insert(ex);  // 64 bytes = banks 16 (pair slot mod 4) .. + 15
        }
      }
      for (int lg = 0; lg < 4; ++lg)
        for (int c = 0; c < 4; ++c) {
          for (auto& kv : by_bank[lg][c])
            if ((int)kv.second.size() > max_bank_ways) max_bank_ways = (int)kv.second.size();
          for (auto& kv : by_quarter[lg][c]) {
            const int n = (int)kv.second.size();
            if (n > max_quarter_any) max_quarter_any = n;
            if (pairs[lg].size() <= 8 && n > max_quarter_small) max_quarter_small = n;
          }
        }
    }
  }
  if constexpr (g + 1 < G) check_group<LOG_R, LOG_T, LAST, g + 1>(table);
}

template <int LOG_R, int TILE_LOG>
static void check_cell() {
  if constexpr (shk_ntt_cell_exists(SHK_NTT_TILE, TILE_LOG, LOG_R)) {
    constexpr int LOG_T = TILE_LOG - LOG_R;
    ++cells;
    // written out: radix at most 2^9, and image + table (32 R bytes) times the workgroups per CU must fit 160 KiB -- at 16 waves per CU
    // for radix 2^8 and 2^9 (1024-element tiles: 4 x (32 + 8) KiB; 2048: 2 x (64 + 8 or 16) KiB), at 20 for the smaller radices, whose
    // 512- and 1024-element tiles (10 x 16 KiB, 5 x 32 KiB) leave no room: the 1024-element tile of radix 2^8, every 2048-element tile
    // to radix 2^9 and every 4096-element tile to radix 2^9
    constexpr bool want = SHK_TW_LDS && (TILE_LOG <= 9 ? false : TILE_LOG == 10 ? LOG_R == 8 : LOG_R <= 9);
    constexpr bool got = tile_tw_in_lds<LOG_R, LOG_T>();
    if (want != got && !failures++) printf("R=2^%d tile 2^%d: qualifies %d, expected %d\n", LOG_R, TILE_LOG, (int)got, (int)want);
    constexpr size_t bytes = tile_lds_bytes<LOG_R, LOG_T>();
    if (bytes != ((size_t)32 << TILE_LOG) + (got ? (size_t)32 << LOG_R : 0) && !failures++) printf("R=2^%d tile 2^%d: LDS size\n", LOG_R, TILE_LOG);
    if (got && bytes * ((size_t)(LOG_R >= 8 ? 16 : 20) >> (TILE_LOG - 8)) > 160 * 1024 && !failures++) printf("R=2^%d tile 2^%d: the table costs a workgroup\n", LOG_R, TILE_LOG);
    if constexpr (got) {
      ++qualifying;
      constexpr uint32_t threads = 1u << (TILE_LOG - 2), region = 2u << LOG_R;
      std::vector<int> table(region, -1);
      for (uint32_t tid = 0; tid < threads; ++tid)
        for (int k = 0; k < tile_tw_fill_chunks<LOG_R, LOG_T>(); ++k) {
          const int j = tile_tw_fill_chunk<LOG_R, LOG_T>(tid, k);
          if (j < 0) continue;
          const uint32_t pos = tw_lds_slot((uint32_t)j >> 2, (uint32_t)j & 3u);
          if (j >= (int)region || pos >= region || table[pos] != -1) {
            if (!failures++) printf("R=2^%d T=2^%d: the copy writes slot %u twice or leaves the region (chunk %d)\n", LOG_R, LOG_T, pos, j);
          } else {
            table[pos] = j;
          }
        }
      if (tile_tw_fill_chunks<LOG_R, LOG_T>() > 2 && !failures++) printf("R=2^%d T=2^%d: more than two chunks per thread\n", LOG_R, LOG_T);
      for (uint32_t pos = 0; pos < region; ++pos)
        if (table[pos] < 0 && !failures++) printf("R=2^%d T=2^%d: slot %u is never written\n", LOG_R, LOG_T, pos);
      check_group<LOG_R, LOG_T, false, 0>(table);
      check_group<LOG_R, LOG_T, true, 0>(table);
    }
  }
}

template <int TILE_LOG>
static void check_tile_size() {
  check_cell<2, TILE_LOG>();
  check_cell<3, TILE_LOG>();
  check_cell<4, TILE_LOG>();
  check_cell<5, TILE_LOG>();
  check_cell<6, TILE_LOG>();
  check_cell<7, TILE_LOG>();
  check_cell<8, TILE_LOG>();
  check_cell<9, TILE_LOG>();
  check_cell<10, TILE_LOG>();
  check_cell<11, TILE_LOG>();
}

int main() {
  check_tile_size<9>();
  check_tile_size<10>();
  check_tile_size<11>();
  check_tile_size<12>();
  printf("%d cells, %d with twiddles in LDS, %d chunk reads, at most %d addresses per bank, %d pairs per bank quarter (%d where a lane group "
         "reads 16 pairs), %d failures\n",
         cells, qualifying, reads, max_bank_ways, max_quarter_small, max_quarter_any, failures);
  return failures ? 1 : 0;
}
