// Resident workgroups per CU of every NTT tile cell that keeps its twiddles in LDS (csrc/ntt_kernels.cuh: tile_tw_in_lds), as the
// runtime computes them for the library's own kernels (linked from libstarkhip.so, nothing is compiled for the device here): one line
//   log_R log_T last lds_image lds_image_plus_table blocks_at_image blocks_at_image_plus_table
// per cell.  The table must never cost a workgroup: two of the cells fill the 160 KiB exactly, so an allocation granule that does not
// divide their size shows here and nowhere else (tests/test_gpu_ntt_tw_lds.py compares the two counts).
#include <cstdio>

#include "ntt_kernels.cuh"

// (log_R, log_T) of the qualifying cells: the 1024-element tile of radix 2^8, 2048- and 4096-element tiles to radix 2^9 (4096 from 2^4)
#define TW_LDS_CELLS(X)                                           \
  X(8, 2)                                                         \
  X(2, 9) X(3, 8) X(4, 7) X(5, 6) X(6, 5) X(7, 4) X(8, 3) X(9, 2) \
  X(4, 8) X(5, 7) X(6, 6) X(7, 5) X(8, 4) X(9, 3)

#define DECLARE(R, T)                                                     \
  extern template __global__ void ntt_pass_kernel<R, T, false>(NttPassArgs); \
  extern template __global__ void ntt_pass_kernel<R, T, true>(NttPassArgs);
TW_LDS_CELLS(DECLARE)

static int failures = 0, listed = 0;

template <int LOG_R, int LOG_T, bool LAST>
static void one() {
  static_assert(shk_ntt_cell_exists(SHK_NTT_TILE, LOG_R + LOG_T, LOG_R) && tile_tw_in_lds<LOG_R, LOG_T>(), "not a qualifying cell");
  const void* k = reinterpret_cast<const void*>(&ntt_pass_kernel<LOG_R, LOG_T, LAST>);
  const size_t image = (size_t)32 << (LOG_R + LOG_T), both = tile_lds_bytes<LOG_R, LOG_T>();
  const int threads = 1 << (LOG_R + LOG_T - 2);
  int at_image = -1, at_both = -1;
  hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)both);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&at_image, k, threads, image);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&at_both, k, threads, both);
  if (e != hipSuccess) {
    ++failures;
    fprintf(stderr, "R=2^%d T=2^%d last=%d: %s\n", LOG_R, LOG_T, (int)LAST, hipGetErrorString(e));
  }
  printf("%d %d %d %zu %zu %d %d\n", LOG_R, LOG_T, (int)LAST, image, both, at_image, at_both);
  ++listed;
}

constexpr int qualifying_cells() {
  int n = 0;
  for (int tl = 9; tl <= 12; ++tl)
    for (int r = 2; r <= 11; ++r)
      if (shk_ntt_cell_exists(SHK_NTT_TILE, tl, r) && r <= 9 && ((32L << tl) + (32L << r)) * ((r >= 8 ? 16 : 20) >> (tl - 8)) <= 160L * 1024) ++n;
  return n;
}

int main() {
#define RUN(R, T)      \
  one<R, T, false>();  \
  one<R, T, true>();
  TW_LDS_CELLS(RUN)
  if (listed != 2 * qualifying_cells()) {
    ++failures;
    fprintf(stderr, "%d kernels listed, the rule admits %d\n", listed, 2 * qualifying_cells());
  }
  return failures ? 1 : 0;
}
