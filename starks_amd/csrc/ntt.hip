// ntt.hip -- instantiations and launchers of the NTT tile passes (ntt_kernels.cuh).
#include <stdlib.h>

#include <atomic>

#include "knobs.hpp"
#include "ntt_kernels.cuh"

namespace {

template <int LOG_R, bool LAST, int TILE_LOG>
hipError_t launch_tile(const NttPassArgs& a, bool xcd, hipStream_t st) {
  constexpr int LOG_T = TILE_LOG - LOG_R;
  static std::atomic<uint64_t> attr_done{0};
  return shk_launch_tile_kernel(ntt_pass_kernel<LOG_R, LOG_T, LAST>, attr_done, LOG_T, 1u << (TILE_LOG - 2),
                                tile_lds_bytes<LOG_R, LOG_T>(), a, xcd, st);
}

// narrow launches (ntt_kernels.cuh): one butterfly per thread, 1024-element tiles of 512 threads or 512-element tiles of 256
template <int LOG_R, bool LAST, int TILE_LOG>
hipError_t launch_narrow(const NttPassArgs& a, hipStream_t st) {
  constexpr int LOG_T = TILE_LOG - LOG_R;
  const uint64_t tiles = (a.total + ((1ull << LOG_T) - 1)) >> LOG_T;
  if (tiles == 0 || tiles > 0x7ffffff0ull) return hipErrorInvalidValue;  // the kernel clamps to column total - 1
  hipLaunchKernelGGL((ntt_narrow_pass_kernel<LOG_R, LOG_T, LAST>), dim3((unsigned)tiles), dim3(1u << (TILE_LOG - 1)), 0, st, a);
  return hipGetLastError();
}

// The one switch over the instantiations: exactly the cells of shk_ntt_cell_exists (knobs.hpp) are compiled.
template <int LOG_R, bool LAST>
hipError_t launch_cell(const ShkNttCell& c, const NttPassArgs& a, hipStream_t st) {
  if (c.form == SHK_NTT_NARROW) {
    if (c.xcd) return hipErrorInvalidValue;
    if constexpr (shk_ntt_cell_exists(SHK_NTT_NARROW, 10, LOG_R)) {
      if (c.tile_log == 10) return launch_narrow<LOG_R, LAST, 10>(a, st);
    }
    if constexpr (shk_ntt_cell_exists(SHK_NTT_NARROW, 9, LOG_R)) {
      if (c.tile_log == 9) return launch_narrow<LOG_R, LAST, 9>(a, st);
    }
    return hipErrorInvalidValue;
  }
  if constexpr (shk_ntt_cell_exists(SHK_NTT_TILE, 12, LOG_R)) {
    if (c.tile_log == 12) return launch_tile<LOG_R, LAST, 12>(a, c.xcd, st);
  }
  if constexpr (shk_ntt_cell_exists(SHK_NTT_TILE, 11, LOG_R)) {
    if (c.tile_log == 11) return launch_tile<LOG_R, LAST, 11>(a, c.xcd, st);
  }
  if constexpr (shk_ntt_cell_exists(SHK_NTT_TILE, 10, LOG_R)) {
    if (c.tile_log == 10) return launch_tile<LOG_R, LAST, 10>(a, c.xcd, st);
  }
  if constexpr (shk_ntt_cell_exists(SHK_NTT_TILE, 9, LOG_R)) {
    if (c.tile_log == 9) return launch_tile<LOG_R, LAST, 9>(a, c.xcd, st);
  }
  return hipErrorInvalidValue;
}

template <bool LAST>
hipError_t dispatch(const ShkNttCell& c, int log_R, const NttPassArgs& a, hipStream_t st) {
  switch (log_R) {
    case 2: return launch_cell<2, LAST>(c, a, st);
    case 3: return launch_cell<3, LAST>(c, a, st);
    case 4: return launch_cell<4, LAST>(c, a, st);
    case 5: return launch_cell<5, LAST>(c, a, st);
    case 6: return launch_cell<6, LAST>(c, a, st);
    case 7: return launch_cell<7, LAST>(c, a, st);
    case 8: return launch_cell<8, LAST>(c, a, st);
    case 9: return launch_cell<9, LAST>(c, a, st);
    case 10: return launch_cell<10, LAST>(c, a, st);
    case 11: return launch_cell<11, LAST>(c, a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t shk_launch_ntt_cell(const ShkNttCell& c, int log_R, bool last, const NttPassArgs& a, hipStream_t st) {
  if (!shk_ntt_cell_exists(c.form, c.tile_log, log_R)) return hipErrorInvalidValue;
  return last ? dispatch<true>(c, log_R, a, st) : dispatch<false>(c, log_R, a, st);
}

// the library's own choice (knobs.hpp: shk_ntt_choose_cell, under the knobs of the process), then that cell
hipError_t shk_launch_ntt_pass(int log_R, bool last, const NttPassArgs& a, hipStream_t st) {
  const ShkNttPassShape shape{a.total, a.log_n, a.log_S, a.pass_index};
  const ShkNttCell c = shk_ntt_choose_cell(shk_knobs(), log_R, last, shape);
  if (c.form == SHK_NTT_NONE) return hipErrorInvalidValue;
  return shk_launch_ntt_cell(c, log_R, last, a, st);
}

hipError_t shk_launch_ntt_tiny(const fp* src, fp* dst, uint32_t n, uint32_t batch, const fp* scale, hipStream_t st) {
  if (batch == 0) return hipSuccess;
  hipLaunchKernelGGL(ntt_tiny_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, src, dst, n, batch, scale);
  return hipGetLastError();
}
