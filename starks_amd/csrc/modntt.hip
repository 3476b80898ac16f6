// modntt.hip -- the kernels of the generic transform (sh_mod_ntt; modntt_items.cuh has the plan and the per-workgroup bodies,
// api_modntt.hip drives them).  One kernel runs any pass: a workgroup loads its tile into LDS, runs the tile's radix-2 stages with a
// barrier between them and stores the tile.  The modulus block is a kernel argument of every launch.
#include "internal.hpp"

namespace {

constexpr uint64_t GX = 1ull << 22;
inline dim3 grid_for_blocks(uint64_t blocks) {
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t block_id() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__global__ void __launch_bounds__(MN_WG) mn_pass_kernel(MnPass a, fpm_mod M, uint64_t tiles) {
  extern __shared__ uint4 mn_lds_raw[];
  fpm* lds = reinterpret_cast<fpm*>(mn_lds_raw);
  const uint64_t wg = block_id();
  if (wg >= tiles) return;  // uniform per workgroup
  mn_load_item(a, M, wg, threadIdx.x, lds);
  __syncthreads();
  for (uint32_t s = 1; s <= a.log_R; ++s) {
    mn_stage_item(a, M, s, wg, threadIdx.x, lds);
    __syncthreads();
  }
  mn_store_item(a, M, wg, threadIdx.x, lds);
}

__global__ void __launch_bounds__(MN_WG) mn_tw_kernel(MnTw t, fpm_mod M) {
  const uint64_t e = block_id() * MN_WG + threadIdx.x;
  if (e < t.count) mn_tw_item(t, M, e);
}

__global__ void __launch_bounds__(MN_WG) mn_pointwise_kernel(const fpm* x, const fpm* y, fpm* out, uint64_t n, fpm_mod M) {
  const uint64_t i = block_id() * MN_WG + threadIdx.x;
  if (i < n) mn_st(out + i, mn_pointwise_item(mn_ld(x + i), mn_ld(y + i), M));
}

}  // namespace

hipError_t shk_mn_pass(const MnPass& a, const fpm_mod& M, hipStream_t st) {
  const uint64_t tiles = mn_tiles(a);
  if (!tiles) return hipSuccess;
  const size_t lds = sizeof(fpm) << (a.log_T + a.log_R);
  hipLaunchKernelGGL(mn_pass_kernel, grid_for_blocks(tiles), dim3(MN_WG), lds, st, a, M, tiles);
  return hipGetLastError();
}
hipError_t shk_mn_tw(const MnTw& t, const fpm_mod& M, hipStream_t st) {
  if (!t.count) return hipSuccess;
  hipLaunchKernelGGL(mn_tw_kernel, grid_for_blocks((t.count + MN_WG - 1) / MN_WG), dim3(MN_WG), 0, st, t, M);
  return hipGetLastError();
}
hipError_t shk_mn_pointwise(const fpm* x, const fpm* y, fpm* out, uint64_t n, const fpm_mod& M, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(mn_pointwise_kernel, grid_for_blocks((n + MN_WG - 1) / MN_WG), dim3(MN_WG), 0, st, x, y, out, n, M);
  return hipGetLastError();
}
