// ntt64.hip -- the kernels of the packed-word transform (sh_mod64_ntt; ntt64_items.cuh has the plan, the index maps and the
// per-workgroup bodies, api_ntt64.hip drives them).  One kernel runs any pass: a workgroup loads its tile into LDS, runs the tile's
// stages in register groups of up to three with a barrier between the groups, and stores the tile.  The modulus block is a kernel
// argument of every launch.  Workgroup and element offsets are 64-bit throughout: 2^28 elements of 8 bytes pass 2^31.
#include "internal.hpp"

namespace {

constexpr uint64_t GX = 1ull << 22;
inline dim3 grid_for_blocks(uint64_t blocks) {
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t block_id() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

__global__ void __launch_bounds__(N64_WG) n64_pass_kernel(N64Pass a, f64_mod M, uint64_t tiles) {
  extern __shared__ uint4 n64_lds_raw[];
  uint64_t* lds = reinterpret_cast<uint64_t*>(n64_lds_raw);
  const uint64_t wg = block_id();
  if (wg >= tiles) return;  // uniform per workgroup
  n64_load_item(a, M, wg, threadIdx.x, lds);
  __syncthreads();
  const uint32_t groups = n64_groups(a.log_R);
  for (uint32_t g = 0; g < groups; ++g) {
    n64_group_any(a, M, g, wg, threadIdx.x, lds);
    __syncthreads();
  }
  n64_store_item(a, M, wg, threadIdx.x, lds);
}

__global__ void __launch_bounds__(N64_WG) n64_tw_kernel(N64Tw t, f64_mod M, uint64_t count) {
  const uint64_t i = block_id() * N64_WG + threadIdx.x;
  if (i < count) n64_tw_item(t, M, i);
}

__global__ void __launch_bounds__(N64_WG) n64_pointwise_kernel(const uint64_t* x, const uint64_t* y, uint64_t* out, uint64_t n, f64_mod M) {
  const uint64_t i = block_id() * N64_WG + threadIdx.x;
  if (i < n) out[i] = n64_pointwise_item(x[i], y[i], M);
}

__global__ void __launch_bounds__(N64_WG) n64_from_limbs_kernel(const uint4* limbs, uint64_t* words, uint64_t count, f64_mod M) {
  const uint64_t i = block_id() * N64_WG + threadIdx.x;
  if (i >= count) return;
  const uint4 lo = limbs[2 * i], hi = limbs[2 * i + 1];
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  words[i] = f64_from_limbs(w, M);
}

__global__ void __launch_bounds__(N64_WG) n64_to_limbs_kernel(const uint64_t* words, uint4* limbs, uint64_t count) {
  const uint64_t i = block_id() * N64_WG + threadIdx.x;
  if (i >= count) return;
  const uint64_t v = words[i];
  limbs[2 * i] = make_uint4((uint32_t)v, (uint32_t)(v >> 32), 0u, 0u);
  limbs[2 * i + 1] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

hipError_t shk_n64_pass(const N64Pass& a, const f64_mod& M, hipStream_t st) {
  const uint64_t tiles = n64_tiles(a);
  if (!tiles) return hipSuccess;
  const size_t lds = sizeof(uint64_t) << (a.log_T + a.log_R);
  hipLaunchKernelGGL(n64_pass_kernel, grid_for_blocks(tiles), dim3(N64_WG), lds, st, a, M, tiles);
  return hipGetLastError();
}
hipError_t shk_n64_tw(const N64Tw& t, const f64_mod& M, hipStream_t st) {
  const uint64_t count = n64_table_entries(t);
  hipLaunchKernelGGL(n64_tw_kernel, grid_for_blocks((count + N64_WG - 1) / N64_WG), dim3(N64_WG), 0, st, t, M, count);
  return hipGetLastError();
}
hipError_t shk_n64_pointwise(const uint64_t* x, const uint64_t* y, uint64_t* out, uint64_t n, const f64_mod& M, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(n64_pointwise_kernel, grid_for_blocks((n + N64_WG - 1) / N64_WG), dim3(N64_WG), 0, st, x, y, out, n, M);
  return hipGetLastError();
}
hipError_t shk_n64_from_limbs(const void* limbs, uint64_t* words, uint64_t count, const f64_mod& M, hipStream_t st) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(n64_from_limbs_kernel, grid_for_blocks((count + N64_WG - 1) / N64_WG), dim3(N64_WG), 0, st,
                     reinterpret_cast<const uint4*>(limbs), words, count, M);
  return hipGetLastError();
}
hipError_t shk_n64_to_limbs(const uint64_t* words, void* limbs, uint64_t count, hipStream_t st) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(n64_to_limbs_kernel, grid_for_blocks((count + N64_WG - 1) / N64_WG), dim3(N64_WG), 0, st, words,
                     reinterpret_cast<uint4*>(limbs), count);
  return hipGetLastError();
}
