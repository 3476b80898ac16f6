// modeval.hip -- the kernels of polynomial evaluation at arbitrary points over any prime modulus below 2^256 (sh_mod_poly_eval;
// modeval_items.cuh has the element steps, poly_items.cuh both drivers, api_modpoly.hip runs them).  poly_eval.hip's launches over fpm:
// the per-point table of x^(2^b) in Montgomery form, the Horner kernel with every workgroup's sum for its group of points, the second
// launch that adds the workgroups; and the tree path's chunk rows, broadcast product and per-point combine.  The modulus block is a
// kernel argument of every launch.
//
// Compiler figures for gfx950 (VGPRs / waves per SIMD; scratch 0 everywhere): pow_table 38 / 8, direct<4> 136 / 3 with 32 KiB of LDS,
// direct<1> 54 / 8 with 8 KiB, sum 48 / 8, chunks 16 / 8, bcast_mul 56 / 8, combine 66 / 7.  Four points per lane keep four
// accumulators, four powers, the coefficient and fpm_mul's nine-word sum live: 136 registers, three workgroups per CU, and every
// coefficient load feeds four independent product chains, as in poly_eval.hip.
#include "internal.hpp"
#include "modeval_items.cuh"

namespace {

constexpr int TPB = 256;
static_assert(PE_WG == TPB, "the direct kernel runs one workgroup of PE_WG lanes");

inline dim3 grid_for(uint64_t work) {
  const uint64_t blocks = (work + TPB - 1) / TPB;
  constexpr uint64_t GX = 1ull << 22;
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t block_id() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }
__device__ __forceinline__ uint64_t tid() { return block_id() * TPB + threadIdx.x; }

__global__ void __launch_bounds__(TPB) me_pow_table_kernel(const fpm* xs, uint64_t m, uint32_t lgS, fpm* tbl, fpm_mod M) {
  const uint64_t i = tid();
  if (i < m) me_pow_table_item(xs, m, lgS, tbl, i, M);
}

// workgroup (b, group, w): lanes g = w PE_WG + threadIdx.x of the group's points; dst[(b W + w) m + i] = the lanes' sum for point i.
// Every lane's value is canonical and fpm_add is exact, so the LDS tree below gives the same bits in any order and for any W.
template <int G>
__global__ void __launch_bounds__(TPB) me_direct_kernel(PeDirect s, const fpm* coefs, const fpm* tbl, fpm* dst, fpm_mod M) {
  __shared__ fpm red[G][TPB];
  const uint64_t blk = block_id();
  if (blk >= s.batch * s.groups * s.W) return;  // uniform per workgroup
  const uint64_t w = blk % s.W, bg = blk / s.W, grp = bg % s.groups, b = bg / s.groups, i0 = grp * G;
  const uint32_t lane = threadIdx.x;
  fpm acc[G];
  me_lane<G>(s, coefs + b * s.n, tbl, i0, w * TPB + lane, acc, M);
#pragma unroll
  for (int q = 0; q < G; ++q) red[q][lane] = acc[q];
  __syncthreads();
  for (uint32_t h = TPB / 2; h > 0; h >>= 1) {
    if (lane < h) {
#pragma unroll
      for (int q = 0; q < G; ++q) red[q][lane] = fpm_add(red[q][lane], red[q][lane + h], M);
    }
    __syncthreads();
  }
  if (lane < G && i0 + lane < s.m) mn_st(dst + (b * s.W + w) * s.m + i0 + lane, red[lane][0]);
}

__global__ void __launch_bounds__(TPB) me_sum_kernel(PeDirect s, const fpm* part, fpm* out, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= s.batch * s.m) return;
  const uint64_t b = g / s.m, i = g - b * s.m;
  mn_st(out + g, me_sum_item(s, part, b, i, M));
}

__global__ void __launch_bounds__(TPB) me_chunks_kernel(const fpm* coefs, uint64_t n, uint64_t N, uint64_t C, uint64_t total, fpm* dst) {
  const uint64_t g = tid();
  if (g >= total) return;
  const uint64_t r = g / N, k = g - r * N;
  mn_st(dst + g, me_chunk_rev_item(coefs, n, N, C, r, k));
}

__global__ void __launch_bounds__(TPB) me_bcast_mul_kernel(fpm* a, const fpm* b, uint64_t len, uint64_t total, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= total) return;
  mn_st(a + g, me_bcast_mul_item(mn_ld(a + g), mn_ld(b + g % len), M));
}

__global__ void __launch_bounds__(TPB) me_combine_kernel(const fpm* leaves, const fpm* xs, uint64_t m, uint64_t N, uint64_t C,
                                                         uint64_t total, fpm* out, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= total) return;
  const uint64_t b = g / m, i = g - b * m;
  mn_st(out + g, me_combine_item(leaves, xs, N, C, b, i, M));
}

}  // namespace

hipError_t shk_me_pow_table(const fpm* xs, uint64_t m, uint32_t lgS, fpm* tbl, const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(me_pow_table_kernel, grid_for(m), dim3(TPB), 0, st, xs, m, lgS, tbl, M);
  return hipGetLastError();
}
hipError_t shk_me_direct(const PeDirect& s, const fpm* coefs, const fpm* tbl, fpm* dst, const fpm_mod& M, hipStream_t st) {
  const dim3 grid = grid_for(s.batch * s.groups * s.W * TPB);
  if (s.G == ME_GROUP)
    hipLaunchKernelGGL(me_direct_kernel<ME_GROUP>, grid, dim3(TPB), 0, st, s, coefs, tbl, dst, M);
  else if (s.G == 1)
    hipLaunchKernelGGL(me_direct_kernel<1>, grid, dim3(TPB), 0, st, s, coefs, tbl, dst, M);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t shk_me_sum(const PeDirect& s, const fpm* part, fpm* out, const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(me_sum_kernel, grid_for(s.batch * s.m), dim3(TPB), 0, st, s, part, out, M);
  return hipGetLastError();
}
hipError_t shk_me_chunks(const fpm* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, fpm* dst, hipStream_t st) {
  const uint64_t total = batch * C * N;
  hipLaunchKernelGGL(me_chunks_kernel, grid_for(total), dim3(TPB), 0, st, coefs, n, N, C, total, dst);
  return hipGetLastError();
}
hipError_t shk_me_bcast_mul(fpm* a, const fpm* b, uint64_t rows, uint64_t len, const fpm_mod& M, hipStream_t st) {
  const uint64_t total = rows * len;
  hipLaunchKernelGGL(me_bcast_mul_kernel, grid_for(total), dim3(TPB), 0, st, a, b, len, total, M);
  return hipGetLastError();
}
hipError_t shk_me_combine(const fpm* leaves, const fpm* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, fpm* out, const fpm_mod& M,
                          hipStream_t st) {
  const uint64_t total = batch * m;
  hipLaunchKernelGGL(me_combine_kernel, grid_for(total), dim3(TPB), 0, st, leaves, xs, m, N, C, total, out, M);
  return hipGetLastError();
}
