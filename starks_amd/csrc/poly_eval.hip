// poly_eval.hip -- the kernels of polynomial evaluation at arbitrary points (sh_poly_eval; poly_items.cuh has the element steps and
// both drivers, api_poly.hip runs them).  The direct path: a small kernel builds each point's table of x^(2^b), the Horner kernel gives
// every workgroup's sum for its group of points, a second launch adds the workgroups.  The tree path's kernels: the chunks of the
// coefficients reversed into rows, one transform multiplied into every row, the chunks combined per point.
#include "internal.hpp"
#include "poly_items.cuh"

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

__global__ void __launch_bounds__(TPB) pow_table_kernel(const fp* xs, uint64_t m, uint32_t lgS, fp* tbl) {
  const uint64_t i = tid();
  if (i < m) pe_pow_table_item(xs, m, lgS, tbl, i);
}

// workgroup (b, group, w): lanes g = w PE_WG + threadIdx.x of the group's points; dst[(b W + w) m + i] = the lanes' sum for point i
template <int G>
__global__ void __launch_bounds__(TPB) direct_kernel(PeDirect s, const fp* coefs, const fp* tbl, fp* dst) {
  __shared__ fp red[G][TPB];
  const uint64_t blk = block_id();
  if (blk >= s.batch * s.groups * s.W) return;  // uniform per workgroup
  const uint64_t w = blk % s.W, bg = blk / s.W, grp = bg % s.groups, b = bg / s.groups, i0 = grp * G;
  const uint32_t lane = threadIdx.x;
  fp acc[G];
  pe_lane<G>(s, coefs + b * s.n, tbl, i0, w * TPB + lane, acc);
#pragma unroll
  for (int q = 0; q < G; ++q) red[q][lane] = acc[q];
  __syncthreads();
  for (uint32_t h = TPB / 2; h > 0; h >>= 1) {
    if (lane < h) {
#pragma unroll
      for (int q = 0; q < G; ++q) red[q][lane] = fp_add(red[q][lane], red[q][lane + h]);
    }
    __syncthreads();
  }
  if (lane < G && i0 + lane < s.m) {
    const fp v = red[lane][0];
    fp_store(dst + (b * s.W + w) * s.m + i0 + lane, s.W == 1 ? fp_canon(v) : v);
  }
}

__global__ void __launch_bounds__(TPB) sum_kernel(PeDirect s, const fp* part, fp* out) {
  const uint64_t g = tid();
  if (g >= s.batch * s.m) return;
  const uint64_t b = g / s.m, i = g - b * s.m;
  fp_store(out + g, pe_sum_item(s, part, b, i));
}

__global__ void __launch_bounds__(TPB) chunks_kernel(const fp* coefs, uint64_t n, uint64_t N, uint64_t C, uint64_t total, fp* dst) {
  const uint64_t g = tid();
  if (g >= total) return;
  const uint64_t r = g / N, k = g - r * N;
  fp_store(dst + g, pe_chunk_rev_item(coefs, n, N, C, r, k));
}

__global__ void __launch_bounds__(TPB) bcast_mul_kernel(fp* a, const fp* b, uint64_t len, uint64_t total) {
  const uint64_t g = tid();
  if (g >= total) return;
  fp_store(a + g, fp_mul(fp_load(a + g), fp_load(b + g % len)));
}

__global__ void __launch_bounds__(TPB) combine_kernel(const fp* leaves, const fp* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t total,
                                                      fp* out) {
  const uint64_t g = tid();
  if (g >= total) return;
  const uint64_t b = g / m, i = g - b * m;
  fp_store(out + g, pe_combine_item(leaves, xs, N, C, b, i));
}

}  // namespace

hipError_t shk_pe_pow_table(const fp* xs, uint64_t m, uint32_t lgS, fp* tbl, hipStream_t st) {
  hipLaunchKernelGGL(pow_table_kernel, grid_for(m), dim3(TPB), 0, st, xs, m, lgS, tbl);
  return hipGetLastError();
}
hipError_t shk_pe_direct(const PeDirect& s, const fp* coefs, const fp* tbl, fp* dst, hipStream_t st) {
  const dim3 grid = grid_for(s.batch * s.groups * s.W * TPB);
  if (s.G == PE_GROUP)
    hipLaunchKernelGGL(direct_kernel<PE_GROUP>, grid, dim3(TPB), 0, st, s, coefs, tbl, dst);
  else
    hipLaunchKernelGGL(direct_kernel<1>, grid, dim3(TPB), 0, st, s, coefs, tbl, dst);
  return hipGetLastError();
}
hipError_t shk_pe_sum(const PeDirect& s, const fp* part, fp* out, hipStream_t st) {
  hipLaunchKernelGGL(sum_kernel, grid_for(s.batch * s.m), dim3(TPB), 0, st, s, part, out);
  return hipGetLastError();
}
hipError_t shk_pe_chunks(const fp* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, fp* dst, hipStream_t st) {
  const uint64_t total = batch * C * N;
  hipLaunchKernelGGL(chunks_kernel, grid_for(total), dim3(TPB), 0, st, coefs, n, N, C, total, dst);
  return hipGetLastError();
}
hipError_t shk_pe_bcast_mul(fp* a, const fp* b, uint64_t rows, uint64_t len, hipStream_t st) {
  const uint64_t total = rows * len;
  hipLaunchKernelGGL(bcast_mul_kernel, grid_for(total), dim3(TPB), 0, st, a, b, len, total);
  return hipGetLastError();
}
hipError_t shk_pe_combine(const fp* leaves, const fp* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, fp* out, hipStream_t st) {
  const uint64_t total = batch * m;
  hipLaunchKernelGGL(combine_kernel, grid_for(total), dim3(TPB), 0, st, leaves, xs, m, N, C, total, out);
  return hipGetLastError();
}
