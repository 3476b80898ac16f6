// poly_arith.hip -- the pointwise and per-node kernels of polynomial products, division, zpoly and lagrange_interp
// (poly_items.cuh has the algebra; api_poly.hip drives the levels with batched NTT plans).  Every kernel is one thread per output
// element and memory-bound: a level moves its [nodes][2d] transforms through once.
#include "internal.hpp"
#include "poly_items.cuh"

namespace {

constexpr int TPB = 256;

inline dim3 grid_for(uint64_t work) {
  const uint64_t blocks = (work + TPB - 1) / TPB;
  constexpr uint64_t GX = 1ull << 22;
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t tid() { return ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * TPB + threadIdx.x; }

__global__ void __launch_bounds__(TPB) copy_kernel(PaCopy c, const fp* src, fp* dst) {
  const uint64_t g = tid();
  if (g >= c.rows * c.len) return;
  const uint64_t r = g / c.len, k = g - r * c.len;
  fp_store(dst + r * c.ds + k, pa_copy_item(c, src, r, k));
}

// out rows j < nodes/2 of 2d = 2^log2d: the parent of transformed rows 2j, 2j + 1
__global__ void __launch_bounds__(TPB) tree_kernel(const fp* hz, fp* oz, const fp* hn, fp* on, uint32_t log2d, uint64_t total) {
  const uint64_t g = tid();
  if (g >= total) return;
  const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1);
  const uint64_t a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
  const fp A = fp_load(hz + a), B = fp_load(hz + b);
  if (oz) fp_store(oz + g, pa_tree_node(A, B, i));
  if (on) fp_store(on + g, pa_num_node(fp_load(hn + a), fp_load(hn + b), A, B, i));
}

// children c = 2j, 2j + 1 at index i: hr[c] <- hd[j] * hr[c ^ 1]  (one thread per sibling pair)
__global__ void __launch_bounds__(TPB) mid_kernel(const fp* hd, fp* hr, uint32_t log2d, uint64_t pairs_total) {
  const uint64_t g = tid();
  if (g >= pairs_total) return;
  const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1);
  const uint64_t a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
  const fp D = fp_load(hd + g), RA = fp_load(hr + a), RB = fp_load(hr + b);
  fp_store(hr + a, fp_mul(D, RB));
  fp_store(hr + b, fp_mul(D, RA));
}

__global__ void __launch_bounds__(TPB) newton_kernel(const fp* F, fp* G, uint64_t n) {
  const uint64_t g = tid();
  if (g >= n) return;
  fp_store(G + g, pa_newton(fp_load(F + g), fp_load(G + g)));
}

__global__ void inv1_kernel(const fp* src, fp* dst) {
  if (threadIdx.x == 0) fp_store(dst, fp_inv(fp_canon(fp_load(src))));
}

__global__ void __launch_bounds__(TPB) deriv_rev_kernel(const fp* top, fp* out, uint64_t N, uint64_t n) {
  const uint64_t g = tid();
  if (g >= N) return;
  fp_store(out + g, pa_deriv_rev(top, N, n, g));
}

__global__ void __launch_bounds__(TPB) weights_kernel(const fp* ys, const fp* inv, fp* out, uint64_t n, uint64_t N) {
  const uint64_t g = tid();
  if (g >= N) return;
  fp_store(out + g, g < n ? pa_weight(fp_load(ys + g), fp_load(inv + g)) : fp_zero());
}

__global__ void __launch_bounds__(TPB) sub_kernel(const fp* a, const fp* b, fp* out, uint64_t n) {
  const uint64_t g = tid();
  if (g >= n) return;
  fp_store(out + g, fp_canon(fp_sub(fp_load(a + g), fp_load(b + g))));
}

}  // namespace

hipError_t shk_pa_copy(const PaCopy& c, const fp* src, fp* dst, hipStream_t st) {
  if (!c.rows || !c.len) return hipSuccess;
  hipLaunchKernelGGL(copy_kernel, grid_for(c.rows * c.len), dim3(TPB), 0, st, c, src, dst);
  return hipGetLastError();
}
hipError_t shk_pa_tree(const fp* hz, fp* oz, const fp* hn, fp* on, uint32_t log2d, uint64_t nodes, hipStream_t st) {
  const uint64_t total = (nodes / 2) << log2d;
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(tree_kernel, grid_for(total), dim3(TPB), 0, st, hz, oz, hn, on, log2d, total);
  return hipGetLastError();
}
hipError_t shk_pa_mid(const fp* hd, fp* hr, uint32_t log2d, uint64_t children, hipStream_t st) {
  const uint64_t total = (children / 2) << log2d;
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(mid_kernel, grid_for(total), dim3(TPB), 0, st, hd, hr, log2d, total);
  return hipGetLastError();
}
hipError_t shk_pa_newton(const fp* F, fp* G, uint64_t n, hipStream_t st) {
  hipLaunchKernelGGL(newton_kernel, grid_for(n), dim3(TPB), 0, st, F, G, n);
  return hipGetLastError();
}
hipError_t shk_pa_inv1(const fp* src, fp* dst, hipStream_t st) {
  hipLaunchKernelGGL(inv1_kernel, dim3(1), dim3(64), 0, st, src, dst);
  return hipGetLastError();
}
hipError_t shk_pa_deriv_rev(const fp* top, fp* out, uint64_t N, uint64_t n, hipStream_t st) {
  hipLaunchKernelGGL(deriv_rev_kernel, grid_for(N), dim3(TPB), 0, st, top, out, N, n);
  return hipGetLastError();
}
hipError_t shk_pa_weights(const fp* ys, const fp* inv, fp* out, uint64_t n, uint64_t N, hipStream_t st) {
  hipLaunchKernelGGL(weights_kernel, grid_for(N), dim3(TPB), 0, st, ys, inv, out, n, N);
  return hipGetLastError();
}
hipError_t shk_pa_sub(const fp* a, const fp* b, fp* out, uint64_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(sub_kernel, grid_for(n), dim3(TPB), 0, st, a, b, out, n);
  return hipGetLastError();
}
