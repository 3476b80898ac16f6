// mod64fri.hip -- the kernels of the FRI commit over any odd modulus below 2^64 on packed 64-bit words (sh_mod64_fri_prove;
// mod64fri_items.cuh has the per-item bodies, api_mod64fri.hip drives them).  The modulus block is a kernel argument of every launch
// that does field arithmetic.  The levels above the leaf kernels, and the index sampler, are the MiMC path's own kernels (kernels.hip):
// nothing there depends on p or on the width of a value.
#include "internal.hpp"
#include "mod64fri_items.cuh"

namespace {

constexpr uint64_t GX = 1ull << 22;
inline dim3 grid_for_blocks(uint64_t blocks) {
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t block_id() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }

// one thread per permute4 row: four 8-byte loads, four leaves and the three nodes above them.  WIDE = the launch fills the chip several
// times over: the hashes use the asm rounds (blake2s.cuh), as in mf_leaves_kernel
template <bool WIDE>
__global__ void __launch_bounds__(MF_WG) m6_leaves_kernel(M6Tree t, uint64_t per_tree) {
  const uint64_t blk = block_id(), b = blk / per_tree, i = (blk - b * per_tree) * MF_WG + threadIdx.x;
  if (b < t.batch && i < (t.n >> 2)) m6_leaves_item<WIDE>(t, b, i);
}

__global__ void __launch_bounds__(MF_WG) m6_fold_kernel(M6Fold a, f64_mod M) {
  const uint64_t g = block_id() * MF_WG + threadIdx.x;
  if (g < (a.n >> 2) * a.batch) m6_fold_item(a, M, g);
}

__global__ void __launch_bounds__(MF_WG) m6_gather_kernel(M6Gather a) {
  const uint64_t g = block_id() * MF_WG + threadIdx.x;
  if (g < a.work_total + a.final_n * a.batch) m6_gather_item(a, g);
}

constexpr uint64_t M6_WIDE_THREADS = 1ull << 19;  // MF_WIDE_THREADS of modfri.hip: the same launch rule

}  // namespace

hipError_t shk_m6_leaves(const M6Tree& t, hipStream_t st) {
  if (t.n < 4 || (t.n & (t.n - 1)) || t.batch == 0) return hipErrorInvalidValue;
  const uint64_t per_tree = ((t.n >> 2) + MF_WG - 1) / MF_WG;
  if ((t.n >> 2) * t.batch >= M6_WIDE_THREADS)
    hipLaunchKernelGGL(m6_leaves_kernel<true>, grid_for_blocks(per_tree * t.batch), dim3(MF_WG), 0, st, t, per_tree);
  else
    hipLaunchKernelGGL(m6_leaves_kernel<false>, grid_for_blocks(per_tree * t.batch), dim3(MF_WG), 0, st, t, per_tree);
  return hipGetLastError();
}

hipError_t shk_m6_fold(const M6Fold& a, const f64_mod& M, hipStream_t st) {
  const uint64_t work = (a.n >> 2) * a.batch;
  if (!work) return hipSuccess;
  hipLaunchKernelGGL(m6_fold_kernel, grid_for_blocks((work + MF_WG - 1) / MF_WG), dim3(MF_WG), 0, st, a, M);
  return hipGetLastError();
}

hipError_t shk_m6_gather(const M6Gather& a, hipStream_t st) {
  const uint64_t work = a.work_total + a.final_n * a.batch;
  if (!work) return hipSuccess;
  hipLaunchKernelGGL(m6_gather_kernel, grid_for_blocks((work + MF_WG - 1) / MF_WG), dim3(MF_WG), 0, st, a);
  return hipGetLastError();
}
