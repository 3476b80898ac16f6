// modfri.hip -- the kernels of the FRI commit over any odd modulus below 2^256 (sh_mod_fri_prove; modfri_items.cuh has the per-item
// bodies, api_modfri.hip drives them).  The modulus block is a kernel argument of every launch that does field arithmetic.  The
// levels above the leaf kernels, and the index sampler, are the MiMC path's own kernels (kernels.hip): nothing there depends on p.
#include "internal.hpp"
#include "modfri_items.cuh"

static_assert(MF_MAX_ROUNDS == SHK_FRI_MAX_ROUNDS, "the gather holds as many rounds as the sampler");

namespace {

constexpr uint64_t GX = 1ull << 22;
inline dim3 grid_for_blocks(uint64_t blocks) {
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t block_id() { return (uint64_t)blockIdx.y * gridDim.x + blockIdx.x; }
// launches over `rows` rows of each of `batch` trees: a workgroup stays inside one tree
inline uint64_t row_blocks(uint64_t rows) { return (rows + MF_WG - 1) / MF_WG; }

// one thread per permute4 row: four leaves and the three nodes above them.  WIDE = the launch fills the chip several times over:
// the hashes use the asm rounds (blake2s.cuh), as in merkle_leaves_kernel
template <bool WIDE>
__global__ void __launch_bounds__(MF_WG) mf_leaves_kernel(MfTree t, uint64_t per_tree) {
  const uint64_t blk = block_id(), b = blk / per_tree, i = (blk - b * per_tree) * MF_WG + threadIdx.x;
  if (b < t.batch && i < (t.n >> 2)) mf_leaves_item<WIDE>(t, b, i);
}

__global__ void __launch_bounds__(MF_WG) mf_fold_kernel(MfFold a, fpm_mod M) {
  const uint64_t g = block_id() * MF_WG + threadIdx.x;
  if (g < (a.n >> 2) * a.batch) mf_fold_item(a, M, g);
}

__global__ void __launch_bounds__(MF_WG) mf_gather_kernel(MfGather a) {
  const uint64_t g = block_id() * MF_WG + threadIdx.x;
  if (g < a.work_total + a.final_n * a.batch) mf_gather_item(a, g);
}

constexpr uint64_t MF_WIDE_THREADS = 1ull << 19;  // MERKLE_WIDE_THREADS of kernels.hip

}  // namespace

hipError_t shk_mf_leaves(const MfTree& t, hipStream_t st) {
  if (t.n < 4 || (t.n & (t.n - 1)) || t.batch == 0) return hipErrorInvalidValue;
  const uint64_t per_tree = row_blocks(t.n >> 2);
  if ((t.n >> 2) * t.batch >= MF_WIDE_THREADS)
    hipLaunchKernelGGL(mf_leaves_kernel<true>, grid_for_blocks(per_tree * t.batch), dim3(MF_WG), 0, st, t, per_tree);
  else
    hipLaunchKernelGGL(mf_leaves_kernel<false>, grid_for_blocks(per_tree * t.batch), dim3(MF_WG), 0, st, t, per_tree);
  return hipGetLastError();
}

hipError_t shk_mf_fold(const MfFold& a, const fpm_mod& M, hipStream_t st) {
  const uint64_t work = (a.n >> 2) * a.batch;
  if (!work) return hipSuccess;
  hipLaunchKernelGGL(mf_fold_kernel, grid_for_blocks((work + MF_WG - 1) / MF_WG), dim3(MF_WG), 0, st, a, M);
  return hipGetLastError();
}

hipError_t shk_mf_gather(const MfGather& a, hipStream_t st) {
  const uint64_t work = a.work_total + a.final_n * a.batch;
  if (!work) return hipSuccess;
  hipLaunchKernelGGL(mf_gather_kernel, grid_for_blocks((work + MF_WG - 1) / MF_WG), dim3(MF_WG), 0, st, a);
  return hipGetLastError();
}
