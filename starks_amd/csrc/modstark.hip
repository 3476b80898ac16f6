// modstark.hip -- the kernels of the STARK prover's middle over any prime modulus below 2^256 (sh_mod_stark_prove; modstark_items.cuh
// has the per-item bodies and the derivation, api_modstark.hip drives them).  The modulus block is a kernel argument of every launch
// that does field arithmetic.  One form per kernel: one thread per work item.  The transforms are modntt.hip's, the trees of plain
// values and the commit rounds modfri.hip's, the tree levels above the leaf kernels and the index sampler the MiMC path's (kernels.hip).
#include "internal.hpp"
#include "modstark_items.cuh"

static_assert(MS_MAX_WIDTH == SHK_STARK_MAX_WIDTH && MS_MAX_TERMS == SHK_STARK_MAX_TERMS, "the generic prover takes the MiMC prover's shapes");

namespace {

// one thread per item, MS_WG per workgroup, a one-dimensional grid: the field kernels see at most batch * width * n <= 2^26 items
// (mod_prepare's limit), the gather 32-byte slots of proofs that fit a buffer
constexpr uint64_t MS_MAX_BLOCKS = 0x7fffffffull;
inline dim3 grid_for_items(uint64_t items) { return dim3((unsigned)((items + MS_WG - 1) / MS_WG)); }
__device__ __forceinline__ uint64_t item_id() { return (uint64_t)blockIdx.x * MS_WG + threadIdx.x; }

__global__ void __launch_bounds__(MS_WG) ms_batch_inv_kernel(MsInv a, fpm_mod M) {
  const uint64_t g = item_id();
  if (g < a.chunks) ms_batch_inv_item(a, M, g);
}
__global__ void __launch_bounds__(MS_WG) ms_den_kernel(MsTables t, fpm_mod M) {
  const uint64_t i = item_id();
  if (i < t.n) ms_den_item(t, M, i);
}
__global__ void __launch_bounds__(MS_WG) ms_tables_kernel(MsTables t, fpm_mod M) {
  const uint64_t i = item_id();
  if (i < t.n) ms_tables_item(t, M, i);
}
__global__ void __launch_bounds__(MS_WG) ms_interp_kernel(MsArgs a, fpm_mod M) {
  const uint64_t col = item_id();
  if (col < (uint64_t)a.batch * a.width) ms_interp_item(a, M, col);
}
__global__ void __launch_bounds__(MS_WG) ms_qprep_kernel(const fpm* pcoef, fpm* q, uint64_t steps, uint64_t total, fpm_mod M) {
  const uint64_t g = item_id();
  if (g < total) ms_qprep_item(pcoef, q, steps, g, M);
}
template <int W>
__global__ void __launch_bounds__(MS_WG) ms_trace_kernel(MsArgs a, fpm_mod M) {
  const uint64_t g = item_id();
  if (g < a.steps * a.batch) ms_trace_item<W>(a, M, g);
}
template <int W>
__global__ void __launch_bounds__(MS_WG) ms_quot_kernel(MsArgs a, fpm_mod M) {
  const uint64_t g = item_id();
  if (g < a.n * a.batch) ms_quot_item<W>(a, M, g / a.n, g & (a.n - 1));
}
// the hash rounds of the packed-leaf kernel: the C++ rounds unless built with -DSHK_MS_LEAF_ASM_ROUNDS=1 (blake2s.cuh's throughput form);
// one form per build, chosen by the A/B in profiles/r15_mod_stark_leaf_rounds_ab.txt
#ifndef SHK_MS_LEAF_ASM_ROUNDS
#define SHK_MS_LEAF_ASM_ROUNDS 0
#endif
__global__ void __launch_bounds__(MS_WG) ms_leaf_rows_kernel(MsArgs a, uint32_t* nodes) {
  const uint64_t g = item_id(), q = a.n >> 2;
  if (g < q * a.batch) ms_leaf_row_item<SHK_MS_LEAF_ASM_ROUNDS != 0>(a, nodes, g / q, g & (q - 1));
}
__global__ void __launch_bounds__(64) ms_scalars_kernel(const uint32_t* mnodes, uint64_t tree_words, uint32_t width, uint32_t batch, fpm cpow,
                                                        fpm* scal, fpm_mod M) {
  const uint64_t b = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (b < batch) ms_scalars_item(mnodes, tree_words, width, cpow, scal, b, M);
}
__global__ void __launch_bounds__(MS_WG) ms_lincomb_kernel(MsArgs a, const fpm* scal, fpm* l, fpm_mod M) {
  const uint64_t g = item_id();
  if (g < a.n * a.batch) ms_lincomb_item(a, scal, l, M, g / a.n, g & (a.n - 1));
}
__global__ void __launch_bounds__(MS_WG) ms_gather_kernel(MsArgs a, MsGather ga) {
  const uint64_t g = item_id();
  if (g < ms_gather_per_proof(a.width, ga.samples, ga.lg) * a.batch) ms_gather_item(a, ga, g);
}

}  // namespace

hipError_t shk_ms_batch_inv(const MsInv& a, const fpm_mod& M, hipStream_t st) {
  if (!a.chunks) return hipSuccess;
  hipLaunchKernelGGL(ms_batch_inv_kernel, grid_for_items(a.chunks), dim3(MS_WG), 0, st, a, M);
  return hipGetLastError();
}

hipError_t shk_ms_tables(const MsTables& t, const fpm& pm2, const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(ms_den_kernel, grid_for_items(t.n), dim3(MS_WG), 0, st, t, M);
  MsInv inv;
  inv.in = t.den;
  inv.out = t.table;
  inv.count = 2 * t.n;
  inv.chunks = (inv.count + MS_INV_CHUNK - 1) / MS_INV_CHUNK;
  inv.pm2 = pm2;
  hipLaunchKernelGGL(ms_batch_inv_kernel, grid_for_items(inv.chunks), dim3(MS_WG), 0, st, inv, M);
  hipLaunchKernelGGL(ms_tables_kernel, grid_for_items(t.n), dim3(MS_WG), 0, st, t, M);
  return hipGetLastError();
}

hipError_t shk_ms_interp(const MsArgs& a, const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(ms_interp_kernel, grid_for_items((uint64_t)a.batch * a.width), dim3(MS_WG), 0, st, a, M);
  return hipGetLastError();
}

hipError_t shk_ms_qprep(const fpm* pcoef, fpm* q, uint64_t steps, uint64_t cols, const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(ms_qprep_kernel, grid_for_items(cols * steps), dim3(MS_WG), 0, st, pcoef, q, steps, cols * steps, M);
  return hipGetLastError();
}

// D and B on the whole domain, then the packed-leaf tree over (P, D, B)
hipError_t shk_ms_quotients_and_merkelize(const MsArgs& a, const fpm_mod& M, uint32_t* d_nodes, hipStream_t st) {
  if (a.n < 4) return hipErrorInvalidValue;
  const dim3 tgrid = grid_for_items(a.steps * a.batch), qgrid = grid_for_items(a.n * a.batch), block(MS_WG);
  switch (a.width) {
#define SHK_CASE(W)                                                     \
  case W:                                                               \
    hipLaunchKernelGGL(ms_trace_kernel<W>, tgrid, block, 0, st, a, M);  \
    hipLaunchKernelGGL(ms_quot_kernel<W>, qgrid, block, 0, st, a, M);   \
    break;
    SHK_CASE(1) SHK_CASE(2) SHK_CASE(3) SHK_CASE(4) SHK_CASE(5) SHK_CASE(6) SHK_CASE(7) SHK_CASE(8) SHK_CASE(9)
#undef SHK_CASE
    default: return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(ms_leaf_rows_kernel, grid_for_items((a.n >> 2) * a.batch), block, 0, st, a, d_nodes);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return shk_merkle_upper_levels(a.n, a.batch, d_nodes, st);
}

hipError_t shk_ms_scalars(const uint32_t* d_mnodes, uint64_t tree_words, uint32_t width, uint32_t batch, const fpm& cpow, fpm* d_scal,
                          const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(ms_scalars_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, d_mnodes, tree_words, width, batch, cpow, d_scal, M);
  return hipGetLastError();
}

hipError_t shk_ms_lincomb(const MsArgs& a, const fpm* d_scal, fpm* d_l, const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(ms_lincomb_kernel, grid_for_items(a.n * a.batch), dim3(MS_WG), 0, st, a, d_scal, d_l, M);
  return hipGetLastError();
}

hipError_t shk_ms_gather(const MsArgs& a, const MsGather& ga, hipStream_t st) {
  if ((ms_gather_per_proof(a.width, ga.samples, ga.lg) * a.batch + MS_WG - 1) / MS_WG > MS_MAX_BLOCKS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ms_gather_kernel, grid_for_items(ms_gather_per_proof(a.width, ga.samples, ga.lg) * a.batch), dim3(MS_WG), 0, st, a, ga);
  return hipGetLastError();
}
