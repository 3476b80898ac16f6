// mod64stark.hip -- the kernels of the STARK prover's middle over any prime modulus below 2^64 on packed 64-bit words
// (sh_mod64_stark_prove; mod64stark_items.cuh has the per-item bodies, api_mod64stark.hip drives them).  The modulus block is a kernel
// argument of every launch that does field arithmetic.  One form per kernel: one thread per work item, the lanes of a wave on consecutive
// items, so that every array access of an item is an 8-byte word per lane at consecutive addresses.  The transforms are ntt64.hip's, the
// trees of plain words and the commit rounds mod64fri.hip's, the tree levels above the leaf kernels and the index sampler the MiMC
// path's (kernels.hip).
#include "internal.hpp"
#include "mod64stark_items.cuh"

static_assert(M6S_MAX_WIDTH == SHK_STARK_MAX_WIDTH && M6S_MAX_TERMS == SHK_STARK_MAX_TERMS, "the packed prover takes the MiMC prover's shapes");

namespace {

// one thread per item, M6S_WG per workgroup, a one-dimensional grid: the field kernels see at most batch * width * n <= 2^28 items
// (mod64_prepare's limit), the gather 32-byte slots of proofs that fit a buffer
constexpr uint64_t M6S_MAX_BLOCKS = 0x7fffffffull;
inline dim3 grid_for_items(uint64_t items) { return dim3((unsigned)((items + M6S_WG - 1) / M6S_WG)); }
__device__ __forceinline__ uint64_t item_id() { return (uint64_t)blockIdx.x * M6S_WG + threadIdx.x; }

__global__ void __launch_bounds__(M6S_WG) m6s_batch_inv_kernel(M6sInv a, f64_mod M) {
  const uint64_t g = item_id();
  if (g < a.chunks) m6s_batch_inv_item(a, M, g);
}
__global__ void __launch_bounds__(M6S_WG) m6s_den_kernel(M6sTables t, f64_mod M) {
  const uint64_t i = item_id();
  if (i < t.n) m6s_den_item(t, M, i);
}
__global__ void __launch_bounds__(M6S_WG) m6s_tables_kernel(M6sTables t, f64_mod M) {
  const uint64_t i = item_id();
  if (i < t.n) m6s_tables_item(t, M, i);
}
__global__ void __launch_bounds__(M6S_WG) m6s_interp_kernel(M6sArgs a, f64_mod M) {
  const uint64_t col = item_id();
  if (col < (uint64_t)a.batch * a.width) m6s_interp_item(a, M, col);
}
__global__ void __launch_bounds__(M6S_WG) m6s_qprep_kernel(const uint64_t* pcoef, uint64_t* q, uint64_t steps, uint64_t total, f64_mod M) {
  const uint64_t g = item_id();
  if (g < total) m6s_qprep_item(pcoef, q, steps, g, M);
}
template <int W>
__global__ void __launch_bounds__(M6S_WG) m6s_trace_kernel(M6sArgs a, f64_mod M) {
  const uint64_t g = item_id();
  if (g < a.steps * a.batch) m6s_trace_item<W>(a, M, g);
}
template <int W>
__global__ void __launch_bounds__(M6S_WG) m6s_quot_kernel(M6sArgs a, f64_mod M) {
  const uint64_t g = item_id();
  if (g < a.n * a.batch) m6s_quot_item<W>(a, M, g / a.n, g & (a.n - 1));
}
// the C++ hash rounds, as the 256-bit path's packed-leaf kernel runs them
__global__ void __launch_bounds__(M6S_WG) m6s_leaf_rows_kernel(M6sArgs a, uint32_t* nodes) {
  const uint64_t g = item_id(), q = a.n >> 2;
  if (g < q * a.batch) m6s_leaf_row_item<false>(a, nodes, g / q, g & (q - 1));
}
__global__ void __launch_bounds__(64) m6s_scalars_kernel(const uint32_t* mnodes, uint64_t tree_words, uint32_t width, uint32_t batch,
                                                         uint64_t cpow, uint64_t* scal, f64_mod M) {
  const uint64_t b = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (b < batch) m6s_scalars_item(mnodes, tree_words, width, cpow, scal, b, M);
}
__global__ void __launch_bounds__(M6S_WG) m6s_lincomb_kernel(M6sArgs a, const uint64_t* scal, uint64_t* l, f64_mod M) {
  const uint64_t g = item_id();
  if (g < a.n * a.batch) m6s_lincomb_item(a, scal, l, M, g / a.n, g & (a.n - 1));
}
__global__ void __launch_bounds__(M6S_WG) m6s_gather_kernel(M6sArgs a, M6sGather ga) {
  const uint64_t g = item_id();
  if (g < m6s_gather_per_proof(a.width, ga.samples, ga.lg) * a.batch) m6s_gather_item(a, ga, g);
}

}  // namespace

hipError_t shk_m6s_tables(const M6sTables& t, const f64_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(m6s_den_kernel, grid_for_items(t.n), dim3(M6S_WG), 0, st, t, M);
  M6sInv inv;
  inv.in = t.den;
  inv.out = t.table;
  inv.count = 2 * t.n;
  inv.chunks = (inv.count + M6S_INV_CHUNK - 1) / M6S_INV_CHUNK;
  hipLaunchKernelGGL(m6s_batch_inv_kernel, grid_for_items(inv.chunks), dim3(M6S_WG), 0, st, inv, M);
  hipLaunchKernelGGL(m6s_tables_kernel, grid_for_items(t.n), dim3(M6S_WG), 0, st, t, M);
  return hipGetLastError();
}

hipError_t shk_m6s_interp(const M6sArgs& a, const f64_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(m6s_interp_kernel, grid_for_items((uint64_t)a.batch * a.width), dim3(M6S_WG), 0, st, a, M);
  return hipGetLastError();
}

hipError_t shk_m6s_qprep(const uint64_t* pcoef, uint64_t* q, uint64_t steps, uint64_t cols, const f64_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(m6s_qprep_kernel, grid_for_items(cols * steps), dim3(M6S_WG), 0, st, pcoef, q, steps, cols * steps, M);
  return hipGetLastError();
}

// D and B on the whole domain, then the packed-leaf tree over (P, D, B)
hipError_t shk_m6s_quotients_and_merkelize(const M6sArgs& a, const f64_mod& M, uint32_t* d_nodes, hipStream_t st) {
  if (a.n < 4) return hipErrorInvalidValue;
  const dim3 tgrid = grid_for_items(a.steps * a.batch), qgrid = grid_for_items(a.n * a.batch), block(M6S_WG);
  switch (a.width) {
#define SHK_CASE(W)                                                     \
  case W:                                                               \
    hipLaunchKernelGGL(m6s_trace_kernel<W>, tgrid, block, 0, st, a, M); \
    hipLaunchKernelGGL(m6s_quot_kernel<W>, qgrid, block, 0, st, a, M);  \
    break;
    SHK_CASE(1) SHK_CASE(2) SHK_CASE(3) SHK_CASE(4) SHK_CASE(5) SHK_CASE(6) SHK_CASE(7) SHK_CASE(8) SHK_CASE(9)
#undef SHK_CASE
    default: return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(m6s_leaf_rows_kernel, grid_for_items((a.n >> 2) * a.batch), block, 0, st, a, d_nodes);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return shk_merkle_upper_levels(a.n, a.batch, d_nodes, st);
}

hipError_t shk_m6s_scalars(const uint32_t* d_mnodes, uint64_t tree_words, uint32_t width, uint32_t batch, uint64_t cpow, uint64_t* d_scal,
                           const f64_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(m6s_scalars_kernel, dim3((batch + 63) / 64), dim3(64), 0, st, d_mnodes, tree_words, width, batch, cpow, d_scal, M);
  return hipGetLastError();
}

hipError_t shk_m6s_lincomb(const M6sArgs& a, const uint64_t* d_scal, uint64_t* d_l, const f64_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(m6s_lincomb_kernel, grid_for_items(a.n * a.batch), dim3(M6S_WG), 0, st, a, d_scal, d_l, M);
  return hipGetLastError();
}

hipError_t shk_m6s_gather(const M6sArgs& a, const M6sGather& ga, hipStream_t st) {
  const uint64_t items = m6s_gather_per_proof(a.width, ga.samples, ga.lg) * a.batch;
  if ((items + M6S_WG - 1) / M6S_WG > M6S_MAX_BLOCKS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(m6s_gather_kernel, grid_for_items(items), dim3(M6S_WG), 0, st, a, ga);
  return hipGetLastError();
}
