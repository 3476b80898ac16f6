// multi_inv.hip -- batch inversion (multi_inv, starks/poly_utils.py:301-320) and four-point interpolation (multi_interp_4,
// poly_utils.py:412-440) on the device, by the tiled product tree of inv_items.cuh.
//
// One workgroup of IV_LANES lanes per tile.  iv_up_kernel writes each tile's product to the next level; iv_down_kernel recomputes
// its tile's chunk products and tree, takes the inverse of the tile product from the level above (or, for the single top tile,
// inverts it with fp_inv: one per call) and walks the tree and the chunks down.  Workgroups never communicate inside a launch: the
// levels are ordered only by being separate launches on one stream.  The LDS tree is 2 * IV_LANES elements (16 KiB).
#include "internal.hpp"
#include "inv_items.cuh"

namespace {

constexpr uint32_t L = IV_LANES;

template <uint32_t C, class Src>
__device__ __forceinline__ void tile_up(const Src& s, uint64_t count, fp* t, IvChunk<C>& ch) {
  const uint32_t l = threadIdx.x;
  t[L + l] = iv_chunk_forward<L, C>(s, count, blockIdx.x, l, ch);
  __syncthreads();
#pragma unroll 1
  for (uint32_t h = L / 2; h >= 1; h /= 2) {
    if (l < h) iv_tree_up(t, h + l);
    __syncthreads();
  }
}

// level j -> level j + 1: the product of each tile
template <uint32_t C, class Src>
__global__ void __launch_bounds__(L) iv_up_kernel(Src s, uint64_t count, fp* next) {
  __shared__ fp t[2 * L];
  IvChunk<C> ch;
  tile_up<C>(s, count, t, ch);
  if (threadIdx.x == 0) fp_store(next + blockIdx.x, fp_canon(t[1]));
}

// tile_inv[tile] = the inverse of the tile's product (the level above, already inverted in place); nullptr: the single top tile,
// whose product is inverted here
template <uint32_t C, class Src>
__global__ void __launch_bounds__(L) iv_down_kernel(Src s, uint64_t count, const fp* tile_inv) {
  __shared__ fp t[2 * L];
  IvChunk<C> ch;
  tile_up<C>(s, count, t, ch);
  const uint32_t l = threadIdx.x;
  if (l == 0) t[1] = tile_inv ? fp_load(tile_inv + blockIdx.x) : fp_inv(t[1]);
  __syncthreads();
#pragma unroll 1
  for (uint32_t h = 1; h < L; h *= 2) {
    if (l < h) iv_tree_down(t, h + l);
    __syncthreads();
  }
  iv_chunk_backward<L, C>(s, count, blockIdx.x, l, ch, t[L + l]);
}

// the whole call: level 0 is `items` (count n), levels 1 .. in scratch (iv_levels(n, L * C).scratch elements); every level is tiled
// by the same T = L * C
template <uint32_t C, class Src>
hipError_t run(const Src& items, uint64_t n, fp* scratch, hipStream_t st) {
  const IvLevels v = iv_levels(n, (uint64_t)L * C);
  auto level = [&](uint32_t j) { return IvElems{scratch + v.off[j], scratch + v.off[j]}; };
  auto tiles = [&](uint32_t j) { return (unsigned)(v.count[j] / (L * C) + (v.count[j] % (L * C) ? 1 : 0)); };
  for (uint32_t j = 0; j + 1 < v.depth; ++j) {
    if (j == 0) hipLaunchKernelGGL((iv_up_kernel<C, Src>), dim3(tiles(0)), dim3(L), 0, st, items, v.count[0], scratch + v.off[1]);
    else hipLaunchKernelGGL((iv_up_kernel<C, IvElems>), dim3(tiles(j)), dim3(L), 0, st, level(j), v.count[j], scratch + v.off[j + 1]);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  for (int j = (int)v.depth - 1; j >= 0; --j) {
    const fp* above = j + 1 < (int)v.depth ? scratch + v.off[j + 1] : nullptr;
    if (j == 0) hipLaunchKernelGGL((iv_down_kernel<C, Src>), dim3(tiles(0)), dim3(L), 0, st, items, v.count[0], above);
    else hipLaunchKernelGGL((iv_down_kernel<C, IvElems>), dim3(tiles(j)), dim3(L), 0, st, level(j), v.count[j], above);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

uint64_t shk_multi_inv_scratch(uint64_t n) { return iv_levels(n, (uint64_t)L * IV_CHUNK).scratch; }
uint64_t shk_multi_interp_4_scratch(uint64_t rows) { return iv_levels(rows, (uint64_t)L * IV_ROW_CHUNK).scratch; }

hipError_t shk_multi_inv(const fp* in, fp* out, uint64_t n, fp* scratch, hipStream_t st) {
  return run<IV_CHUNK>(IvElems{in, out}, n, scratch, st);
}

hipError_t shk_multi_interp_4(const fp* xs, const fp* ys, fp* coeffs, uint64_t rows, fp* scratch, hipStream_t st) {
  return run<IV_ROW_CHUNK>(IvRows{xs, ys, coeffs}, rows, scratch, st);
}
