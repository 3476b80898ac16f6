// modpoly.hip -- the kernels of polynomial arithmetic and batch inversion over any prime modulus below 2^256 (modpoly_items.cuh has the
// element steps, poly_items.cuh the drivers, api_modpoly.hip the host side).  The per-element kernels are one thread per output and
// memory-bound next to the transforms between them; the batch inversion is multi_inv.hip's tiled product tree over fpm, one workgroup
// per tile, the levels ordered by being separate launches on one stream.  The modulus block is a kernel argument of every launch.
#include "internal.hpp"
#include "modpoly_items.cuh"

namespace {

constexpr int TPB = 256;
constexpr uint32_t L = MP_IV_LANES;

inline dim3 grid_for(uint64_t work) {
  const uint64_t blocks = (work + TPB - 1) / TPB;
  constexpr uint64_t GX = 1ull << 22;
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t tid() { return ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * TPB + threadIdx.x; }

__global__ void __launch_bounds__(TPB) mp_copy_kernel(PaCopy c, const fpm* src, fpm* dst, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= c.rows * c.len) return;
  const uint64_t r = g / c.len, k = g - r * c.len;
  mn_st(dst + r * c.ds + k, mp_copy_item(c, src, r, k, M));
}

// the byte swap between 32-byte big-endian wire values and limbs (its own inverse); nothing is reduced
__global__ void __launch_bounds__(TPB) mp_swap_kernel(const fpm* src, fpm* dst, uint64_t n) {
  const uint64_t g = tid();
  if (g >= n) return;
  const fpm v = mn_ld(src + g);
  mn_st(dst + g, fpm_from_wire_words(v.v));
}

// out rows j < nodes/2 of 2d = 2^log2d: the parent of transformed rows 2j, 2j + 1
__global__ void __launch_bounds__(TPB) mp_tree_kernel(const fpm* hz, fpm* oz, const fpm* hn, fpm* on, uint32_t log2d, uint64_t total,
                                                      fpm_mod M) {
  const uint64_t g = tid();
  if (g >= total) return;
  const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1);
  const uint64_t a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
  const fpm A = mn_ld(hz + a), B = mn_ld(hz + b);
  if (oz) mn_st(oz + g, mp_tree_node(A, B, i, M));
  if (on) mn_st(on + g, mp_num_node(mn_ld(hn + a), mn_ld(hn + b), A, B, i, M));
}

// children c = 2j, 2j + 1 at index i: hr[c] <- hd[j] * hr[c ^ 1]  (one thread per sibling pair)
__global__ void __launch_bounds__(TPB) mp_mid_kernel(const fpm* hd, fpm* hr, uint32_t log2d, uint64_t pairs_total, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= pairs_total) return;
  const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1);
  const uint64_t a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
  fpm oa, ob;
  mp_mid(mn_ld(hd + g), mn_ld(hr + a), mn_ld(hr + b), &oa, &ob, M);
  mn_st(hr + a, oa);
  mn_st(hr + b, ob);
}

__global__ void __launch_bounds__(TPB) mp_newton_kernel(const fpm* F, fpm* G, uint64_t n, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= n) return;
  mn_st(G + g, mp_newton(mn_ld(F + g), mn_ld(G + g), M));
}

__global__ void __launch_bounds__(64) mp_inv1_kernel(const fpm* src, fpm* dst, fpm pm2, fpm_mod M) {
  if (threadIdx.x == 0) mn_st(dst, mp_inv1(mn_ld(src), pm2, M));
}

__global__ void __launch_bounds__(TPB) mp_deriv_rev_kernel(const fpm* top, fpm* out, uint64_t N, uint64_t n, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= N) return;
  mn_st(out + g, mp_deriv_rev(top, N, n, g, M));
}

__global__ void __launch_bounds__(TPB) mp_weights_kernel(const fpm* ys, const fpm* inv, fpm* out, uint64_t n, uint64_t N, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= N) return;
  mn_st(out + g, g < n ? mp_weight(mn_ld(ys + g), mn_ld(inv + g), M) : fpm_zero());
}

__global__ void __launch_bounds__(TPB) mp_sub_kernel(const fpm* a, const fpm* b, fpm* out, uint64_t n, fpm_mod M) {
  const uint64_t g = tid();
  if (g >= n) return;
  mn_st(out + g, mp_sub(mn_ld(a + g), mn_ld(b + g), M));
}

// ---- the batch inversion ---------------------------------------------------------------------------------------------------------------
template <uint32_t C, class Src>
__device__ __forceinline__ void tile_up(const Src& s, const fpm_mod& M, uint64_t count, fpm* t, MpChunk<C>& ch) {
  const uint32_t l = threadIdx.x;
  t[L + l] = mp_chunk_forward<L, C>(s, M, count, blockIdx.x, l, ch);
  __syncthreads();
#pragma unroll 1
  for (uint32_t h = L / 2; h >= 1; h /= 2) {
    if (l < h) mp_tree_up(t, h + l, M);
    __syncthreads();
  }
}

// level j -> level j + 1: the product of each tile, Montgomery form
template <uint32_t C, class Src>
__global__ void __launch_bounds__(L) mp_iv_up_kernel(Src s, uint64_t count, fpm* next, fpm_mod M) {
  __shared__ fpm t[2 * L];
  MpChunk<C> ch;
  tile_up<C>(s, M, count, t, ch);
  if (threadIdx.x == 0) mn_st(next + blockIdx.x, t[1]);
}

// tile_inv[tile] = the inverse of the tile's product (the level above, already inverted in place); nullptr: the single top tile, whose
// product is inverted here by the call's one p - 2 power
template <uint32_t C, class Src>
__global__ void __launch_bounds__(L) mp_iv_down_kernel(Src s, uint64_t count, const fpm* tile_inv, fpm pm2, fpm_mod M) {
  __shared__ fpm t[2 * L];
  MpChunk<C> ch;
  tile_up<C>(s, M, count, t, ch);
  const uint32_t l = threadIdx.x;
  if (l == 0) t[1] = tile_inv ? mn_ld(tile_inv + blockIdx.x) : mp_top_inv(t[1], pm2, M);
  __syncthreads();
#pragma unroll 1
  for (uint32_t h = 1; h < L; h *= 2) {
    if (l < h) mp_tree_down(t, h + l, M);
    __syncthreads();
  }
  mp_chunk_backward<L, C>(s, M, count, blockIdx.x, l, ch, t[L + l]);
}

template <uint32_t C, class Src>
hipError_t run(const Src& items, uint64_t n, fpm* scratch, const fpm_mod& M, hipStream_t st) {
  const IvLevels v = mp_iv_levels<L, C>(n);
  const fpm pm2 = ms_pm2(M);
  auto level = [&](uint32_t j) { return MpMont{scratch + v.off[j]}; };
  auto tiles = [&](uint32_t j) { return (unsigned)(v.count[j] / (L * C) + (v.count[j] % (L * C) ? 1 : 0)); };
  for (uint32_t j = 0; j + 1 < v.depth; ++j) {
    if (j == 0) hipLaunchKernelGGL((mp_iv_up_kernel<C, Src>), dim3(tiles(0)), dim3(L), 0, st, items, v.count[0], scratch + v.off[1], M);
    else hipLaunchKernelGGL((mp_iv_up_kernel<C, MpMont>), dim3(tiles(j)), dim3(L), 0, st, level(j), v.count[j], scratch + v.off[j + 1], M);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  for (int j = (int)v.depth - 1; j >= 0; --j) {
    const fpm* above = j + 1 < (int)v.depth ? scratch + v.off[j + 1] : nullptr;
    if (j == 0) hipLaunchKernelGGL((mp_iv_down_kernel<C, Src>), dim3(tiles(0)), dim3(L), 0, st, items, v.count[0], above, pm2, M);
    else hipLaunchKernelGGL((mp_iv_down_kernel<C, MpMont>), dim3(tiles(j)), dim3(L), 0, st, level(j), v.count[j], above, pm2, M);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace

#define MP_LAUNCH(kernel, work, ...)                                              \
  do {                                                                            \
    hipLaunchKernelGGL(kernel, grid_for(work), dim3(TPB), 0, st, __VA_ARGS__);    \
    return hipGetLastError();                                                     \
  } while (0)

hipError_t shk_mp_copy(const PaCopy& c, const fpm* src, fpm* dst, const fpm_mod& M, hipStream_t st) {
  if (!c.rows || !c.len) return hipSuccess;
  MP_LAUNCH(mp_copy_kernel, c.rows * c.len, c, src, dst, M);
}
hipError_t shk_mp_swap(const void* src, void* dst, uint64_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  MP_LAUNCH(mp_swap_kernel, n, static_cast<const fpm*>(src), static_cast<fpm*>(dst), n);
}
hipError_t shk_mp_tree(const fpm* hz, fpm* oz, const fpm* hn, fpm* on, uint32_t log2d, uint64_t nodes, const fpm_mod& M, hipStream_t st) {
  const uint64_t total = (nodes / 2) << log2d;
  if (!total) return hipSuccess;
  MP_LAUNCH(mp_tree_kernel, total, hz, oz, hn, on, log2d, total, M);
}
hipError_t shk_mp_mid(const fpm* hd, fpm* hr, uint32_t log2d, uint64_t children, const fpm_mod& M, hipStream_t st) {
  const uint64_t total = (children / 2) << log2d;
  if (!total) return hipSuccess;
  MP_LAUNCH(mp_mid_kernel, total, hd, hr, log2d, total, M);
}
hipError_t shk_mp_newton(const fpm* F, fpm* G, uint64_t n, const fpm_mod& M, hipStream_t st) {
  if (!n) return hipSuccess;
  MP_LAUNCH(mp_newton_kernel, n, F, G, n, M);
}
hipError_t shk_mp_inv1(const fpm* src, fpm* dst, const fpm_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(mp_inv1_kernel, dim3(1), dim3(64), 0, st, src, dst, ms_pm2(M), M);
  return hipGetLastError();
}
hipError_t shk_mp_deriv_rev(const fpm* top, fpm* out, uint64_t N, uint64_t n, const fpm_mod& M, hipStream_t st) {
  if (!N) return hipSuccess;
  MP_LAUNCH(mp_deriv_rev_kernel, N, top, out, N, n, M);
}
hipError_t shk_mp_weights(const fpm* ys, const fpm* inv, fpm* out, uint64_t n, uint64_t N, const fpm_mod& M, hipStream_t st) {
  if (!N) return hipSuccess;
  MP_LAUNCH(mp_weights_kernel, N, ys, inv, out, n, N, M);
}
hipError_t shk_mp_sub(const fpm* a, const fpm* b, fpm* out, uint64_t n, const fpm_mod& M, hipStream_t st) {
  if (!n) return hipSuccess;
  MP_LAUNCH(mp_sub_kernel, n, a, b, out, n, M);
}

uint64_t shk_mp_multi_inv_scratch(uint64_t n) { return mp_iv_levels<L, MP_IV_CHUNK>(n).scratch; }
uint64_t shk_mp_multi_interp_4_scratch(uint64_t rows) { return mp_iv_levels<L, MP_IV_ROW_CHUNK>(rows).scratch; }
hipError_t shk_mp_multi_inv(const fpm* in, fpm* out, uint64_t n, fpm* scratch, const fpm_mod& M, hipStream_t st) {
  return run<MP_IV_CHUNK>(MpElems{in, out}, n, scratch, M, st);
}
hipError_t shk_mp_multi_interp_4(const fpm* xs, const fpm* ys, fpm* coeffs, uint64_t rows, fpm* scratch, const fpm_mod& M, hipStream_t st) {
  return run<MP_IV_ROW_CHUNK>(MpRows{xs, ys, coeffs}, rows, scratch, M, st);
}
