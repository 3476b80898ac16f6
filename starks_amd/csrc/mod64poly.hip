// mod64poly.hip -- the kernels of polynomial arithmetic and batch inversion over any prime modulus below 2^64 on packed 64-bit words
// (mod64poly_items.cuh has the element steps, poly_items.cuh the drivers, api_mod64poly.hip the host side).  The modulus block is a
// kernel argument of every launch: no __constant__, no global.
//
// The per-element kernels move 8 bytes per element and are memory-bound.  tree, mid, newton and sub give every lane two consecutive
// words: when every array of the launch starts on a 16-byte boundary (the host decides, per launch) the pair moves as one 16-byte
// access, else as two words; an odd last word is handled by the pair's first half alone.  The grids are modpoly.hip's: one thread per
// pair (there: per element), 256 lanes, the block count folded into two grid dimensions above 2^22.  copy gathers by stride and
// direction, deriv_rev and weights read shifted sources: one word per lane.
//
// The batch inversion is multi_inv.hip's tiled product tree, one workgroup of 256 lanes per tile, the tile's tree 2 x 256 words of LDS,
// the levels ordered by being separate launches on one stream.
//
// Compiler figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; not measurements).  Scratch is 0 in every
// kernel; waves per SIMD is the occupancy the compiler reports:
//   kernel                              VGPRs  waves/SIMD
//   m6p_copy_kernel                        17      8
//   m6p_tree_kernel                        38      8
//   m6p_mid_kernel                         36      8
//   m6p_newton_kernel                      22      8
//   m6p_inv1_kernel                         4      8
//   m6p_deriv_rev_kernel                   17      8
//   m6p_weights_kernel                     17      8
//   m6p_sub_kernel                         21      8
//   m6p_iv_up_kernel<8, M6pElems>          40      8
//   m6p_iv_up_kernel<8, M6pMont>           28      8
//   m6p_iv_down_kernel<8, M6pElems>        94      5
//   m6p_iv_down_kernel<8, M6pMont>         88      5
//   m6p_iv_up_kernel<4, M6pRows>           45      8
//   m6p_iv_up_kernel<4, M6pMont>           21      8
//   m6p_iv_down_kernel<4, M6pRows>         80      6
//   m6p_iv_down_kernel<4, M6pMont>         48      8
// Tile constants kept: 256 lanes x 8 values (multi_inv, T = 2048) and 256 lanes x 4 rows (multi_interp_4, T = 1024), four times the
// generic chunks, as a word is a quarter of an fpm's registers.  Both down kernels stay without scratch and at 5 and 6 waves per SIMD,
// enough to cover the loads of kernels that read every item twice and write it once; the rows' finish() is about sixty products per
// row, and with the chunk walked by an unrolled loop instead of m6p_chunk_back_from's recursion the compiler declined the unroll and
// put the chunk in scratch (80 bytes per lane).  With 2 and 3 rows per lane the rows' down kernel has 62 and 65 VGPRs: nothing is
// gained by a smaller tile.  The LDS tree is 4 KiB per workgroup at every chunk.
#include "internal.hpp"
#include "mod64poly_items.cuh"

namespace {

constexpr int TPB = 256;
constexpr uint32_t L = M6P_IV_LANES;

inline dim3 grid_for(uint64_t work) {
  const uint64_t blocks = (work + TPB - 1) / TPB;
  constexpr uint64_t GX = 1ull << 22;
  return blocks <= GX ? dim3((unsigned)blocks) : dim3((unsigned)GX, (unsigned)((blocks + GX - 1) / GX));
}
__device__ __forceinline__ uint64_t tid() { return ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * TPB + threadIdx.x; }

// words i and i + 1 of p (the second only when two): one 16-byte access when wide (p + i is then 16-byte aligned: p is, i is even)
struct W2 {
  uint64_t a, b;
};
__device__ __forceinline__ W2 ld2(const uint64_t* p, uint64_t i, bool two, bool wide) {
  W2 r = {0, 0};
  if (wide && two) {
    const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p + i);
    r.a = v.x;
    r.b = v.y;
  } else {
    r.a = p[i];
    if (two) r.b = p[i + 1];
  }
  return r;
}
__device__ __forceinline__ void st2(uint64_t* p, uint64_t i, const W2& v, bool two, bool wide) {
  if (wide && two) {
    *reinterpret_cast<ulonglong2*>(p + i) = make_ulonglong2(v.a, v.b);
  } else {
    p[i] = v.a;
    if (two) p[i + 1] = v.b;
  }
}

__global__ void __launch_bounds__(TPB) m6p_copy_kernel(PaCopy c, const uint64_t* src, uint64_t* dst, f64_mod M) {
  const uint64_t g = tid();
  if (g >= c.rows * c.len) return;
  const uint64_t r = g / c.len, k = g - r * c.len;
  dst[r * c.ds + k] = m6p_copy_item(c, src, r, k, M);
}

// out rows j < nodes/2 of 2d = 2^log2d: the parent of transformed rows 2j, 2j + 1.  total and 2d are even, so a pair never straddles
// two rows and is never cut short.
__global__ void __launch_bounds__(TPB) m6p_tree_kernel(const uint64_t* hz, uint64_t* oz, const uint64_t* hn, uint64_t* on, uint32_t log2d,
                                                       uint64_t total, bool wide, f64_mod M) {
  const uint64_t g = 2 * tid();
  if (g >= total) return;
  const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1);
  const uint64_t a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
  const W2 A = ld2(hz, a, true, wide), B = ld2(hz, b, true, wide);
  if (oz) st2(oz, g, W2{m6p_tree_node(A.a, B.a, i, M), m6p_tree_node(A.b, B.b, i + 1, M)}, true, wide);
  if (on) {
    const W2 NA = ld2(hn, a, true, wide), NB = ld2(hn, b, true, wide);
    st2(on, g, W2{m6p_num_node(NA.a, NB.a, A.a, B.a, i, M), m6p_num_node(NA.b, NB.b, A.b, B.b, i + 1, M)}, true, wide);
  }
}

// children c = 2j, 2j + 1 at index i: hr[c] <- hd[j] * hr[c ^ 1]  (one thread per two sibling pairs)
__global__ void __launch_bounds__(TPB) m6p_mid_kernel(const uint64_t* hd, uint64_t* hr, uint32_t log2d, uint64_t pairs_total, bool wide,
                                                      f64_mod M) {
  const uint64_t g = 2 * tid();
  if (g >= pairs_total) return;
  const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1);
  const uint64_t a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
  const W2 D = ld2(hd, g, true, wide), RA = ld2(hr, a, true, wide), RB = ld2(hr, b, true, wide);
  W2 oa, ob;
  m6p_mid(D.a, RA.a, RB.a, &oa.a, &ob.a, M);
  m6p_mid(D.b, RA.b, RB.b, &oa.b, &ob.b, M);
  st2(hr, a, oa, true, wide);
  st2(hr, b, ob, true, wide);
}

__global__ void __launch_bounds__(TPB) m6p_newton_kernel(const uint64_t* F, uint64_t* G, uint64_t n, bool wide, f64_mod M) {
  const uint64_t g = 2 * tid();
  if (g >= n) return;
  const bool two = g + 1 < n;
  const W2 f = ld2(F, g, two, wide), x = ld2(G, g, two, wide);
  st2(G, g, W2{m6p_newton(f.a, x.a, M), two ? m6p_newton(f.b, x.b, M) : 0}, two, wide);
}

__global__ void __launch_bounds__(64) m6p_inv1_kernel(const uint64_t* src, uint64_t* dst, f64_mod M) {
  if (threadIdx.x == 0) *dst = m6p_inv1(*src, M);
}

__global__ void __launch_bounds__(TPB) m6p_deriv_rev_kernel(const uint64_t* top, uint64_t* out, uint64_t N, uint64_t n, f64_mod M) {
  const uint64_t g = tid();
  if (g >= N) return;
  out[g] = m6p_deriv_rev(top, N, n, g, M);
}

__global__ void __launch_bounds__(TPB) m6p_weights_kernel(const uint64_t* ys, const uint64_t* inv, uint64_t* out, uint64_t n, uint64_t N,
                                                          f64_mod M) {
  const uint64_t g = tid();
  if (g >= N) return;
  out[g] = g < n ? m6p_weight(ys[g], inv[g], M) : 0;
}

__global__ void __launch_bounds__(TPB) m6p_sub_kernel(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n, bool wide, f64_mod M) {
  const uint64_t g = 2 * tid();
  if (g >= n) return;
  const bool two = g + 1 < n;
  const W2 x = ld2(a, g, two, wide), y = ld2(b, g, two, wide);
  st2(out, g, W2{m6p_sub(x.a, y.a, M), two ? m6p_sub(x.b, y.b, M) : 0}, two, wide);
}

// ---- the batch inversion ---------------------------------------------------------------------------------------------------------------
template <uint32_t C, class Src>
__device__ __forceinline__ void tile_up(const Src& s, const f64_mod& M, uint64_t count, uint64_t* t, M6pChunk<C>& ch) {
  const uint32_t l = threadIdx.x;
  t[L + l] = m6p_chunk_forward<L, C>(s, M, count, blockIdx.x, l, ch);
  __syncthreads();
#pragma unroll 1
  for (uint32_t h = L / 2; h >= 1; h /= 2) {
    if (l < h) m6p_tree_up(t, h + l, M);
    __syncthreads();
  }
}

// level j -> level j + 1: the product of each tile, Montgomery form
template <uint32_t C, class Src>
__global__ void __launch_bounds__(L) m6p_iv_up_kernel(Src s, uint64_t count, uint64_t* next, f64_mod M) {
  __shared__ uint64_t t[2 * L];
  M6pChunk<C> ch;
  tile_up<C>(s, M, count, t, ch);
  if (threadIdx.x == 0) next[blockIdx.x] = t[1];
}

// tile_inv[tile] = the inverse of the tile's product (the level above, already inverted in place); nullptr: the single top tile, whose
// product is inverted here by the call's one p - 2 power
template <uint32_t C, class Src>
__global__ void __launch_bounds__(L) m6p_iv_down_kernel(Src s, uint64_t count, const uint64_t* tile_inv, f64_mod M) {
  __shared__ uint64_t t[2 * L];
  M6pChunk<C> ch;
  tile_up<C>(s, M, count, t, ch);
  const uint32_t l = threadIdx.x;
  if (l == 0) t[1] = tile_inv ? tile_inv[blockIdx.x] : m6p_top_inv(t[1], M);
  __syncthreads();
#pragma unroll 1
  for (uint32_t h = 1; h < L; h *= 2) {
    if (l < h) m6p_tree_down(t, h + l, M);
    __syncthreads();
  }
  m6p_chunk_backward<L, C>(s, M, count, blockIdx.x, l, ch, t[L + l]);
}

template <uint32_t C, class Src>
hipError_t run(const Src& items, uint64_t n, uint64_t* scratch, const f64_mod& M, hipStream_t st) {
  const IvLevels v = m6p_iv_levels<L, C>(n);
  auto level = [&](uint32_t j) { return M6pMont{scratch + v.off[j]}; };
  auto tiles = [&](uint32_t j) { return (unsigned)(v.count[j] / (L * C) + (v.count[j] % (L * C) ? 1 : 0)); };
  for (uint32_t j = 0; j + 1 < v.depth; ++j) {
    if (j == 0) hipLaunchKernelGGL((m6p_iv_up_kernel<C, Src>), dim3(tiles(0)), dim3(L), 0, st, items, v.count[0], scratch + v.off[1], M);
    else hipLaunchKernelGGL((m6p_iv_up_kernel<C, M6pMont>), dim3(tiles(j)), dim3(L), 0, st, level(j), v.count[j], scratch + v.off[j + 1], M);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  for (int j = (int)v.depth - 1; j >= 0; --j) {
    const uint64_t* above = j + 1 < (int)v.depth ? scratch + v.off[j + 1] : nullptr;
    if (j == 0) hipLaunchKernelGGL((m6p_iv_down_kernel<C, Src>), dim3(tiles(0)), dim3(L), 0, st, items, v.count[0], above, M);
    else hipLaunchKernelGGL((m6p_iv_down_kernel<C, M6pMont>), dim3(tiles(j)), dim3(L), 0, st, level(j), v.count[j], above, M);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// every array of a launch on a 16-byte boundary ?  (a null pointer is an array the launch does not touch)
inline bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

}  // namespace

#define M6P_LAUNCH(kernel, work, ...)                                             \
  do {                                                                            \
    hipLaunchKernelGGL(kernel, grid_for(work), dim3(TPB), 0, st, __VA_ARGS__);    \
    return hipGetLastError();                                                     \
  } while (0)

hipError_t shk_m6p_copy(const PaCopy& c, const uint64_t* src, uint64_t* dst, const f64_mod& M, hipStream_t st) {
  if (!c.rows || !c.len) return hipSuccess;
  M6P_LAUNCH(m6p_copy_kernel, c.rows * c.len, c, src, dst, M);
}
hipError_t shk_m6p_tree(const uint64_t* hz, uint64_t* oz, const uint64_t* hn, uint64_t* on, uint32_t log2d, uint64_t nodes,
                        const f64_mod& M, hipStream_t st) {
  const uint64_t total = (nodes / 2) << log2d;
  if (!total) return hipSuccess;
  if (log2d == 0) return hipErrorInvalidValue;  // a row is 2d >= 2 words: the pairs rely on it
  M6P_LAUNCH(m6p_tree_kernel, total / 2, hz, oz, hn, on, log2d, total, aligned16({hz, oz, hn, on}), M);
}
hipError_t shk_m6p_mid(const uint64_t* hd, uint64_t* hr, uint32_t log2d, uint64_t children, const f64_mod& M, hipStream_t st) {
  const uint64_t total = (children / 2) << log2d;
  if (!total) return hipSuccess;
  if (log2d == 0) return hipErrorInvalidValue;
  M6P_LAUNCH(m6p_mid_kernel, total / 2, hd, hr, log2d, total, aligned16({hd, hr}), M);
}
hipError_t shk_m6p_newton(const uint64_t* F, uint64_t* G, uint64_t n, const f64_mod& M, hipStream_t st) {
  if (!n) return hipSuccess;
  M6P_LAUNCH(m6p_newton_kernel, (n + 1) / 2, F, G, n, aligned16({F, G}), M);
}
hipError_t shk_m6p_inv1(const uint64_t* src, uint64_t* dst, const f64_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(m6p_inv1_kernel, dim3(1), dim3(64), 0, st, src, dst, M);
  return hipGetLastError();
}
hipError_t shk_m6p_deriv_rev(const uint64_t* top, uint64_t* out, uint64_t N, uint64_t n, const f64_mod& M, hipStream_t st) {
  if (!N) return hipSuccess;
  M6P_LAUNCH(m6p_deriv_rev_kernel, N, top, out, N, n, M);
}
hipError_t shk_m6p_weights(const uint64_t* ys, const uint64_t* inv, uint64_t* out, uint64_t n, uint64_t N, const f64_mod& M,
                           hipStream_t st) {
  if (!N) return hipSuccess;
  M6P_LAUNCH(m6p_weights_kernel, N, ys, inv, out, n, N, M);
}
hipError_t shk_m6p_sub(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n, const f64_mod& M, hipStream_t st) {
  if (!n) return hipSuccess;
  M6P_LAUNCH(m6p_sub_kernel, (n + 1) / 2, a, b, out, n, aligned16({a, b, out}), M);
}

uint64_t shk_m6p_multi_inv_scratch(uint64_t n) { return m6p_iv_levels<L, M6P_IV_CHUNK>(n).scratch; }
uint64_t shk_m6p_multi_interp_4_scratch(uint64_t rows) { return m6p_iv_levels<L, M6P_IV_ROW_CHUNK>(rows).scratch; }
hipError_t shk_m6p_multi_inv(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* scratch, const f64_mod& M, hipStream_t st) {
  return run<M6P_IV_CHUNK>(M6pElems{in, out}, n, scratch, M, st);
}
hipError_t shk_m6p_multi_interp_4(const uint64_t* xs, const uint64_t* ys, uint64_t* coeffs, uint64_t rows, uint64_t* scratch,
                                  const f64_mod& M, hipStream_t st) {
  return run<M6P_IV_ROW_CHUNK>(M6pRows{xs, ys, coeffs}, rows, scratch, M, st);
}
