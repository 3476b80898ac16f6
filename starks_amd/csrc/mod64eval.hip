// mod64eval.hip -- the kernels of polynomial evaluation at arbitrary points over any prime modulus below 2^64 on packed 64-bit words
// (sh_mod64_poly_eval; mod64eval_items.cuh has the element steps, poly_items.cuh both drivers, api_mod64poly.hip runs them).
// modeval.hip's launches over words: the per-point table of x^(2^b) in Montgomery form, the Horner kernel with every workgroup's sum
// for its group of points, the second launch that adds the workgroups; and the tree path's chunk rows, broadcast product and per-point
// combine.  The modulus block is a kernel argument of every launch: no __constant__, no global.
//
// chunks, bcast_mul and sum move 8 bytes per element and are memory-bound: every lane takes two consecutive words and moves them as
// one 16-byte access.  Workspace arrays are 16-byte aligned and always move so; where a launch touches a CALLER's array (chunks reads
// the coefficients, sum writes the output) the host decides per launch, as in mod64poly.hip: that pointer on a 16-byte boundary and
// an even row length, so that a pair never straddles two rows and stays aligned, else single words on that side.  sum also shares
// every output among min(W, 64) lanes of a wave: W is large exactly when the points are few.
//
// Compiler figures (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage; not measurements).  Scratch is 0 in every
// kernel; waves per SIMD is the occupancy the compiler reports:
//   kernel                   VGPRs  waves/SIMD  LDS bytes
//   m6e_pow_table_kernel        21      8            0
//   m6e_direct_kernel<4>        26      8         8192
//   m6e_direct_kernel<1>        18      8         2048
//   m6e_sum_kernel              24      8            0
//   m6e_chunks_kernel           16      8            0
//   m6e_bcast_mul_kernel        36      8            0
//   m6e_combine_kernel          30      8            0
// Points per lane.  The powers y[q] are uniform over a workgroup and live in scalar registers, so a point costs its accumulator alone:
// direct<8> has 36 VGPRs at 8 waves and 16 KiB of LDS, direct<16> 53 VGPRs at 5 waves and 32 KiB, both without scratch.
// Measured on the MI355X, forced direct path over Goldilocks, medians of 7 (profiles/r24_mod64_poly_eval.json, "group"), for 4 / 8 /
// 16 points per lane: 64 points x 2^20 coefficients 0.125 / 0.138 / 0.189 ms; 2^10 points x 2^16 coefficients 0.121 / 0.131 /
// 0.176 ms; 2^14 x 2^14, where every build fills the grid, 0.368 / 0.368 / 0.393 ms.  Four is kept.  More points per lane save
// coefficient loads that the caches serve anyway and cost workgroups: the shape rule (pe_direct_shape_of) gives a point group at most
// n / (64 x 256) workgroups, so at 64 x 2^20 four points per lane run 1024 workgroups, eight 512 and sixteen 256 on 256 CUs.  For the
// same reason m = G - 1, which runs one point per lane, is faster than m = G: over 2^20 coefficients 0.034 against 0.062 ms at G = 4
// (0.035 / 0.100 at 8, 0.045 / 0.173 at 16).  Not tried: a shape rule of this path's own, which poly_items.cuh would have to carry.
// 1 point x 2^24 coefficients takes 0.068 ms, 2.0 TB/s of coefficients against the 6.3 TB/s the chip copies at: direct<1> is 47 us
// of it in a kernel trace (profiles/r24_mod64_poly_eval_kernel_stats.csv) and runs one dependent product chain per lane at 4 waves
// per SIMD -- bound by the chain's latency, not by bytes; with one lane per output the sum of its 1024 workgroups took another 143 us
// (profiles/r24_mod64_poly_eval_kernel_stats_lane_per_output.csv, a trace of that earlier build), which is why sum shares an output
// among lanes: 7 us now.
#include "internal.hpp"
#include "mod64eval_items.cuh"

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

// words i and i + 1 of p as one 16-byte access (p + i is 16-byte aligned: the host checked p, i is even)
struct W2 {
  uint64_t a, b;
};
__device__ __forceinline__ W2 ld2(const uint64_t* p, uint64_t i) {
  const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p + i);
  return W2{v.x, v.y};
}
__device__ __forceinline__ void st2(uint64_t* p, uint64_t i, const W2& v) {
  *reinterpret_cast<ulonglong2*>(p + i) = make_ulonglong2(v.a, v.b);
}

__global__ void __launch_bounds__(TPB) m6e_pow_table_kernel(const uint64_t* xs, uint64_t m, uint32_t lgS, uint64_t* tbl, f64_mod M) {
  const uint64_t i = tid();
  if (i < m) m6e_pow_table_item(xs, m, lgS, tbl, i, M);
}

// workgroup (b, group, w): lanes g = w PE_WG + threadIdx.x of the group's points; dst[(b W + w) m + i] = the lanes' sum for point i.
// Every lane's value is canonical and f64_add is exact, so the LDS tree below gives the same bits in any order and for any W.
template <int G>
__global__ void __launch_bounds__(TPB) m6e_direct_kernel(PeDirect s, const uint64_t* coefs, const uint64_t* tbl, uint64_t* dst, f64_mod M) {
  __shared__ uint64_t red[G][TPB];
  const uint64_t blk = block_id();
  if (blk >= s.batch * s.groups * s.W) return;  // uniform per workgroup
  const uint64_t w = blk % s.W, bg = blk / s.W, grp = bg % s.groups, b = bg / s.groups, i0 = grp * G;
  const uint32_t lane = threadIdx.x;
  uint64_t acc[G];
  m6e_lane<G>(s, coefs + b * s.n, tbl, i0, w * TPB + lane, acc, M);
#pragma unroll
  for (int q = 0; q < G; ++q) red[q][lane] = acc[q];
  __syncthreads();
  for (uint32_t h = TPB / 2; h > 0; h >>= 1) {
    if (lane < h) {
#pragma unroll
      for (int q = 0; q < G; ++q) red[q][lane] = f64_add(red[q][lane], red[q][lane + h], M);
    }
    __syncthreads();
  }
  if (lane < G && i0 + lane < s.m) dst[(b * s.W + w) * s.m + i0 + lane] = red[lane][0];
}

// A unit is one output word, or, when wide, two consecutive ones (m is even and part, out are 16-byte aligned, so the pair is one
// row's points i, i + 1 at an even index everywhere).  SL = 2^lgSL <= 64 consecutive lanes share a unit: lane `sub` adds the workgroup
// sums w = sub, sub + SL, ... and the SL partial sums meet by shuffles inside the wave.  W is large exactly when there are few points
// (1 point x 2^24 coefficients: W = 1024), where one lane per output would walk its W loads one after the other; f64_add is exact, so
// the order of the additions changes no bit.  Every lane of a wave reaches the shuffles: idle units carry zeros.
__global__ void __launch_bounds__(TPB) m6e_sum_kernel(PeDirect s, const uint64_t* part, uint64_t* out, uint32_t lgSL, bool wide, f64_mod M) {
  const uint64_t t = tid(), unit = t >> lgSL, total = s.batch * s.m, units = wide ? total / 2 : total;
  const uint32_t SL = 1u << lgSL, sub = (uint32_t)t & (SL - 1);
  const bool live = unit < units;
  const uint64_t g = wide ? 2 * unit : unit, b = live ? g / s.m : 0, i = g - b * s.m;
  W2 acc = {0, 0};
  if (live) {
    if (wide) {
      for (uint64_t w = sub; w < s.W; w += SL) {
        const W2 v = ld2(part, (b * s.W + w) * s.m + i);
        acc.a = f64_add(acc.a, v.a, M);
        acc.b = f64_add(acc.b, v.b, M);
      }
    } else {
      acc.a = m6e_sum_item(s, part, b, i, sub, SL, M);
    }
  }
  for (uint32_t h = SL / 2; h > 0; h >>= 1) {
    acc.a = f64_add(acc.a, __shfl_xor((unsigned long long)acc.a, (int)h), M);
    acc.b = f64_add(acc.b, __shfl_xor((unsigned long long)acc.b, (int)h), M);
  }
  if (live && sub == 0) {
    if (wide) st2(out, g, acc);
    else out[g] = acc.a;
  }
}

// rows of N >= 2 words (N a power of two) and total even: the pair g, g + 1 is one row's k, k + 1, read from s, s - 1.  dst is a
// workspace buffer, 16-byte aligned (the launcher refuses another); wide_src: the caller's coefs is too and n is even, so
// b n + s - 1 is even
__global__ void __launch_bounds__(TPB) m6e_chunks_kernel(const uint64_t* coefs, uint64_t n, uint64_t N, uint64_t C, uint64_t total,
                                                         uint64_t* dst, bool wide_src) {
  const uint64_t g = 2 * tid();
  if (g >= total) return;
  const uint64_t r = g / N, k = g - r * N;
  const uint64_t b = r / C, s = (r - b * C) * N + N - 1 - k;  // m6e_chunk_rev_item's source of k; k + 1 reads s - 1 >= 0
  W2 v;
  if (wide_src && s < n) {
    const W2 u = ld2(coefs, b * n + s - 1);
    v = W2{u.b, u.a};
  } else {
    v = W2{m6e_chunk_rev_item(coefs, n, N, C, r, k), m6e_chunk_rev_item(coefs, n, N, C, r, k + 1)};
  }
  st2(dst, g, v);
}

// len and total are even: the pair g, g + 1 is one row's i, i + 1 with i even.  Both arrays are workspace buffers, 16-byte aligned
// (the launcher refuses others): there is no single-word form
__global__ void __launch_bounds__(TPB) m6e_bcast_mul_kernel(uint64_t* a, const uint64_t* b, uint64_t len, uint64_t total, f64_mod M) {
  const uint64_t g = 2 * tid();
  if (g >= total) return;
  const W2 x = ld2(a, g), y = ld2(b, g % len);
  st2(a, g, W2{m6e_bcast_mul_item(x.a, y.a, M), m6e_bcast_mul_item(x.b, y.b, M)});
}

__global__ void __launch_bounds__(TPB) m6e_combine_kernel(const uint64_t* leaves, const uint64_t* xs, uint64_t m, uint64_t N, uint64_t C,
                                                          uint64_t total, uint64_t* out, f64_mod M) {
  const uint64_t g = tid();
  if (g >= total) return;
  const uint64_t b = g / m, i = g - b * m;
  out[g] = m6e_combine_item(leaves, xs, N, C, b, i, M);
}

// every array of a launch on a 16-byte boundary ?
inline bool aligned16(std::initializer_list<const void*> ps) {
  uintptr_t bits = 0;
  for (const void* p : ps) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

}  // namespace

hipError_t shk_m6e_pow_table(const uint64_t* xs, uint64_t m, uint32_t lgS, uint64_t* tbl, const f64_mod& M, hipStream_t st) {
  hipLaunchKernelGGL(m6e_pow_table_kernel, grid_for(m), dim3(TPB), 0, st, xs, m, lgS, tbl, M);
  return hipGetLastError();
}
hipError_t shk_m6e_direct(const PeDirect& s, const uint64_t* coefs, const uint64_t* tbl, uint64_t* dst, const f64_mod& M, hipStream_t st) {
  const dim3 grid = grid_for(s.batch * s.groups * s.W * TPB);
  if (s.G == M6E_GROUP)
    hipLaunchKernelGGL(m6e_direct_kernel<M6E_GROUP>, grid, dim3(TPB), 0, st, s, coefs, tbl, dst, M);
  else if (s.G == 1)
    hipLaunchKernelGGL(m6e_direct_kernel<1>, grid, dim3(TPB), 0, st, s, coefs, tbl, dst, M);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t shk_m6e_sum(const PeDirect& s, const uint64_t* part, uint64_t* out, const f64_mod& M, hipStream_t st) {
  const bool wide = s.m % 2 == 0 && aligned16({part, out});
  uint32_t lgSL = 0;  // SL = min(W, 64) lanes per unit, W a power of two
  while (lgSL < 6 && (2ull << lgSL) <= s.W) ++lgSL;
  const uint64_t units = wide ? s.batch * s.m / 2 : s.batch * s.m;
  hipLaunchKernelGGL(m6e_sum_kernel, grid_for(units << lgSL), dim3(TPB), 0, st, s, part, out, lgSL, wide, M);
  return hipGetLastError();
}
hipError_t shk_m6e_chunks(const uint64_t* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, uint64_t* dst, hipStream_t st) {
  const uint64_t total = batch * C * N;
  if (N < 2 || (N & (N - 1)) || !aligned16({dst})) return hipErrorInvalidValue;  // rows of an even number of words, pairs stored whole
  hipLaunchKernelGGL(m6e_chunks_kernel, grid_for(total / 2), dim3(TPB), 0, st, coefs, n, N, C, total, dst,
                     n % 2 == 0 && aligned16({coefs}));
  return hipGetLastError();
}
hipError_t shk_m6e_bcast_mul(uint64_t* a, const uint64_t* b, uint64_t rows, uint64_t len, const f64_mod& M, hipStream_t st) {
  const uint64_t total = rows * len;
  if (len % 2 || !aligned16({a, b})) return hipErrorInvalidValue;
  hipLaunchKernelGGL(m6e_bcast_mul_kernel, grid_for(total / 2), dim3(TPB), 0, st, a, b, len, total, M);
  return hipGetLastError();
}
hipError_t shk_m6e_combine(const uint64_t* leaves, const uint64_t* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, uint64_t* out,
                           const f64_mod& M, hipStream_t st) {
  const uint64_t total = batch * m;
  hipLaunchKernelGGL(m6e_combine_kernel, grid_for(total), dim3(TPB), 0, st, leaves, xs, m, N, C, total, out, M);
  return hipGetLastError();
}
