// mod64witness.hip -- STARK witnesses on the device over any odd modulus 3 <= p < 2^64 on packed 64-bit words, from any AIR's step
// polynomials: modwitness.hip's twin on fp64m.cuh.  The f64_mod block travels by value as a kernel argument; there is no __constant__
// and no device global.
//
// One dispatch writes rows [k0, k1) of every unit's [width][steps] witness; the host (api_mod64stark.hip) launches the trace in slices,
// each one resuming from the row the previous one wrote.  The step of one unit is split over a group of G lanes of one wave
// (witness_items.cuh: wi_plan; mod64witness_items.cuh: m6w_lane, m6w_gather); 64 / G units share a wave and run the same split.  The
// term table is staged in LDS once per dispatch from the image mod64_stark_terms uploaded for the packed prover (Montgomery coefficient
// words, exponent rows of W bytes); the "coefficient is 1" flag is derived here (m6w_unit).
//
// The exchange of a step goes through LDS without a workgroup barrier, exactly as in witness.hip: a group never leaves its wave, each
// lane owns W slots of 8 bytes, and the wave-local fence / wave_barrier / fence orders the wave's writes before its reads and the reads
// before the next step's writes.  The only addresses that depend on data are the witness rows; none depends on a field value.
//
// STORE (mod64witness_items.cuh): M6W_PASS leaves Montgomery rows for mod64_witness_finish_kernel, M6W_INLINE converts on the store path.
#include <type_traits>

#include "internal.hpp"
#include "mod64witness_items.cuh"

namespace {

constexpr int WG = 64;  // one wave per workgroup: the kernel is latency-bound, so waves are spread over as many CUs as possible

#define SHK_WAVE_SYNC()                                    \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)

// f(integral_constant<int, c>) for c = C .. W - 1 (modwitness.hip: each_dim): the loops over the dimensions that hold a conversion
// product per dimension stay straight-line code, so P[] is never indexed by a loop variable and stays in registers
template <int C, int W, class F>
__device__ __forceinline__ void each_dim(F&& f) {
  if constexpr (C < W) {
    f(std::integral_constant<int, C>{});
    each_dim<C + 1, W>(f);
  }
}

template <int W, int STORE>
__global__ void __launch_bounds__(WG) mod64_witness_kernel(Mod64WitnessArgs a, f64_mod M) {
  __shared__ WiRow rows[SHK_STARK_MAX_TERMS];
  __shared__ uint64_t coefs[SHK_STARK_MAX_TERMS];
  __shared__ uint64_t slots[WG * W];
  for (uint32_t t = threadIdx.x; t < a.nterms; t += WG) {  // nterms <= SHK_STARK_MAX_TERMS (checked by the caller)
    uint32_t dim = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) dim += a.begin[c + 1] <= t ? 1u : 0u;
    const uint64_t cf = a.coef[t];
    rows[t] = wi_pack_row(dim, m6w_unit(cf, M), a.exps + (uint64_t)t * W, W);
    coefs[t] = cf;
  }
  __syncthreads();
  const uint32_t G = a.plan.group, lane = threadIdx.x, j = lane & (G - 1);
  const uint64_t unit = (uint64_t)blockIdx.x * (WG / G) + lane / G;
  if (unit >= a.batch) return;  // whole groups only: G divides the wave
  uint32_t t0 = 0, t1 = 0;
#pragma unroll
  for (uint32_t i = 0; i < WI_MAX_GROUP; ++i)  // static indices: a lane-indexed kernel argument would be copied to scratch
    if (j == i) {
      t0 = a.plan.t0[i];
      t1 = a.plan.t1[i];
    }
  const uint64_t s = a.steps;
  uint64_t* col = a.wit + unit * W * s;
  uint64_t P[W];
  uint64_t k = a.k0;
  if (k == 0) {  // witness[c][0] = inputs[c] mod p: f64_to_mont takes any 64-bit word
    each_dim<0, W>([&](auto ci) {
      constexpr int c = decltype(ci)::value;
      P[c] = f64_to_mont(a.inputs[unit * W + c], M);
      if ((uint32_t)c % G == j) col[c * s] = m6w_stored<STORE>(P[c], M);
    });
    k = 1;
  } else {  // resume from the row the previous dispatch wrote
    each_dim<0, W>([&](auto ci) {
      constexpr int c = decltype(ci)::value;
      P[c] = m6w_resumed<STORE>(col[c * s + (k - 1)], M);
    });
  }
  uint64_t* mine = slots + lane * W;
  const uint64_t* group = slots + (lane - j) * W;
#pragma unroll 1
  for (; k < a.k1; ++k) {
    uint64_t Q[W];
    m6w_lane<W>(rows, coefs, t0, t1, P, Q, M);
    if (G == 1) {
#pragma unroll
      for (int c = 0; c < W; ++c) P[c] = Q[c];
    } else {
#pragma unroll
      for (int c = 0; c < W; ++c) mine[c] = Q[c];
      SHK_WAVE_SYNC();
      m6w_gather<W>(group, a.plan, P, M);
      SHK_WAVE_SYNC();
    }
    each_dim<0, W>([&](auto ci) {
      constexpr int c = decltype(ci)::value;
      if ((uint32_t)c % G == j) col[c * s + k] = m6w_stored<STORE>(P[c], M);
    });
  }
}

// M6W_PASS's closing pass over the whole witness: bandwidth-bound, grid-stride
__global__ void __launch_bounds__(256) mod64_witness_finish_kernel(uint64_t* wit, uint64_t count, f64_mod M) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) wit[i] = m6w_finish(wit[i], M);
}

template <int W>
hipError_t launch(const Mod64WitnessArgs& a, const f64_mod& M, bool inl, hipStream_t st) {
  const uint32_t per = WG / a.plan.group;
  const dim3 grid((a.batch + per - 1) / per), block(WG);
  if (inl) hipLaunchKernelGGL((mod64_witness_kernel<W, M6W_INLINE>), grid, block, 0, st, a, M);
  else hipLaunchKernelGGL((mod64_witness_kernel<W, M6W_PASS>), grid, block, 0, st, a, M);
  return hipGetLastError();
}

}  // namespace

// rows [k0, k1) of the witnesses of a.batch units over M; width 1 .. SHK_STARK_MAX_WIDTH (checked by the caller)
hipError_t shk_mod64_witness_slice(const Mod64WitnessArgs& a, const f64_mod& M, uint32_t width, bool inl, hipStream_t st) {
  switch (width) {
    case 1: return launch<1>(a, M, inl, st);
    case 2: return launch<2>(a, M, inl, st);
    case 3: return launch<3>(a, M, inl, st);
    case 4: return launch<4>(a, M, inl, st);
    case 5: return launch<5>(a, M, inl, st);
    case 6: return launch<6>(a, M, inl, st);
    case 7: return launch<7>(a, M, inl, st);
    case 8: return launch<8>(a, M, inl, st);
    case 9: return launch<9>(a, M, inl, st);
    default: return hipErrorInvalidValue;
  }
}

// count Montgomery words -> plain canonical, in place
hipError_t shk_mod64_witness_finish(uint64_t* wit, uint64_t count, const f64_mod& M, hipStream_t st) {
  const uint64_t blocks = (count + 255) / 256;
  hipLaunchKernelGGL(mod64_witness_finish_kernel, dim3((uint32_t)(blocks < (1u << 16) ? blocks : (1u << 16))), dim3(256), 0, st, wit, count, M);
  return hipGetLastError();
}
