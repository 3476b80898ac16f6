// modwitness.hip -- STARK witnesses on the device over any odd modulus 3 <= p < 2^256 from any AIR's step polynomials: witness.hip's
// twin on fpm.cuh.  The modulus block travels by value as a kernel argument; there is no __constant__ and no device global.
//
// One dispatch writes rows [k0, k1) of every unit's [width][steps] witness; the host (api_modstark.hip) launches the trace in slices,
// each one resuming from the row the previous one wrote.  The step of one unit is split over a group of G lanes of one wave
// (witness_items.cuh: wi_plan; modwitness_items.cuh: mwi_lane, mwi_gather); 64 / G units share a wave and run the same split.  The
// term table is staged in LDS once per dispatch from the image mod_stark_terms uploaded for the prover and the verifier (Montgomery
// coefficients, exponent rows of W bytes); the "coefficient is 1" flag is derived here (mwi_unit).
//
// The exchange of a step goes through LDS without a workgroup barrier, exactly as in witness.hip: a group never leaves its wave, each
// lane owns W slots, and the wave-local fence / wave_barrier / fence orders the wave's writes before its reads and the reads before the
// next step's writes.
//
// STORE (modwitness_items.cuh): MWI_PASS leaves Montgomery rows for mod_witness_finish_kernel, MWI_INLINE converts on the store path.
#include <type_traits>

#include "internal.hpp"
#include "modntt_items.cuh"  // mn_ld, mn_st
#include "modwitness_items.cuh"

namespace {

constexpr int WG = 64;  // one wave per workgroup: the kernel is latency-bound, so waves are spread over as many CUs as possible

#define SHK_WAVE_SYNC()                                    \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)

// f(integral_constant<int, c>) for c = C .. W - 1.  The two loops over the dimensions that hold a conversion product per dimension are
// written with it: as `#pragma unroll` loops they exceed the pragma's size limit from width 5 up, stay loops, and P[] -- then indexed
// by a loop variable -- moves to scratch for the whole kernel.
template <int C, int W, class F>
__device__ __forceinline__ void each_dim(F&& f) {
  if constexpr (C < W) {
    f(std::integral_constant<int, C>{});
    each_dim<C + 1, W>(f);
  }
}

template <int W, int STORE>
__global__ void __launch_bounds__(WG) mod_witness_kernel(ModWitnessArgs a, fpm_mod M) {
  __shared__ WiRow rows[SHK_STARK_MAX_TERMS];
  __shared__ fpm coefs[SHK_STARK_MAX_TERMS];
  __shared__ fpm slots[WG * W];
  for (uint32_t t = threadIdx.x; t < a.nterms; t += WG) {
    uint32_t dim = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) dim += a.begin[c + 1] <= t ? 1u : 0u;
    const fpm cf = mn_ld(a.coef + t);
    rows[t] = wi_pack_row(dim, mwi_unit(cf, M), a.exps + (uint64_t)t * W, W);
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
  fpm* col = a.wit + unit * W * s;
  fpm P[W];
  uint64_t k = a.k0;
  if (k == 0) {  // witness[c][0] = inputs[c] mod p: fpm_to_mont takes any 256-bit value
    each_dim<0, W>([&](auto ci) {
      constexpr int c = decltype(ci)::value;
      P[c] = fpm_to_mont(mn_ld(a.inputs + unit * W + c), M);
      if ((uint32_t)c % G == j) mn_st(col + c * s, mwi_stored<STORE>(P[c], M));
    });
    k = 1;
  } else {  // resume from the row the previous dispatch wrote
    each_dim<0, W>([&](auto ci) {
      constexpr int c = decltype(ci)::value;
      P[c] = mwi_resumed<STORE>(mn_ld(col + c * s + (k - 1)), M);
    });
  }
  fpm* mine = slots + lane * W;
  const fpm* group = slots + (lane - j) * W;
#pragma unroll 1
  for (; k < a.k1; ++k) {
    fpm Q[W];
    mwi_lane<W>(rows, coefs, t0, t1, P, Q, M);
    if (G == 1) {
#pragma unroll
      for (int c = 0; c < W; ++c) P[c] = Q[c];
    } else {
#pragma unroll
      for (int c = 0; c < W; ++c) mine[c] = Q[c];
      SHK_WAVE_SYNC();
      mwi_gather<W>(group, a.plan, P, M);
      SHK_WAVE_SYNC();
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
      if ((uint32_t)c % G == j) mn_st(col + c * s + k, mwi_stored<STORE>(P[c], M));
  }
}

// MWI_PASS's closing pass over the whole witness: bandwidth-bound, grid-stride
__global__ void __launch_bounds__(256) mod_witness_finish_kernel(fpm* wit, uint64_t count, fpm_mod M) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) mn_st(wit + i, mwi_finish(mn_ld(wit + i), M));
}

template <int W>
hipError_t launch(const ModWitnessArgs& a, const fpm_mod& M, bool inl, hipStream_t st) {
  const uint32_t per = WG / a.plan.group;
  const dim3 grid((a.batch + per - 1) / per), block(WG);
  if (inl) hipLaunchKernelGGL((mod_witness_kernel<W, MWI_INLINE>), grid, block, 0, st, a, M);
  else hipLaunchKernelGGL((mod_witness_kernel<W, MWI_PASS>), grid, block, 0, st, a, M);
  return hipGetLastError();
}

}  // namespace

// rows [k0, k1) of the witnesses of a.batch units over M; width 1 .. SHK_STARK_MAX_WIDTH (checked by the caller)
hipError_t shk_mod_witness_slice(const ModWitnessArgs& a, const fpm_mod& M, uint32_t width, bool inl, hipStream_t st) {
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

// count Montgomery values -> plain canonical, in place
hipError_t shk_mod_witness_finish(fpm* wit, uint64_t count, const fpm_mod& M, hipStream_t st) {
  const uint64_t blocks = (count + 255) / 256;
  hipLaunchKernelGGL(mod_witness_finish_kernel, dim3((uint32_t)(blocks < (1u << 16) ? blocks : (1u << 16))), dim3(256), 0, st, wit, count, M);
  return hipGetLastError();
}
