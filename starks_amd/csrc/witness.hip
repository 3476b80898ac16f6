// witness.hip -- STARK witnesses on the device from any AIR's step polynomials (AIR.generate_witness, starks/air.py:32-52, 121-123).
//
// One dispatch writes rows [k0, k1) of every unit's [width][steps] witness; the host (api_stark.hip) launches the trace in such slices so that
// no dispatch walks an unbounded number of steps, each one resuming from the row the previous one wrote.  The step of one unit is split
// over a group of G lanes of one wave (witness_items.cuh: wi_plan, wi_lane, wi_gather); 64 / G units share a wave and run the same
// split, so their lanes take the same branches.  The term table of the system is staged in LDS once per dispatch, from the table
// stark_terms uploaded for the prover (coefficients and exponent rows only).
//
// The exchange of a step goes through LDS without a workgroup barrier: a group never leaves its wave and each lane owns W slots.  Every
// lane writes its partial sums to its own slots, then SHK_WAVE_SYNC orders the wave's LDS writes before its reads (a wave's LDS
// instructions execute in issue order; the fences make the compiler wait for the writes and keep the reads behind them), the lanes read
// the slots of their group, and a second SHK_WAVE_SYNC keeps the next step's writes behind those reads.  No other wave touches the slots.
#include "internal.hpp"
#include "witness_items.cuh"

namespace {

constexpr int WG = 64;  // one wave per workgroup: the kernel is latency-bound, so waves are spread over as many CUs as possible

#define SHK_WAVE_SYNC()                                    \
  do {                                                     \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); \
    __builtin_amdgcn_wave_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); \
  } while (0)

template <int W>
__global__ void __launch_bounds__(WG) witness_kernel(WitnessArgs a) {
  __shared__ WiRow rows[SHK_STARK_MAX_TERMS];
  __shared__ fp coefs[SHK_STARK_MAX_TERMS];
  __shared__ fp slots[WG * W];
  for (uint32_t t = threadIdx.x; t < a.nterms; t += WG) {
    uint32_t dim = 0;
#pragma unroll
    for (int c = 0; c < W; ++c) dim += a.begin[c + 1] <= t ? 1u : 0u;
    const uint8_t* ex = a.exps + (uint64_t)t * (W + 1);
    rows[t] = wi_pack_row(dim, ex[W] != 0, ex, W);
    coefs[t] = fp_load(a.coef + t);
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
  fp* col = a.wit + unit * W * s;
  fp P[W];
  uint64_t k = a.k0;
  if (k == 0) {  // witness[c][0] = inputs[c] mod p
#pragma unroll
    for (int c = 0; c < W; ++c) {
      P[c] = fp_load(a.inputs + unit * W + c);
      if ((uint32_t)c % G == j) fp_store(col + c * s, fp_canon(P[c]));
    }
    k = 1;
  } else {  // resume from the row the previous dispatch wrote
#pragma unroll
    for (int c = 0; c < W; ++c) P[c] = fp_load(col + c * s + (k - 1));
  }
  fp* mine = slots + lane * W;
  const fp* group = slots + (lane - j) * W;
#pragma unroll 1
  for (; k < a.k1; ++k) {
    fp Q[W];
    wi_lane<W>(rows, coefs, t0, t1, P, Q);
    if (G == 1) {
#pragma unroll
      for (int c = 0; c < W; ++c) P[c] = Q[c];
    } else {
#pragma unroll
      for (int c = 0; c < W; ++c) mine[c] = Q[c];
      SHK_WAVE_SYNC();
      wi_gather<W>(group, a.plan, P);
      SHK_WAVE_SYNC();
    }
#pragma unroll
    for (int c = 0; c < W; ++c)
      if ((uint32_t)c % G == j) fp_store(col + c * s + k, fp_canon(P[c]));
  }
}

template <int W>
hipError_t launch(const WitnessArgs& a, hipStream_t st) {
  const uint32_t per = WG / a.plan.group;
  hipLaunchKernelGGL(witness_kernel<W>, dim3((a.batch + per - 1) / per), dim3(WG), 0, st, a);
  return hipGetLastError();
}

}  // namespace

// rows [k0, k1) of the witnesses of a.batch units; width 1 .. SHK_STARK_MAX_WIDTH (checked by the caller)
hipError_t shk_stark_witness_slice(const WitnessArgs& a, uint32_t width, hipStream_t st) {
  switch (width) {
    case 1: return launch<1>(a, st);
    case 2: return launch<2>(a, st);
    case 3: return launch<3>(a, st);
    case 4: return launch<4>(a, st);
    case 5: return launch<5>(a, st);
    case 6: return launch<6>(a, st);
    case 7: return launch<7>(a, st);
    case 8: return launch<8>(a, st);
    case 9: return launch<9>(a, st);
    default: return hipErrorInvalidValue;
  }
}
