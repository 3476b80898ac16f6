// modverify_dev.hip -- the batched device verifiers of FRI and STARK proofs over a run-time modulus below 2^256 (sh_dev_mod_fri_verify,
// sh_dev_mod_stark_verify, include/starkhip.h): every proof of a batch checked as shk::mod_fri_verify (modverify.hip) checks it, in verify_dev.hip's split:
//   1. index sets, 2. Merkle branches   verify_dev.hip's own kernels (field-free: shk_verify_sets_and_branches)
//   3. FRI rows     one lane per (proof, round, sample), blockIdx.y = round: mv_fri_row
//   3'. spot checks (STARK proofs, sh_dev_mod_stark_verify) one lane per (proof, sample) in 64-lane blocks: mv_spot
//   4. final layer  one workgroup per proof: permute4 tree in LDS against the last root, then the degree bound over the lanes in the
//                   cross-multiplied form (modverify_items.cuh); it also writes the statuses (everything before it is ahead of it
//                   on the stream)
// The modulus block and every plan constant travel BY VALUE as kernel arguments: no __constant__, no device global, so two contexts
// with different moduli run side by side.  No address depends on proof bytes: offsets come from the plan, sampled indices only pick
// exponents.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "modverify_items.cuh"

namespace {

constexpr uint32_t MV_TPB = 256;

struct MvRowRound {
  fpm w, inv_i;
  uint64_t roudeg, off;
  int64_t root_off;
  uint32_t samples, set_off, l1, l2;
};
struct MvRowsArgs {
  MvRowRound r[SHK_FRI_MAX_ROUNDS];
};
// blockIdx.y = round
__global__ void __launch_bounds__(MV_TPB) mv_fri_rows_kernel(const uint8_t* proofs, uint64_t plen, const uint8_t* roots, uint32_t batch,
                                                             fpm_mod M, MvRowsArgs a, const uint32_t* ys, uint32_t ys_per, uint32_t* flags) {
  const MvRowRound& rd = a.r[blockIdx.y];
  const uint64_t g = (uint64_t)blockIdx.x * MV_TPB + threadIdx.x;
  if (g >= (uint64_t)rd.samples * batch) return;
  const uint32_t b = (uint32_t)(g / rd.samples), i = (uint32_t)(g - (uint64_t)b * rd.samples);
  const uint8_t* proof = proofs + (uint64_t)b * plen;
  const uint8_t* mroot = rd.root_off < 0 ? roots + 32ull * b : proof + rd.root_off;
  const fpm sx = mv_field_mont(mroot, M);  // field(m[1]) (fri.py:229), used modulo p
  const uint8_t* sample = proof + rd.off + 32 + (uint64_t)i * 32 * (rd.l2 + 4ull * rd.l1);
  const uint32_t y = ys[(uint64_t)b * ys_per + rd.set_off + i];
  if (!mv_fri_row(sample, rd.l1, rd.l2, rd.w, rd.inv_i, rd.roudeg, y, sx, M)) flags[b] = 1;
}

struct MvSpotArgs {
  MvSpotConst sc;
  uint64_t pb, lb, io_stride;
  uint32_t samples, row;
  uint32_t tbegin[SHK_STARK_MAX_WIDTH + 1];
};
// one lane per (proof, sample): the transition and boundary constraints at x = G2^pos (mv_spot)
__global__ void __launch_bounds__(64) mv_spot_kernel(const uint8_t* proofs, uint64_t plen, uint32_t batch, fpm_mod M, MvSpotArgs a,
                                                     const fpm* inputs, const fpm* outputs, const fpm* coef, const uint8_t* exps,
                                                     const uint32_t* ys, uint32_t ys_per, uint32_t* flags) {
  const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= (uint64_t)a.samples * batch) return;
  const uint32_t b = (uint32_t)(g / a.samples), i = (uint32_t)(g - (uint64_t)b * a.samples);
  const uint8_t* b1 = proofs + (uint64_t)b * plen + 64 + (2 * a.pb + a.lb) * i;
  const uint64_t io = (uint64_t)b * a.sc.width * a.io_stride;
  if (!mv_spot(b1, b1 + a.pb, ys[(uint64_t)b * ys_per + i], a.sc, inputs + io, outputs + io, a.io_stride, coef, exps, a.row, a.tbegin, M))
    flags[b] = 1;
}

struct MvFinalArgs {
  fpm w, D;
  fpm xk[VB_MAX_K], cof[VB_MAX_K];
  uint64_t off, len, k;
  int64_t root_off;  // the last committed root; -1: the caller's root (no FRI round)
  uint32_t exclude;
};
// one workgroup per proof; dynamic LDS: the tree's nodes [1, len) of 32 bytes (the layout of merkelize, merkle_tree.py:36-56)
__global__ void __launch_bounds__(MV_TPB) mv_final_kernel(const uint8_t* proofs, uint64_t plen, const uint8_t* roots, fpm_mod M,
                                                          MvFinalArgs a, const uint32_t* flags, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t nodes[];  // [len][8]
  __shared__ fpm xk[VB_MAX_K], wgt[VB_MAX_K];
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* proof = proofs + (uint64_t)b * plen;
  const uint8_t* data = proof + a.off;
  const uint32_t len = (uint32_t)a.len;
  bool bad = false;
  // nodes [len/2, len) from the permuted leaves (permute4, merkle_tree.py:11-23), then level by level up to the root
  for (uint32_t m = len / 2 + tid; m < len; m += MV_TPB) {
    uint32_t l[8], r[8];
    vb_load8(data + 32 * vb_final_leaf(2 * m - len, len), l);
    vb_load8(data + 32 * vb_final_leaf(2 * m + 1 - len, len), r);
    const b2digest d = b2_hash_pair(l, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) nodes[8 * m + i] = d.h[i];
  }
  for (uint32_t s = len / 2; s > 1; s /= 2) {
    __syncthreads();
    for (uint32_t m = s / 2 + tid; m < s; m += MV_TPB) {
      const b2digest d = b2_hash_pair(nodes + 16 * m, nodes + 16 * m + 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) nodes[8 * m + i] = d.h[i];
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t r[8];
    vb_load8(a.root_off < 0 ? roots + 32ull * b : proof + a.root_off, r);
    for (int i = 0; i < 8; ++i) bad = bad || nodes[8 + i] != r[i];
  }
  // the degree bound: weights of the first k retained points, then the other points over the lanes
  const uint64_t k = a.k, np = vb_npts(a.len, a.exclude);
  if (tid < k) {
    xk[tid] = a.xk[tid];
    wgt[tid] = mv_final_weight(tid, a.exclude, data, a.cof, M);
  }
  __syncthreads();
  for (uint64_t t = k + tid; t < np; t += MV_TPB)
    if (!mv_final_point(t, k, a.w, a.exclude, data, xk, wgt, a.D, M)) bad = true;
  bad = __syncthreads_or(bad);
  if (tid == 0) status[b] = (bad || flags[b]) ? SH_ERR_REJECTED : SH_OK;
}


// the FRI rows of a plan, all rounds in one launch
hipError_t mv_launch_rows(const MvPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, const uint32_t* ys, uint32_t* flags,
                          hipStream_t st) {
  const VbPlan& s = p.shape;
  if (!s.rounds) return hipSuccess;
  MvRowsArgs ra = {};
  uint32_t smax = 0;
  for (uint32_t r = 0; r < s.rounds; ++r) {
    const VbRound& rd = s.r[r];
    ra.r[r] = {p.w[r], p.inv_i[r], rd.roudeg, rd.off, rd.root_off, rd.samples, rd.set_off, rd.l1, rd.l2};
    smax = rd.samples > smax ? rd.samples : smax;
  }
  const uint64_t items = (uint64_t)smax * batch;
  hipLaunchKernelGGL(mv_fri_rows_kernel, dim3((uint32_t)((items + MV_TPB - 1) / MV_TPB), s.rounds), dim3(MV_TPB), 0, st, proofs, s.plen,
                     roots, batch, p.M, ra, ys, s.ys_per_proof, flags);
  return hipGetLastError();
}

// the final layer and the statuses.  The root it must hash to is the last round's root2; without a round the committed root itself:
// l_root (byte 32) of a STARK proof, the caller's root of a FRI proof
hipError_t mv_launch_final(const MvPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, const uint32_t* flags,
                           int32_t* status, hipStream_t st) {
  const VbPlan& s = p.shape;
  MvFinalArgs fa;
  fa.w = p.w_final;
  fa.D = p.D;
  fa.off = s.final_off;
  fa.len = s.final_len;
  fa.k = s.k;
  fa.root_off = s.rounds ? (int64_t)s.r[s.rounds - 1].off : (s.stark ? 32 : -1);
  fa.exclude = s.exclude;
  for (uint32_t i = 0; i < VB_MAX_K; ++i) {
    fa.xk[i] = p.xk[i];
    fa.cof[i] = p.cof[i];
  }
  hipLaunchKernelGGL(mv_final_kernel, dim3(batch), dim3(MV_TPB), (size_t)s.final_len * 32, st, proofs, s.plen, roots, p.M, fa, flags, status);
  return hipGetLastError();
}

}  // namespace

hipError_t shk_mod_verify_batch(const MvPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, uint32_t* ys,
                                uint32_t* flags, int32_t* status, hipStream_t st) {
  hipError_t e = shk_verify_sets_and_branches(p.shape, proofs, batch, roots, ys, flags, st);
  if (e != hipSuccess) return e;
  if ((e = mv_launch_rows(p, proofs, batch, roots, ys, flags, st)) != hipSuccess) return e;
  return mv_launch_final(p, proofs, batch, roots, flags, status, st);
}

// sets + branches -> FRI rows -> spot checks -> final layer and statuses; a STARK proof carries its roots, so `roots` is null
hipError_t shk_mod_verify_stark_batch(const MvPlan& p, const uint8_t* proofs, uint32_t batch, const fpm* inputs, const fpm* outputs,
                                      uint64_t io_stride, const fpm* coef, const uint8_t* exps, uint32_t row, const uint32_t* tbegin,
                                      uint32_t* ys, uint32_t* flags, int32_t* status, hipStream_t st) {
  const VbPlan& s = p.shape;
  hipError_t e = shk_verify_sets_and_branches(s, proofs, batch, nullptr, ys, flags, st);
  if (e != hipSuccess) return e;
  if ((e = mv_launch_rows(p, proofs, batch, nullptr, ys, flags, st)) != hipSuccess) return e;
  MvSpotArgs sa = {};
  sa.sc = p.sc;
  sa.pb = s.pb;
  sa.lb = s.lb;
  sa.io_stride = io_stride;
  sa.samples = s.samples;
  sa.row = row;
  for (uint32_t d = 0; d <= s.width; ++d) sa.tbegin[d] = tbegin[d];
  const uint64_t items = (uint64_t)s.samples * batch;
  hipLaunchKernelGGL(mv_spot_kernel, dim3((uint32_t)((items + 63) / 64)), dim3(64), 0, st, proofs, s.plen, batch, p.M, sa, inputs, outputs,
                     coef, exps, ys, s.ys_per_proof, flags);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return mv_launch_final(p, proofs, batch, nullptr, flags, status, st);
}
