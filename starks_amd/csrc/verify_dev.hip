// verify_dev.hip -- batched device verifiers (sh_dev_stark_verify / sh_dev_fri_verify, include/starkhip.h): every proof of a batch
// checked as sh_stark_verify / sh_fri_verify (verify.hip) checks it, split into independent items (verify_items.cuh):
//   1. index sets      one quad of lanes per (proof, set): the spot positions (entropy l_root) and each FRI round's rows (root2)
//   2. Merkle branches one lane per branch, one launch for all branch classes, blocks of one class (equal chain length and leaf size
//                      across the wave)
//   3. FRI rows        one lane per (proof, round, sample): the cubic through the row at special_x against the column value
//   4. spot checks     one lane per (proof, sample): transition and boundary constraints at x = g2^pos
//   5. final layer     one workgroup per proof: permute4 tree against the last root, then the degree bound over the lanes;
//                      it also writes the statuses (everything before it is ahead of it on the stream)
// A failing item sets its proof's flag; the status is SH_ERR_REJECTED where the flag is set, SH_OK elsewhere.
// No address depends on proof bytes: offsets come from the plan, sampled indices only pick hash order and exponents.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "verify_items.cuh"

namespace {

constexpr uint32_t VB_TPB = 256;

struct VbSets {  // index sets per proof: set 0 = the spot positions (STARK only), then one per FRI round
  uint64_t entropy_off[SHK_FRI_MAX_ROUNDS + 1];  // byte offset of the entropy in a proof
  uint32_t modulus[SHK_FRI_MAX_ROUNDS + 1];
  uint32_t count[SHK_FRI_MAX_ROUNDS + 1];
  uint32_t set_off[SHK_FRI_MAX_ROUNDS + 1];
  uint32_t exclude;
};

// blockIdx.y = set; 16 quads = 16 proofs per block
__global__ void __launch_bounds__(64) vb_indices_kernel(const uint8_t* proofs, uint64_t plen, uint32_t batch, VbSets s, uint32_t ys_per,
                                                        uint32_t* ys) {
  __shared__ __attribute__((aligned(16))) uint32_t slots[16 * 16];
  const uint32_t set = blockIdx.y;
  const uint32_t b = blockIdx.x * 16 + (threadIdx.x >> 2);
  const bool live = b < batch;
  const uint64_t bb = live ? b : 0;
  sample_indices_quad(slots, reinterpret_cast<const uint32_t*>(proofs + bb * plen + s.entropy_off[set]), live, s.modulus[set],
                      s.count[set], s.exclude, ys + bb * ys_per + s.set_off[set]);
}

struct VbClass {  // `reps` x `count` branches per proof of one shape
  uint64_t off;        // byte offset of the first branch in a proof
  uint64_t stride;     // bytes between consecutive samples
  uint64_t rep_stride; // bytes between repetitions (the 2 packed branches of a spot check, the 4 row branches of a FRI sample)
  int64_t root_off;    // byte offset of the root in the proof; -1: the caller's root [batch][32]
  uint32_t count, reps, set_off, add, rep_add, mod, entries, leaf_bytes;
};

constexpr uint32_t VB_MAX_CLASSES = 2 + 2 * SHK_FRI_MAX_ROUNDS;
struct VbClasses {
  VbClass c[VB_MAX_CLASSES];
};
// blockIdx.y = class: every class in one launch, so that the short FRI classes run beside the long spot-check ones; a block never mixes
// classes (equal chain length and leaf size across each wave)
__global__ void __launch_bounds__(VB_TPB) vb_branch_kernel(const uint8_t* proofs, uint64_t plen, const uint8_t* roots, uint32_t batch,
                                                           VbClasses cs, const uint32_t* ys, uint32_t ys_per, uint32_t* flags) {
  const VbClass& c = cs.c[blockIdx.y];
  const uint64_t g = (uint64_t)blockIdx.x * VB_TPB + threadIdx.x;
  const uint32_t per = c.count * c.reps;
  if (g >= (uint64_t)per * batch) return;
  const uint32_t b = (uint32_t)(g / per), r = (uint32_t)(g - (uint64_t)b * per);
  const uint32_t j = r / c.count, i = r - j * c.count;
  const uint8_t* proof = proofs + (uint64_t)b * plen;
  const uint8_t* root = c.root_off < 0 ? roots + 32ull * b : proof + c.root_off;
  const uint64_t index = ((uint64_t)ys[(uint64_t)b * ys_per + c.set_off + i] + c.add + (uint64_t)j * c.rep_add) % c.mod;
  if (!vb_branch(proof + c.off + (uint64_t)i * c.stride + (uint64_t)j * c.rep_stride, root, index, c.entries, c.leaf_bytes))
    flags[b] = 1;
}

struct VbRowsArgs {
  VbRound r[SHK_FRI_MAX_ROUNDS];
};
// blockIdx.y = round
__global__ void __launch_bounds__(VB_TPB) vb_fri_rows_kernel(const uint8_t* proofs, uint64_t plen, const uint8_t* roots, uint32_t batch,
                                                             VbRowsArgs a, const uint32_t* ys, uint32_t ys_per, uint32_t* flags) {
  const VbRound& rd = a.r[blockIdx.y];
  const uint64_t g = (uint64_t)blockIdx.x * VB_TPB + threadIdx.x;
  if (g >= (uint64_t)rd.samples * batch) return;
  const uint32_t b = (uint32_t)(g / rd.samples), i = (uint32_t)(g - (uint64_t)b * rd.samples);
  const uint8_t* proof = proofs + (uint64_t)b * plen;
  const uint8_t* mroot = rd.root_off < 0 ? roots + 32ull * b : proof + rd.root_off;
  const fp special_x = vb_field(mroot);  // field(m[1]) (fri.py:229)
  const uint8_t* sample = proof + rd.off + 32 + (uint64_t)i * 32 * (rd.l2 + 4ull * rd.l1);
  const uint32_t y = ys[(uint64_t)b * ys_per + rd.set_off + i];
  if (!vb_fri_row(sample, rd.l1, rd.l2, rd.w, rd.inv_i, rd.roudeg, y, special_x)) flags[b] = 1;
}

struct VbSpotArgs {
  VbSpotConst sc;
  uint64_t pb, lb, io_stride;
  uint32_t samples, row;
  uint32_t tbegin[SHK_STARK_MAX_WIDTH + 1];
};
__global__ void __launch_bounds__(64) vb_spot_kernel(const uint8_t* proofs, uint64_t plen, uint32_t batch, VbSpotArgs a, const fp* inputs,
                                                     const fp* outputs, const fp* coef, const uint8_t* exps, const uint32_t* ys,
                                                     uint32_t ys_per, uint32_t* flags) {
  const uint64_t g = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= (uint64_t)a.samples * batch) return;
  const uint32_t b = (uint32_t)(g / a.samples), i = (uint32_t)(g - (uint64_t)b * a.samples);
  const uint8_t* b1 = proofs + (uint64_t)b * plen + 64 + (2 * a.pb + a.lb) * i;
  const uint64_t io = (uint64_t)b * a.sc.width * a.io_stride;
  if (!vb_spot(b1, b1 + a.pb, ys[(uint64_t)b * ys_per + i], a.sc, inputs + io, outputs + io, a.io_stride, coef, exps, a.row, a.tbegin))
    flags[b] = 1;
}

struct VbFinalArgs {
  fp w;
  fp xk[VB_MAX_K], inv_den[VB_MAX_K];
  uint64_t off, len, k;
  int64_t root_off;  // the last committed root; -1: the caller's root (no FRI round)
  uint32_t exclude;
};
// one workgroup per proof; dynamic LDS: the tree's nodes [1, len) of 32 bytes (the layout of merkelize, merkle_tree.py:36-56)
__global__ void __launch_bounds__(VB_TPB) vb_final_kernel(const uint8_t* proofs, uint64_t plen, const uint8_t* roots, VbFinalArgs a,
                                                          const uint32_t* flags, int32_t* status) {
  extern __shared__ __attribute__((aligned(16))) uint32_t nodes[];  // [len][8]
  __shared__ fp xk[VB_MAX_K], wgt[VB_MAX_K];
  const uint32_t b = blockIdx.x, tid = threadIdx.x;
  const uint8_t* proof = proofs + (uint64_t)b * plen;
  const uint8_t* data = proof + a.off;
  const uint32_t len = (uint32_t)a.len;
  bool bad = false;
  // nodes [len/2, len) from the permuted leaves (permute4, merkle_tree.py:11-23), then level by level up to the root
  for (uint32_t m = len / 2 + tid; m < len; m += VB_TPB) {
    uint32_t l[8], r[8];
    vb_load8(data + 32 * vb_final_leaf(2 * m - len, len), l);
    vb_load8(data + 32 * vb_final_leaf(2 * m + 1 - len, len), r);
    const b2digest d = b2_hash_pair(l, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) nodes[8 * m + i] = d.h[i];
  }
  for (uint32_t s = len / 2; s > 1; s /= 2) {
    __syncthreads();
    for (uint32_t m = s / 2 + tid; m < s; m += VB_TPB) {
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
    wgt[tid] = vb_final_weight(tid, a.exclude, data, a.inv_den);
  }
  __syncthreads();
  for (uint64_t t = k + tid; t < np; t += VB_TPB)
    if (!vb_final_point(t, k, a.w, a.exclude, data, xk, wgt)) bad = true;
  bad = __syncthreads_or(bad);
  if (tid == 0) status[b] = (bad || flags[b]) ? SH_ERR_REJECTED : SH_OK;
}

}  // namespace

// launches 1 and 2 above (declared in verify_items.cuh)
hipError_t shk_verify_sets_and_branches(const VbPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, uint32_t* ys,
                                        uint32_t* flags, hipStream_t st) {
  hipError_t e = hipMemsetAsync(flags, 0, (size_t)batch * 4, st);
  if (e != hipSuccess) return e;
  const uint64_t plen = p.plen;
  // 1. index sets
  VbSets s = {};
  uint32_t nsets = 0;
  if (p.stark) {
    s.entropy_off[0] = 32;  // l_root
    s.modulus[0] = (uint32_t)p.n;
    s.count[0] = p.samples;
    s.set_off[0] = 0;
    nsets = 1;
  }
  for (uint32_t r = 0; r < p.rounds; ++r, ++nsets) {
    s.entropy_off[nsets] = p.r[r].off;  // root2
    s.modulus[nsets] = (uint32_t)(p.r[r].roudeg / 4);
    s.count[nsets] = p.r[r].samples;
    s.set_off[nsets] = p.r[r].set_off;
  }
  s.exclude = p.exclude;  // the spot positions exclude multiples of ext = the FRI proof's exclude
  if (nsets) {
    hipLaunchKernelGGL(vb_indices_kernel, dim3((batch + 15) / 16, nsets), dim3(64), 0, st, proofs, plen, batch, s, p.ys_per_proof, ys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  // 2. Merkle branches, all classes in one launch
  VbClasses cs;
  uint32_t ncls = 0;
  if (p.stark) {
    const uint64_t per = 2 * p.pb + p.lb;
    const uint32_t entries = p.lg + 1;
    // the two packed branches of position pos and (pos + ext) % n against m_root; then the l branch against l_root
    cs.c[ncls++] = {64, per, p.pb, 0, p.samples, 2, 0, 0, p.ext, (uint32_t)p.n, entries, 96 * p.width};
    cs.c[ncls++] = {64 + 2 * p.pb, per, 0, 32, p.samples, 1, 0, 0, 0, (uint32_t)p.n, entries, 32};
  }
  for (uint32_t r = 0; r < p.rounds; ++r) {
    const VbRound& rd = p.r[r];
    const uint64_t per = 32ull * (rd.l2 + 4ull * rd.l1);
    const uint32_t q = (uint32_t)(rd.roudeg / 4);
    // the column branch (y against root2), then the 4 row branches (y + j n_r / 4 against the round's committed root)
    cs.c[ncls++] = {rd.off + 32, per, 0, (int64_t)rd.off, rd.samples, 1, rd.set_off, 0, 0, q, rd.l2, 32};
    cs.c[ncls++] = {rd.off + 32 + 32ull * rd.l2, per, 32ull * rd.l1, rd.root_off, rd.samples, 4, rd.set_off, 0, q, (uint32_t)rd.roudeg,
                    rd.l1, 32};
  }
  uint64_t most = 0;
  for (uint32_t i = 0; i < ncls; ++i) {
    const uint64_t items = (uint64_t)cs.c[i].count * cs.c[i].reps * batch;
    most = items > most ? items : most;
  }
  if (most) {
    hipLaunchKernelGGL(vb_branch_kernel, dim3((uint32_t)((most + VB_TPB - 1) / VB_TPB), ncls), dim3(VB_TPB), 0, st, proofs, plen, roots, batch,
                       cs, ys, p.ys_per_proof, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// Launch the whole verification of `batch` proofs of plan p.  ys / flags: device scratch of batch * p.ys_per_proof and batch u32
// (flags zeroed here).  STARK only: inputs / outputs limb form (element (b, d) at (b width + d) io_stride), coef / exps / tbegin = the
// step polynomials (exponent rows of `row` bytes).  FRI only: roots [batch][32] = the committed roots.
hipError_t shk_verify_batch(const VbPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, const fp* inputs,
                            const fp* outputs, uint64_t io_stride, const fp* coef, const uint8_t* exps, uint32_t row,
                            const uint32_t* tbegin, uint32_t* ys, uint32_t* flags, int32_t* status, hipStream_t st) {
  hipError_t e = shk_verify_sets_and_branches(p, proofs, batch, roots, ys, flags, st);
  if (e != hipSuccess) return e;
  const uint64_t plen = p.plen;
  // 3. FRI rows
  if (p.rounds) {
    VbRowsArgs ra;
    uint32_t smax = 0;
    for (uint32_t r = 0; r < p.rounds; ++r) {
      ra.r[r] = p.r[r];
      smax = p.r[r].samples > smax ? p.r[r].samples : smax;
    }
    const uint64_t items = (uint64_t)smax * batch;
    hipLaunchKernelGGL(vb_fri_rows_kernel, dim3((uint32_t)((items + VB_TPB - 1) / VB_TPB), p.rounds), dim3(VB_TPB), 0, st, proofs, plen,
                       roots, batch, ra, ys, p.ys_per_proof, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  // 4. spot checks
  if (p.stark) {
    VbSpotArgs sa = {};
    sa.sc = p.sc;
    sa.pb = p.pb;
    sa.lb = p.lb;
    sa.io_stride = io_stride;
    sa.samples = p.samples;
    sa.row = row;
    for (uint32_t d = 0; d <= p.width; ++d) sa.tbegin[d] = tbegin[d];
    const uint64_t items = (uint64_t)p.samples * batch;
    hipLaunchKernelGGL(vb_spot_kernel, dim3((uint32_t)((items + 63) / 64)), dim3(64), 0, st, proofs, plen, batch, sa, inputs, outputs,
                       coef, exps, ys, p.ys_per_proof, flags);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  // 5. final layer and statuses
  VbFinalArgs fa;
  fa.w = p.w_final;
  fa.off = p.final_off;
  fa.len = p.final_len;
  fa.k = p.k;
  fa.root_off = p.rounds ? (int64_t)p.r[p.rounds - 1].off : (p.stark ? 32 : -1);
  fa.exclude = p.exclude;
  for (uint32_t i = 0; i < VB_MAX_K; ++i) {
    fa.xk[i] = p.xk[i];
    fa.inv_den[i] = p.inv_den[i];
  }
  hipLaunchKernelGGL(vb_final_kernel, dim3(batch), dim3(VB_TPB), (size_t)p.final_len * 32, st, proofs, plen, roots, fa, flags, status);
  return hipGetLastError();
}
