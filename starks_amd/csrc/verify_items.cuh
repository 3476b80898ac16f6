// verify_items.cuh -- the per-item checks of the batched device verifiers (verify_dev.hip) and the host plan they run by.
//
// sh_stark_verify / sh_fri_verify (verify.hip) walk one proof serially.  The batch verifiers split the same checks into independent
// items -- index sets, Merkle branches, FRI rows, STARK spot checks, the final layer -- and OR the failures per proof.  Every item
// function here is __host__ __device__, so tests/native/verify_batch_host.cpp runs the same decomposition on the CPU and compares each
// decision with the host verifier's.  verify.hip shares none of this code: it stays the independent yardstick.
//
// Addressing rule: with one shape per call, every byte offset is a function of (shape, proof, item) alone.  Values read from a proof
// (sampled indices, field elements) only choose hash order and exponents, so a hostile proof cannot move a read outside its own bytes.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/starkhip.h"
#include "blake2s.cuh"
#include "fp256.cuh"
#include "internal.hpp"  // SHK_FRI_MAX_ROUNDS, SHK_STARK_MAX_WIDTH, SHK_STARK_MAX_TERMS

#define VB_HD __host__ __device__ __forceinline__

constexpr uint64_t VB_MAX_FINAL = 1u << 10;  // largest final FRI layer a batch verifier takes (one workgroup per proof, its tree in LDS)
constexpr uint64_t VB_MAX_K = 16;            // the final layer's degree bound: the round loop runs while maxdeg_plus_1 > 16

// ---- reading a proof ----------------------------------------------------------------------------------------------------------
VB_HD void vb_load8(const uint8_t* p, uint32_t w[8]) {  // 32 bytes, 4-byte aligned
  const uint32_t* s = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = s[i];
}
VB_HD fp vb_field(const uint8_t* p) {  // int.from_bytes(b, 'big') % p
  uint32_t w[8];
  vb_load8(p, w);
  return fp_canon(fp_from_wire_words(w));
}
VB_HD bool vb_eq(const fp& a, const fp& b) { return fp_eq_canon(fp_canon(a), fp_canon(b)); }

// BLAKE2s of A || B, A and B `len` bytes each (len a multiple of 32: a packed leaf and its sibling, or two 32-byte nodes)
VB_HD void vb_hash_two(const uint8_t* a, const uint8_t* b, uint32_t len, uint32_t h[8]) {
  const uint32_t half = len / 32, blocks = len / 32;  // 2 len bytes = len / 32 blocks of 64
  b2_init(h);
#pragma unroll 1
  for (uint32_t blk = 0; blk < blocks; ++blk) {
    uint32_t m[16];
    const uint32_t c0 = 2 * blk, c1 = 2 * blk + 1;
    vb_load8(c0 < half ? a + 32 * c0 : b + 32 * (c0 - half), m);
    vb_load8(c1 < half ? a + 32 * c1 : b + 32 * (c1 - half), m + 8);
    b2_compress(h, m, 64 * (blk + 1), blk + 1 == blocks);
  }
}

// ---- verify_branch (merkle_tree.py:71-86) --------------------------------------------------------------------------------------
// proof = leaf (leaf_bytes) | sibling (leaf_bytes) | entries - 2 nodes of 32 bytes; leaf_bytes = 32 for a plain tree, 32 k for a
// packed one.  `index` only picks the hash order.
VB_HD bool vb_branch(const uint8_t* proof, const uint8_t* root, uint64_t index, uint32_t entries, uint32_t leaf_bytes) {
  if (entries < 2) return false;
  const uint64_t half = 1ull << (entries - 1);
  const uint64_t q = half / 4;
  if (q == 0 || index >= half) return false;
  uint64_t idx = index / q + 4 * (index % q) + half;  // get_index_in_permuted + half
  uint32_t h[8];
  if (idx & 1)
    vb_hash_two(proof + leaf_bytes, proof, leaf_bytes, h);
  else
    vb_hash_two(proof, proof + leaf_bytes, leaf_bytes, h);
  idx >>= 1;
  const uint8_t* node = proof + 2 * leaf_bytes;
#pragma unroll 1
  for (uint32_t e = 2; e < entries; ++e, node += 32, idx >>= 1) {
    uint32_t m[16], s[8];
    vb_load8(node, s);
    const bool right = idx & 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      m[i] = right ? s[i] : h[i];
      m[8 + i] = right ? h[i] : s[i];
    }
    b2_init(h);
    b2_compress(h, m, 64, true);
  }
  uint32_t r[8];
  vb_load8(root, r);
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) ok = ok && h[i] == r[i];
  return ok;
}

// ---- one sampled FRI row (fri.py:318-337) -----------------------------------------------------------------------------------------
// sample = column branch (l2 entries) | 4 row branches (l1 entries each); the column value must be the value at special_x of the
// cubic through (w^(y + j n/4), row[j]), in the closed form of kernels.hip:fri_fold_row
VB_HD bool vb_fri_row(const uint8_t* sample, uint32_t l1, uint32_t l2, const fp& w, const fp& inv_i, uint64_t roudeg, uint64_t y,
                      const fp& special_x) {
  const uint8_t* rows = sample + 32ull * l2;
  const fp r0 = vb_field(rows), r1 = vb_field(rows + 32ull * l1), r2 = vb_field(rows + 64ull * l1), r3 = vb_field(rows + 96ull * l1);
  const fp colval = vb_field(sample);
  const fp x1_inv = fp_pow_u64(w, (roudeg - y % roudeg) % roudeg);  // w^-y
  const fp t = fp_mul(special_x, x1_inv);
  const fp u0 = fp_add(r0, r2), u1 = fp_sub(r0, r2), u2 = fp_add(r1, r3);
  const fp u3 = fp_mul(fp_sub(r1, r3), inv_i);
  const fp G0 = fp_add(u0, u2), G2 = fp_sub(u0, u2), G1 = fp_add(u1, u3), G3 = fp_sub(u1, u3);
  fp acc = fp_add(fp_mul(G3, t), G2);
  acc = fp_add(fp_mul(acc, t), G1);
  acc = fp_add(fp_mul(acc, t), G0);
  return vb_eq(fp_div4(acc), colval);
}

// ---- one STARK spot check (stark.py:355-374) ---------------------------------------------------------------------------------------
struct VbSpotConst {
  fp g2, last, inv_last_m1;
  uint64_t steps;
  uint32_t width;
};
// b1 / b2 = the two packed branches of the sample (leaf = P | D | B of the position, resp. of its g1 successor); in / out = the boundary
// values (limb form, element d at d * io_stride); terms: coef[t] (limb form), exps rows of `row` bytes, dimension d owns
// [tbegin[d], tbegin[d + 1]).  Reads field values from memory where it needs them: no per-dimension register arrays.
VB_HD bool vb_spot(const uint8_t* b1, const uint8_t* b2, uint64_t pos, const VbSpotConst& c, const fp* in, const fp* out,
                   uint64_t io_stride, const fp* coef, const uint8_t* exps, uint32_t row, const uint32_t* tbegin) {
  const uint32_t W = c.width;
  const fp x = fp_pow_u64(c.g2, pos);
  const fp xm = fp_sub(x, c.last);
  if (vb_eq(xm, fp_zero())) return false;  // the sampling excludes the trace points; a proof that lands there is malformed
  // P(g1 x) - step(P(x)) = Z(x) D(x), Z(x) = (x^steps - 1) / (x - x_last), is checked multiplied through by x - x_last != 0: the
  // same decision without an inversion per lane
  const fp zn = fp_sub(fp_pow_u64(x, c.steps), fp_one());
  const fp z2 = fp_mul(fp_sub(x, fp_one()), xm);
  bool ok = true;
#pragma unroll 1
  for (uint32_t d = 0; d < W; ++d) {
    fp acc = fp_zero();
#pragma unroll 1
    for (uint32_t t = tbegin[d]; t < tbegin[d + 1]; ++t) {
      fp prod = fp_canon(coef[t]);
#pragma unroll 1
      for (uint32_t v = 0; v < W; ++v) {
        const uint32_t e = exps[(uint64_t)t * row + v];
        if (!e) continue;
        const fp pv = vb_field(b1 + 32ull * v);
#pragma unroll 1
        for (uint32_t k = 0; k < e; ++k) prod = fp_mul(prod, pv);
      }
      acc = fp_add(acc, prod);
    }
    const fp pg = vb_field(b2 + 32ull * d), dx = vb_field(b1 + 32ull * (W + d));
    ok = ok && vb_eq(fp_mul(fp_sub(pg, acc), xm), fp_mul(zn, dx));
    const fp px = vb_field(b1 + 32ull * d), bx = vb_field(b1 + 32ull * (2 * W + d));
    const fp iv = fp_canon(in[d * io_stride]), ov = fp_canon(out[d * io_stride]);
    const fp slope = fp_mul(fp_sub(ov, iv), c.inv_last_m1);
    const fp interp = fp_add(fp_sub(iv, slope), fp_mul(slope, x));
    ok = ok && vb_eq(fp_sub(px, fp_mul(bx, z2)), interp);
  }
  return ok;
}

// ---- the final layer (fri.py:340-366) ----------------------------------------------------------------------------------------------
// leaf t of the permute4 tree over `len` values holds value (t % 4) len/4 + t / 4
VB_HD uint64_t vb_final_leaf(uint64_t t, uint64_t len) { return (t & 3) * (len >> 2) + (t >> 2); }
// the retained points: x in [0, len) with x % exclude != 0 (every x when exclude == 0, none when exclude == 1)
VB_HD uint64_t vb_npts(uint64_t len, uint32_t exclude) { return exclude ? len - (len + exclude - 1) / exclude : len; }
VB_HD uint64_t vb_pt(uint64_t t, uint32_t exclude) { return exclude ? t + 1 + t / (exclude - 1) : t; }
// barycentric weight of retained point a < k: val / prod_{b != a} (x_a - x_b), x_i = w^pts[i]; the inverted products depend on the
// shape alone (VbPlan::inv_den)
VB_HD fp vb_final_weight(uint64_t a, uint32_t exclude, const uint8_t* data, const fp* inv_den) {
  return fp_mul(vb_field(data + 32 * vb_pt(a, exclude)), inv_den[a]);
}
// retained point t >= k lies on the interpolant through the first k (xk[b] = x of retained point b, wgt = vb_final_weight)
VB_HD bool vb_final_point(uint64_t t, uint64_t k, const fp& w, uint32_t exclude, const uint8_t* data, const fp* xk, const fp* wgt) {
  const uint64_t pt = vb_pt(t, exclude);
  const fp x = fp_pow_u64(w, pt);
  fp total = fp_zero();
#pragma unroll 1
  for (uint64_t a = 0; a < k; ++a) {
    fp num = wgt[a];
#pragma unroll 1
    for (uint64_t b = 0; b < k; ++b)
      if (b != a) num = fp_mul(num, fp_sub(x, xk[b]));
    total = fp_add(total, num);
  }
  return vb_eq(total, vb_field(data + 32 * pt));
}

// ---- the plan: every offset of one proof shape, decided on the host before anything is launched ---------------------------------
struct VbRound {
  fp w, inv_i;           // generator of the round's domain; I^-1 = w^(3 n_r / 4)
  uint64_t roudeg;       // n_r
  uint64_t off;          // byte offset of the round's root2 in a proof; the samples follow it
  int64_t root_off;      // byte offset of the round's committed root (special_x, row branches); -1: the caller's root [batch][32]
  uint32_t samples, set_off, l1, l2;
};
struct VbPlan {
  uint32_t stark;        // 1: a STARK proof (spot checks, then the FRI proof of l at fri_off), 0: a FRI proof
  uint64_t plen;         // bytes per proof
  uint32_t exclude;      // exclude_multiples_of of the index sets of every FRI round and of the final layer
  // STARK spot checks
  uint64_t steps, n;
  uint32_t ext, width, samples, lg;
  uint64_t pb, lb;       // bytes of a packed branch, of the l branch
  VbSpotConst sc;
  // FRI rounds
  uint32_t rounds;
  VbRound r[SHK_FRI_MAX_ROUNDS];
  uint64_t final_off, final_len, k;
  fp w_final;
  fp xk[VB_MAX_K];       // x of the first k retained points of the final layer
  fp inv_den[VB_MAX_K];  // 1 / prod_{b != a} (xk[a] - xk[b])
  uint32_t ys_per_proof;  // sampled indices per proof: set 0 = the spot positions (STARK), then one set per round
};

inline uint32_t vb_ilog2(uint64_t n) {
  uint32_t k = 0;
  while ((1ull << k) < n) ++k;
  return k;
}
inline fp vb_root_pow2(uint32_t lg) {  // 7^((p - 1) / 2^lg), the generator the prover takes (stark.py:246)
  const uint32_t pm1[8] = {0u, 0xfffffea1u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  fp r = fp_one(), b = fp_from_u32(7u);
  for (uint32_t i = lg; i < 256; ++i) {  // bit i of p - 1 is bit i - lg of the exponent
    if ((pm1[i / 32] >> (i % 32)) & 1) r = fp_mul(r, b);
    b = fp_sqr(b);
  }
  return r;
}
inline fp vb_wire(const uint8_t b[32]) {
  uint32_t w[8];
  memcpy(w, b, 32);
  return fp_canon(fp_from_wire_words(w));
}

// The FRI part of a plan (fri.py:268-366 on the flat layout from byte `off`, round-0 root at root_off).  Returns what the host
// verifier returns for a proof of this shape that passes every check (SH_OK, or SH_ERR_INVALID), or SH_ERR_UNSUPPORTED for a final
// layer over VB_MAX_FINAL.
inline int vb_plan_fri(VbPlan* p, uint64_t off, int64_t root_off, uint64_t n, const fp& root, uint64_t md, uint32_t exclude,
                       uint32_t samples, uint32_t set_off) {
  fp w = root;
  uint64_t roudeg = n;
  bool first = true;
  p->rounds = 0;
  p->exclude = exclude;
  while (md > 16) {
    if (roudeg < 16) return SH_ERR_INVALID;
    if (p->rounds == SHK_FRI_MAX_ROUNDS) return SH_ERR_UNSUPPORTED;  // (unreachable: the sampling below refuses n_r / 4 >= 2^24 first)
    const uint32_t s = first ? samples : 40;
    const uint64_t q = roudeg / 4;
    if (q >= (1ull << 24) || exclude == 1) return SH_ERR_INVALID;  // get_pseudorandom_indices asserts / divides by zero
    if ((exclude ? q * (exclude - 1) / exclude : q) == 0) return SH_ERR_INVALID;
    VbRound& r = p->r[p->rounds++];
    r.w = w;
    r.inv_i = fp_pow_u64(w, 3 * q);
    r.roudeg = roudeg;
    r.off = off;
    r.root_off = root_off;
    r.samples = s;
    r.set_off = set_off;
    const uint32_t lg = vb_ilog2(roudeg);
    r.l1 = lg + 1;
    r.l2 = lg - 1;
    set_off += s;
    root_off = (int64_t)off;  // the next round's committed root is this round's root2
    off += 32 + (uint64_t)s * 32 * (r.l2 + 4ull * r.l1);
    w = fp_pow_u64(w, 4);
    md /= 4;
    roudeg /= 4;
    first = false;
  }
  if (roudeg < 4) return SH_ERR_INVALID;
  if (roudeg > VB_MAX_FINAL) return SH_ERR_UNSUPPORTED;
  p->final_off = off;
  p->final_len = roudeg;
  const uint64_t np = vb_npts(roudeg, exclude);
  p->k = md < np ? md : np;
  p->w_final = w;
  // the barycentric denominators, inverted together (one inversion: prefix products)
  fp den[VB_MAX_K], pre[VB_MAX_K + 1];
  pre[0] = fp_one();
  for (uint64_t a = 0; a < p->k; ++a) p->xk[a] = fp_pow_u64(w, vb_pt(a, exclude));
  for (uint64_t a = 0; a < p->k; ++a) {
    den[a] = fp_one();
    for (uint64_t b = 0; b < p->k; ++b)
      if (b != a) den[a] = fp_mul(den[a], fp_sub(p->xk[a], p->xk[b]));
    pre[a + 1] = fp_mul(pre[a], den[a]);
  }
  fp inv = fp_inv(pre[p->k]);
  for (uint64_t a = p->k; a-- > 0;) {
    p->inv_den[a] = fp_canon(fp_mul(inv, pre[a]));
    inv = fp_mul(inv, den[a]);
  }
  p->plen = off + 32 * roudeg;
  p->ys_per_proof = set_off;
  return SH_OK;
}

// sh_fri_verify's verdict on the shape, then the plan
inline int vb_plan_fri_proof(VbPlan* p, uint64_t n, const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples) {
  memset(p, 0, sizeof *p);
  if (!root || n < 4 || (n & (n - 1)) || samples == 0) return SH_ERR_INVALID;
  if (n > (1ull << 32)) return SH_ERR_UNSUPPORTED;
  const fp w = vb_wire(root);
  if (!vb_eq(fp_pow_u64(w, n / 2), fp_neg(fp_one()))) return SH_ERR_ROOT_ORDER;
  return vb_plan_fri(p, 0, -1, n, w, maxdeg_plus_1, exclude, samples, 0);
}

// sh_stark_verify's verdict on the shape, then the plan
inline int vb_plan_stark_proof(VbPlan* p, uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* term_exps,
                               const uint32_t* term_counts, uint32_t samples) {
  memset(p, 0, sizeof *p);
  if (!term_exps || !term_counts || width == 0 || samples == 0) return SH_ERR_INVALID;
  if (steps < 2 || (steps & (steps - 1)) || ext < 2 || (ext & (ext - 1))) return SH_ERR_INVALID;
  if (steps >= (1ull << 24) || ext >= (1u << 24) || steps * ext >= (1ull << 24)) return SH_ERR_INVALID;
  if (width > SHK_STARK_MAX_WIDTH) return SH_ERR_UNSUPPORTED;
  uint64_t total = 0;
  for (uint32_t d = 0; d < width; ++d) {
    if (term_counts[d] > SHK_STARK_MAX_TERMS) return SH_ERR_UNSUPPORTED;
    total += term_counts[d];
  }
  if (total == 0 || total > SHK_STARK_MAX_TERMS) return total ? SH_ERR_UNSUPPORTED : SH_ERR_INVALID;
  uint32_t degree = 0;
  for (uint64_t t = 0; t < total; ++t) {
    uint32_t sum = 0;
    for (uint32_t v = 0; v < width; ++v) sum += term_exps[t * width + v];
    if (sum > degree) degree = sum;
  }
  const uint64_t n = steps * ext;
  const uint32_t lg = vb_ilog2(n), k = 3 * width;
  p->stark = 1;
  p->steps = steps;
  p->n = n;
  p->ext = ext;
  p->width = width;
  p->samples = samples;
  p->lg = lg;
  p->pb = 32ull * (2 * k + (lg - 1));
  p->lb = 32ull * (lg + 1);
  const fp g2 = vb_root_pow2(lg);
  p->sc.g2 = g2;
  p->sc.last = fp_pow_u64(g2, (steps - 1) * ext);
  p->sc.inv_last_m1 = fp_inv(fp_sub(p->sc.last, fp_one()));
  p->sc.steps = steps;
  p->sc.width = width;
  const uint64_t fri_off = 64 + (2 * p->pb + p->lb) * samples;
  const int rc = vb_plan_fri(p, fri_off, 32, n, g2, steps * (uint64_t)degree, ext, 40, samples);
  p->stark = 1;
  return rc;
}

// verify_dev.hip: the field-free head of a batch verification -- zero the flags, draw every index set, check every Merkle branch.  It
// reads the plan's offsets and counts alone; the verifier over another modulus (modverify_dev.hip) starts with it too.
hipError_t shk_verify_sets_and_branches(const VbPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, uint32_t* ys,
                                        uint32_t* flags, hipStream_t st);
