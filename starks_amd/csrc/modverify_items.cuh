// modverify_items.cuh -- the per-item checks of the batched FRI verifier over any odd modulus below 2^256 (modverify_dev.hip) and the
// host plan they run by: verify_items.cuh's decomposition on the run-time-modulus arithmetic of fpm.cuh.
//
// The field-free pieces are verify_items.cuh's own -- vb_branch, vb_hash_two, vb_final_leaf, vb_npts, vb_pt, the index sampler -- and
// every byte offset of a shape sits in a VbPlan (MvPlan::shape: its fp fields stay zero), so the index-set and branch kernels of
// verify_dev.hip run as they are.  What depends on the field is here: the row item, the two final-layer items and the plan's
// constants.  Everything is __host__ __device__: tests/native/modverify_host.cpp walks the same items on the CPU over the same plan
// and compares every decision with the host verifier's (modverify.hip), which shares none of this code.
//
// Forms.  A value read from a proof is any 256-bit number and is taken modulo p (mv_field: plain, canonical).  The plan's constants --
// generators, I^-1, the final layer's x_k, cofactors and D -- are in Montgomery form, so fpm_mul(plain, constant) is plain and
// canonical and two canonical plain values compare limb for limb.
//
// NO INVERSION, anywhere: p may be composite (root^(n/2) = -1 is all that is asked of it), where x^(p-2) is not an inverse.
//   row          the closed form of mf_fold_row / vb_fri_row: I^-1 = w^(3 n/4), the 1/4 is two halvings (p is odd).
//   final layer  the interpolant through the first k retained points, cross-multiplied.  With den_a = prod_{b != a} (x_a - x_b),
//                D = prod_a den_a and cof_a = D / den_a = prod_{c != a} den_c (a product, not a quotient), point t passes when
//                    sum_a data_a cof_a prod_{b != a} (x_t - x_b) == data_t D.
//                root^(n/2) = -1 modulo an odd p gives w order n modulo every prime factor of p, so every w^d - 1, 0 < d < n, and with
//                them every den_a and D are units: the check is the reference's data_t == sum_a data_a / den_a prod (x_t - x_b)
//                multiplied through by a unit, the same decision for every proof.
//
// Addressing rule (verify_items.cuh): every byte offset is a function of (shape, proof, item) alone; what is read from a proof only
// chooses hash order and exponents.
#pragma once
#include "fpm.cuh"
#include "modfri_items.cuh"  // mf_half
#include "verify_items.cuh"

#define MV_HD __host__ __device__ __forceinline__

// int.from_bytes(b, 'big') % p of 32 proof bytes (4-byte aligned): plain, canonical
MV_HD fpm mv_field(const uint8_t* b, const fpm_mod& M) {
  uint32_t w[8];
  vb_load8(b, w);
  return fpm_canon(fpm_from_wire_words(w), M);
}
// the same in Montgomery form (one product: fpm_to_mont takes any 256-bit value)
MV_HD fpm mv_field_mont(const uint8_t* b, const fpm_mod& M) {
  uint32_t w[8];
  vb_load8(b, w);
  return fpm_to_mont(fpm_from_wire_words(w), M);
}

// ---- one sampled FRI row (fri.py:318-337) -----------------------------------------------------------------------------------------
// sample = column branch (l2 entries) | 4 row branches (l1 entries each); w, inv_i and sx_mont = field(merkle_root) in Montgomery form
MV_HD bool mv_fri_row(const uint8_t* sample, uint32_t l1, uint32_t l2, const fpm& w, const fpm& inv_i, uint64_t roudeg, uint64_t y,
                      const fpm& sx_mont, const fpm_mod& M) {
  const uint8_t* rows = sample + 32ull * l2;
  const fpm r0 = mv_field(rows, M), r1 = mv_field(rows + 32ull * l1, M), r2 = mv_field(rows + 64ull * l1, M),
            r3 = mv_field(rows + 96ull * l1, M);
  const fpm colval = mv_field(sample, M);
  const fpm t = fpm_mul(sx_mont, fpm_pow(w, (roudeg - y % roudeg) % roudeg, M), M);  // x* w^-y, Montgomery form
  const fpm u0 = fpm_add(r0, r2, M), u1 = fpm_sub(r0, r2, M), u2 = fpm_add(r1, r3, M);
  const fpm u3 = fpm_mul(fpm_sub(r1, r3, M), inv_i, M);
  const fpm G0 = fpm_add(u0, u2, M), G2 = fpm_sub(u0, u2, M), G1 = fpm_add(u1, u3, M), G3 = fpm_sub(u1, u3, M);
  fpm acc = fpm_add(fpm_mul(G3, t, M), G2, M);
  acc = fpm_add(fpm_mul(acc, t, M), G1, M);
  acc = fpm_add(fpm_mul(acc, t, M), G0, M);
  return fpm_eq(mf_half(mf_half(acc, M), M), colval);
}

// ---- the final layer (fri.py:340-366), cross-multiplied -----------------------------------------------------------------------------
// data_a D / den_a of retained point a < k (plain)
MV_HD fpm mv_final_weight(uint64_t a, uint32_t exclude, const uint8_t* data, const fpm* cof, const fpm_mod& M) {
  return fpm_mul(mv_field(data + 32 * vb_pt(a, exclude), M), cof[a], M);
}
// retained point t >= k lies on the interpolant through the first k (xk[b] = x of retained point b, Montgomery form; wgt = the weights)
MV_HD bool mv_final_point(uint64_t t, uint64_t k, const fpm& w, uint32_t exclude, const uint8_t* data, const fpm* xk, const fpm* wgt,
                          const fpm& D, const fpm_mod& M) {
  const uint64_t pt = vb_pt(t, exclude);
  const fpm x = fpm_pow(w, pt, M);
  fpm total = fpm_zero();
#pragma unroll 1
  for (uint64_t a = 0; a < k; ++a) {
    fpm num = wgt[a];
#pragma unroll 1
    for (uint64_t b = 0; b < k; ++b)
      if (b != a) num = fpm_mul(num, fpm_sub(x, xk[b], M), M);
    total = fpm_add(total, num, M);
  }
  return fpm_eq(total, fpm_mul(mv_field(data + 32 * pt, M), D, M));
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------
struct MvPlan {
  fpm_mod M;
  VbPlan shape;  // every offset and count of the shape (stark = 0); its field constants are not used
  fpm w[SHK_FRI_MAX_ROUNDS], inv_i[SHK_FRI_MAX_ROUNDS];  // per round: the domain's generator and I^-1 = w^(3 n_r / 4), Montgomery form
  fpm w_final;         // generator of the final layer's domain, Montgomery form
  fpm xk[VB_MAX_K];    // x of the first k retained points of the final layer, Montgomery form
  fpm cof[VB_MAX_K];   // prod_{c != a} den_c, Montgomery form
  fpm D;               // prod_a den_a, Montgomery form
};

constexpr uint64_t MV_MAX_N = 1ull << 26;  // as sh_mod_fri_prove (MN_MAX_LOG_N)

// sh_mod_fri_verify's verdict on the shape -- what it returns for a proof of that shape that passes every check -- then the plan;
// SH_ERR_UNSUPPORTED for a final layer over VB_MAX_FINAL.  `why` receives the reason of a refusal.
inline int mv_plan_fri_proof(MvPlan* p, const uint8_t modulus[32], uint64_t n, const uint8_t root[32], uint64_t md, uint32_t exclude,
                             uint32_t samples, const char** why) {
  memset(p, 0, sizeof *p);
  *why = "null pointer";
  if (!modulus || !root) return SH_ERR_INVALID;
  *why = "the modulus must be odd and at least 3";
  if (!fpm_mod_init(modulus, &p->M)) return SH_ERR_INVALID;
  const fpm_mod& M = p->M;
  *why = "n must be a power of two and at least 4";
  if (n < 4 || (n & (n - 1))) return SH_ERR_INVALID;
  *why = "samples must be at least 1";
  if (samples == 0) return SH_ERR_INVALID;
  *why = "n is limited to 2^26";
  if (n > MV_MAX_N) return SH_ERR_UNSUPPORTED;
  const fpm wp = fpm_from_wire_bytes(root);
  *why = "root is not below the modulus";
  if (!fpm_below_p(wp, M)) return SH_ERR_ROOT_ORDER;
  fpm w = fpm_to_mont(wp, M);
  *why = "root does not have order n in this ring (root^(n/2) != -1)";
  if (!fpm_eq(fpm_pow(w, n / 2, M), fpm_neg(fpm_from_words(M.one), M))) return SH_ERR_ROOT_ORDER;
  VbPlan& s = p->shape;
  s.exclude = exclude;
  uint64_t roudeg = n, off = 0, set_off = 0;
  int64_t root_off = -1;
  bool first = true;
  while (md > 16) {
    *why = "a round with fewer than 16 points (maxdeg_plus_1 is too large for n)";
    if (roudeg < 16) return SH_ERR_INVALID;
    const uint32_t smp = first ? samples : 40;
    const uint64_t q = roudeg / 4;
    *why = "a column of 2^24 rows or more cannot be sampled (utils.py:69)";
    if (q >= (1ull << 24)) return SH_ERR_INVALID;  // n = 2^26 with a round: the host verifier's sampler refuses it with this code
    *why = "exclude_multiples_of = 1 divides by zero in the reference (utils.py:90)";
    if (exclude == 1) return SH_ERR_INVALID;
    *why = "exclude_multiples_of leaves no row to sample";
    if ((exclude ? q * (exclude - 1) / exclude : q) == 0) return SH_ERR_INVALID;
    *why = "more sampled rows per proof than the index sets hold (2^32)";
    if (set_off + smp > 0xffffffffull) return SH_ERR_UNSUPPORTED;
    // (q < 2^24 and 16 points or more per round: at most SHK_FRI_MAX_ROUNDS rounds)
    const uint32_t r = s.rounds++;
    p->w[r] = w;
    p->inv_i[r] = fpm_pow(w, 3 * q, M);
    VbRound& rd = s.r[r];
    rd.roudeg = roudeg;
    rd.off = off;
    rd.root_off = root_off;
    rd.samples = smp;
    rd.set_off = (uint32_t)set_off;
    const uint32_t lg = vb_ilog2(roudeg);
    rd.l1 = lg + 1;
    rd.l2 = lg - 1;
    set_off += smp;
    root_off = (int64_t)off;  // the next round's committed root is this round's root2
    off += 32 + (uint64_t)smp * 32 * (rd.l2 + 4ull * rd.l1);
    w = fpm_pow(w, 4, M);
    md /= 4;
    roudeg /= 4;
    first = false;
  }
  // (roudeg >= 4 here: n >= 4 without a round, and a round keeps a quarter of 16 points or more)
  *why = "the batch verifiers take a final layer of at most 2^10 points";
  if (roudeg > VB_MAX_FINAL) return SH_ERR_UNSUPPORTED;
  s.final_off = off;
  s.final_len = roudeg;
  const uint64_t np = vb_npts(roudeg, exclude);
  const uint64_t k = md < np ? md : np;
  s.k = k;
  s.plen = off + 32 * roudeg;
  s.ys_per_proof = (uint32_t)set_off;
  p->w_final = w;
  fpm den[VB_MAX_K];
  const fpm one = fpm_from_words(M.one);
  for (uint64_t a = 0; a < k; ++a) p->xk[a] = fpm_pow(w, vb_pt(a, exclude), M);
  p->D = one;
  for (uint64_t a = 0; a < k; ++a) {
    den[a] = one;
    for (uint64_t b = 0; b < k; ++b)
      if (b != a) den[a] = fpm_mul(den[a], fpm_sub(p->xk[a], p->xk[b], M), M);
    p->D = fpm_mul(p->D, den[a], M);
  }
  for (uint64_t a = 0; a < k; ++a) {
    p->cof[a] = one;
    for (uint64_t c = 0; c < k; ++c)
      if (c != a) p->cof[a] = fpm_mul(p->cof[a], den[c], M);
  }
  *why = "";
  return SH_OK;
}

// modverify_dev.hip: launch the whole verification of `batch` proofs of plan p.  ys / flags: device scratch of batch *
// p.shape.ys_per_proof and batch u32 (flags zeroed here); roots [batch][32] = the committed roots.
hipError_t shk_mod_verify_batch(const MvPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, uint32_t* ys,
                                uint32_t* flags, int32_t* status, hipStream_t st);
