// modfri_items.cuh -- the FRI commit (fri.py:189-266) over any odd modulus below 2^256 (fpm.cuh): the per-item bodies of the leaf
// level of a Merkle tree, the fold and the branch gather as functions of (tree, row) resp. (work item).  modfri.hip wraps them in
// kernels, api_modfri.hip drives them; tests/native/modfri_host.cpp walks the same functions on the host over the same grids.
//
// Values are PLAIN and CANONICAL (below p) everywhere between the kernels: the transform's last pass leaves them so (modntt_items.cuh)
// and the fold returns them so.  A leaf is therefore the value's 8 limbs as 32 big-endian bytes, x.to_bytes() (modp.py:94-95), with no
// reduction modulo anything -- in particular not modulo the MiMC prime, which would change a value in [MIMC_P, p).  The trees keep no
// leaf level (sh_dev_merkelize_plain's does, it is its output): the gather re-derives a sampled leaf from its value, a byte swap.
//
// Fold (the closed form of kernels.hip's fri_fold_row): with q = n / 4, x_i = w^i, I = w^q and v_j = values[i + j q],
//   column[i] = 1/4 (G0 + G1 t + G2 t^2 + G3 t^3),  t = x* / x_i,
//   G0 = u0 + u2, G2 = u0 - u2, G1 = u1 + u3, G3 = u1 - u3,  u0 = v0 + v2, u1 = v0 - v2, u2 = v1 + v3, u3 = (v1 - v3) / I.
// root^(n/2) = -1 makes I^2 = -1, so the four denominators of the reference's Lagrange route (poly_utils.py:412-440) are 4 x_i^3 up to
// a power of I: units of any ring where 2 is, and the closed form is that route's value, residue for residue.  Only the multipliers
// are in Montgomery form -- t and I^-1 --, fpm_mul(plain, Montgomery) is plain and canonical: five products per row.  The challenge
// x* = field(m[1]) is any 256-bit value (fri.py:229 keeps the bytes); fpm_to_mont reduces it, once per thread.  The 1/4 is two halvings.
// w_r^(-i) of round r is w0^(-i 4^r) = -w0^(n0/2 - i 4^r) for i > 0: one entry of the ROUND-0 transform's table (w0^e in Montgomery
// form, e < n0 / 2; i 4^r < n0 / 4), so the commit builds no table of its own.
#pragma once
#include "blake2s.cuh"
#include "modntt_items.cuh"

constexpr uint32_t MF_WG = 256;          // threads per workgroup
constexpr uint32_t MF_MAX_ROUNDS = 12;   // SHK_FRI_MAX_ROUNDS

struct MfTree {
  const fpm* values;   // [batch][n] plain values, hashed as they are stored
  uint32_t* nodes;     // [batch][2n][8 words], the layout of merkle_tree.py:36-56
  uint64_t n;          // >= 4
  uint32_t batch;
  uint32_t store_leaves;  // write nodes[n, 2n) too (permute4 order)
};

struct MfFold {
  const fpm* values;       // [batch][n] plain canonical (wire form, any value, when wire_io)
  const uint32_t* nodes;   // [batch][2n][8 words]: the challenge is node 1 of tree b; null: special_x
  fpm special_x;           // any 256-bit value, plain
  fpm* column;             // [batch][n/4] plain canonical (wire form when wire_io)
  const fpm* tw;           // w0^e, Montgomery form, e < n0 / 2
  uint64_t n;
  uint32_t batch, log_n0, round_shift;  // this round's generator is w0^(2^round_shift)
  uint32_t wire_io;
  fpm inv_i;               // (w0^(n0/4))^-1, Montgomery form
};

struct MfRound {
  const fpm* values;         // [batch][n]   the values under nodes_m
  const fpm* column;         // [batch][n/4] the values under nodes_m2
  const uint32_t* nodes_m;   // [batch][2n][8]
  const uint32_t* nodes_m2;  // [batch][2q][8], q = n/4
  uint64_t n;
  uint64_t round_off;        // byte offset of this round inside a proof
  uint64_t work_begin;       // first work item of this round (prefix sum of (samples * slots + 1) * batch)
  uint32_t samples;
  uint32_t ys_off;           // ys[ys_off + b * samples ...]
};
struct MfGather {
  MfRound r[MF_MAX_ROUNDS];
  uint32_t rounds, batch;
  const uint32_t* ys;
  uint8_t* proof;            // [batch][proof_stride]
  uint64_t proof_stride, work_total;
  const fpm* final_values;   // [batch][final_n], written as wire bytes at proof[b] + final_off (fri.py:212-214)
  uint64_t final_n, final_off;
};

// ---- 32-byte node access -----------------------------------------------------------------------------------------------------------
FPM_HD void mf_ld8(const uint32_t* p, uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
  w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
#else
  for (int i = 0; i < 8; ++i) w[i] = p[i];
#endif
}
FPM_HD void mf_st8(uint32_t* p, const uint32_t w[8]) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
#else
  for (int i = 0; i < 8; ++i) p[i] = w[i];
#endif
}

// ---- the leaf level ----------------------------------------------------------------------------------------------------------------
// row i of permute4 (merkle_tree.py:11-23) of one tree: the leaves v[j] = values[i + j n/4], the two nodes above them and their parent
template <bool WIDE>
FPM_HD void mf_hash_row(uint32_t* tree, uint64_t n, uint64_t i, const fpm v[4], bool store_leaves) {
  uint32_t w[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    fpm_to_wire_words(v[j], w[j]);
    if (store_leaves) mf_st8(tree + (n + 4 * i + j) * 8, w[j]);
  }
  const b2digest d0 = b2_hash_pair<WIDE>(w[0], w[1]), d1 = b2_hash_pair<WIDE>(w[2], w[3]);
  mf_st8(tree + (n / 2 + 2 * i) * 8, d0.h);
  mf_st8(tree + (n / 2 + 2 * i + 1) * 8, d1.h);
  const b2digest d2 = b2_hash_pair<WIDE>(d0.h, d1.h);
  mf_st8(tree + (n / 4 + i) * 8, d2.h);
  if (i == 0) {
    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    mf_st8(tree, z);  // nodes[0]: the reference keeps b'' there
  }
}
template <bool WIDE>
FPM_HD void mf_leaves_item(const MfTree& t, uint64_t b, uint64_t i) {
  const uint64_t q = t.n >> 2;
  const fpm* src = t.values + b * t.n + i;
  fpm v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = mn_ld(src + j * q);
  mf_hash_row<WIDE>(t.nodes + b * (2 * t.n) * 8, t.n, i, v, t.store_leaves != 0);
}

// ---- the fold ----------------------------------------------------------------------------------------------------------------------
// x / 2 for canonical x: (x + p) / 2 when x is odd; canonical
FPM_HD fpm mf_half(const fpm& x, const fpm_mod& M) {
  const uint32_t mask = (x.v[0] & 1u) ? 0xffffffffu : 0u;
  uint32_t t[9];
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t s = (uint64_t)x.v[i] + (M.p[i] & mask) + carry;
    t[i] = (uint32_t)s;
    carry = s >> 32;
  }
  t[8] = (uint32_t)carry;
  fpm r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (t[i] >> 1) | (t[i + 1] << 31);
  return r;
}
// the challenge of tree b in Montgomery form
FPM_HD fpm mf_challenge(const MfFold& a, const fpm_mod& M, uint64_t b) {
  fpm sx = a.special_x;
  if (a.nodes) {
    uint32_t w[8];
    mf_ld8(a.nodes + (b * 2 * a.n + 1) * 8, w);  // special_x = field(m[1]) (fri.py:229), unreduced bytes
    sx = fpm_from_wire_words(w);
  }
  return fpm_to_mont(sx, M);
}
FPM_HD fpm mf_fold_row(const MfFold& a, const fpm_mod& M, const fpm& sx_mont, uint64_t b, uint64_t i) {
  const uint64_t q = a.n >> 2;
  const fpm* v = a.values + b * a.n + i;
  fpm v0 = mn_ld(v), v1 = mn_ld(v + q), v2 = mn_ld(v + 2 * q), v3 = mn_ld(v + 3 * q);
  if (a.wire_io) {
    v0 = fpm_canon(fpm_from_wire_words(v0.v), M);
    v1 = fpm_canon(fpm_from_wire_words(v1.v), M);
    v2 = fpm_canon(fpm_from_wire_words(v2.v), M);
    v3 = fpm_canon(fpm_from_wire_words(v3.v), M);
  }
  const uint64_t j = i << a.round_shift;  // below n0 / 4
  fpm t = sx_mont;
  if (j) t = fpm_neg(fpm_mul(sx_mont, mn_ld(a.tw + ((1ull << (a.log_n0 - 1)) - j)), M), M);
  const fpm u0 = fpm_add(v0, v2, M), u1 = fpm_sub(v0, v2, M), u2 = fpm_add(v1, v3, M);
  const fpm u3 = fpm_mul(fpm_sub(v1, v3, M), a.inv_i, M);
  const fpm G0 = fpm_add(u0, u2, M), G2 = fpm_sub(u0, u2, M), G1 = fpm_add(u1, u3, M), G3 = fpm_sub(u1, u3, M);
  fpm acc = fpm_add(fpm_mul(G3, t, M), G2, M);
  acc = fpm_add(fpm_mul(acc, t, M), G1, M);
  acc = fpm_add(fpm_mul(acc, t, M), G0, M);
  return mf_half(mf_half(acc, M), M);
}
// one fold row per work item: a round's column, and sh_mod_fri_fold
FPM_HD void mf_fold_item(const MfFold& a, const fpm_mod& M, uint64_t g) {
  const uint64_t q = a.n >> 2, b = g / q, i = g - b * q;
  fpm r = mf_fold_row(a, M, mf_challenge(a, M, b), b, i);
  if (a.wire_io) {
    fpm w;
    fpm_to_wire_words(r, w.v);
    r = w;
  }
  mn_st(a.column + b * q + i, r);
}

// ---- the gather: mk_branch (merkle_tree.py:59-68) for the 5 branches of every sample of every round, and the final layer -------------
FPM_HD void mf_gather_item(const MfGather& a, uint64_t g0) {
  uint32_t w[8];
  if (g0 >= a.work_total) {  // the final layer: [x.to_bytes() for x in values] (fri.py:214)
    const uint64_t g = g0 - a.work_total;
    if (g >= a.final_n * a.batch) return;
    const uint64_t b = g / a.final_n, i = g - b * a.final_n;
    fpm_to_wire_words(mn_ld(a.final_values + g), w);
    mf_st8(reinterpret_cast<uint32_t*>(a.proof + b * a.proof_stride + a.final_off) + 8 * i, w);
    return;
  }
  uint32_t ri = 0;
  while (ri + 1 < a.rounds && g0 >= a.r[ri + 1].work_begin) ++ri;
  const MfRound& rd = a.r[ri];
  const uint64_t g = g0 - rd.work_begin;
  const uint64_t q = rd.n >> 2;
  uint32_t l1 = 1;
  while ((1ull << (l1 - 1)) < rd.n) ++l1;  // log2(n) + 1
  const uint32_t l2 = l1 - 2;              // log2(n/4) + 1
  const uint32_t per_sample = l2 + 4 * l1;
  const uint64_t per_proof = (uint64_t)rd.samples * per_sample + 1;  // +1: the root2 slot
  const uint64_t b = g / per_proof;
  uint64_t r = g - b * per_proof;
  uint32_t* out = reinterpret_cast<uint32_t*>(a.proof + b * a.proof_stride + rd.round_off);
  const uint32_t* m = rd.nodes_m + b * 2 * rd.n * 8;
  const uint32_t* m2 = rd.nodes_m2 + b * 2 * q * 8;
  if (r == 0) {
    mf_ld8(m2 + 8, w);
    mf_st8(out, w);
    return;
  }
  r -= 1;
  const uint32_t s = (uint32_t)(r / per_sample), slot = (uint32_t)(r - (uint64_t)s * per_sample);
  const uint32_t y = a.ys[rd.ys_off + b * rd.samples + s];
  const uint32_t* tree;
  const fpm* vals;
  uint64_t leaves, index;
  uint32_t lev;
  if (slot < l2) {
    tree = m2; vals = rd.column + b * q; leaves = q; index = y; lev = slot;
  } else {
    const uint32_t br = (slot - l2) / l1;
    tree = m; vals = rd.values + b * rd.n; leaves = rd.n; index = y + q * br; lev = (slot - l2) - br * l1;
  }
  const uint64_t ld4 = leaves >> 2;  // get_index_in_permuted (merkle_tree.py:26-33)
  const uint64_t pi = index / ld4 + 4 * (index % ld4);
  if (lev <= 1) {
    // branch entries 0 and 1 are the leaf and its sibling leaf: permuted slot pi (or pi ^ 1) holds the value at (pi & 3) n/4 + (pi >> 2)
    const uint64_t ps = pi ^ lev;
    fpm_to_wire_words(mn_ld(vals + (ps & 3) * ld4 + (ps >> 2)), w);
  } else {
    mf_ld8(tree + (((pi + leaves) >> (lev - 1)) ^ 1) * 8, w);
  }
  mf_st8(out + 8 + ((uint64_t)s * per_sample + slot) * 8, w);
}
