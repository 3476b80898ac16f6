// mod64fri_items.cuh -- the FRI commit (fri.py:189-266) over any odd modulus below 2^64 on packed 64-bit words (fp64m.cuh): the per-item
// bodies of the leaf level of a Merkle tree, the fold and the branch gather as functions of (tree, row) resp. (work item).  mod64fri.hip
// wraps them in kernels, api_mod64fri.hip drives them; tests/native/mod64fri_host.cpp walks the same functions on the host over the same
// grids.  The proof bytes are modfri_items.cuh's over the same modulus: only the width of a stored value differs.
//
// Values are PLAIN and CANONICAL 8-byte words everywhere between the kernels: the packed transform's last pass leaves them so
// (ntt64_items.cuh) and the fold returns them so.  A leaf is x.to_bytes() (modp.py:94-95): 24 zero bytes, then the word big-endian, with
// no reduction of any kind.  The trees keep no leaf level (sh_dev_mod64_merkelize's does, it is its output): the gather re-derives a
// sampled leaf from its word.
//
// Fold: the closed form of mf_fold_row (modfri_items.cuh) on f64_* arithmetic -- with q = n / 4, I = w^q and v_j = values[i + j q],
//   column[i] = 1/4 (G0 + G1 t + G2 t^2 + G3 t^3),  t = x* / x_i,
//   G0 = u0 + u2, G2 = u0 - u2, G1 = u1 + u3, G3 = u1 - u3,  u0 = v0 + v2, u1 = v0 - v2, u2 = v1 + v3, u3 = (v1 - v3) / I.
// Only the multipliers are in Montgomery form -- t and I^-1 --, f64_mul(plain, Montgomery) is plain and canonical: five products per
// row.  The challenge x* = field(m[1]) is any 256-bit value (fri.py:229 keeps the bytes): f64_from_limbs reduces it after the byte swap,
// once per thread.  w_r^(-i) of round r is w0^(n0 - i 4^r), read from the ROUND-0 transform's own lo | hi table as
// hi[e >> h] lo[e & (2^h - 1)] (one product; e < n0): the commit builds no table of its own.  The 1/4 is two halvings; for p above 2^63
// the sum x + p of a halving carries a 65th bit, which m6_half shifts back in.
#pragma once
#include "blake2s.cuh"
#include "modfri_items.cuh"  // mf_ld8 / mf_st8, MF_WG, MF_MAX_ROUNDS
#include "ntt64_items.cuh"

struct M6Tree {
  const uint64_t* values;  // [batch][n] words, hashed as they are stored
  uint32_t* nodes;         // [batch][2n][8 words], the layout of merkle_tree.py:36-56
  uint64_t n;              // >= 4
  uint32_t batch;
  uint32_t store_leaves;   // write nodes[n, 2n) too (permute4 order)
};

struct M6Fold {
  const uint64_t* values;  // [batch][n] plain canonical (any 64-bit value when canon_in)
  const uint32_t* nodes;   // [batch][2n][8 words]: the challenge is node 1 of tree b; null: special_x
  uint32_t special_x[8];   // any 256-bit value, 8 x u32 little-endian limbs
  uint64_t* column;        // [batch][n/4] plain canonical
  const uint64_t *lo, *hi; // the round-0 transform's tables: w0^e = hi[e >> log_h] lo[e & (2^log_h - 1)], Montgomery form
  uint64_t n;
  uint32_t batch, log_n0, log_h, round_shift;  // this round's generator is w0^(2^round_shift)
  uint32_t canon_in;
  uint64_t inv_i;          // (w0^(n0/4))^-1, Montgomery form
};

struct M6Round {
  const uint64_t* values;    // [batch][n]   the words under nodes_m
  const uint64_t* column;    // [batch][n/4] the words under nodes_m2
  const uint32_t* nodes_m;   // [batch][2n][8]
  const uint32_t* nodes_m2;  // [batch][2q][8], q = n/4
  uint64_t n;
  uint64_t round_off;        // byte offset of this round inside a proof
  uint64_t work_begin;       // first work item of this round (prefix sum of (samples * slots + 1) * batch)
  uint32_t samples;
  uint32_t ys_off;           // ys[ys_off + b * samples ...]
};
struct M6Gather {
  M6Round r[MF_MAX_ROUNDS];
  uint32_t rounds, batch;
  const uint32_t* ys;
  uint8_t* proof;               // [batch][proof_stride]
  uint64_t proof_stride, work_total;
  const uint64_t* final_values; // [batch][final_n], written as 32-byte wire values at proof[b] + final_off (fri.py:212-214)
  uint64_t final_n, final_off;
};

// x.to_bytes(): 24 zero bytes, then the word big-endian
F64_HD void m6_wire_words(uint64_t x, uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 6; ++i) w[i] = 0u;
  w[6] = __builtin_bswap32((uint32_t)(x >> 32));
  w[7] = __builtin_bswap32((uint32_t)x);
}

// ---- the leaf level ----------------------------------------------------------------------------------------------------------------
// row i of permute4 (merkle_tree.py:11-23) of tree b: the leaves values[i + j n/4], the two nodes above them and their parent
template <bool WIDE>
F64_HD void m6_leaves_item(const M6Tree& t, uint64_t b, uint64_t i) {
  const uint64_t q = t.n >> 2;
  const uint64_t* src = t.values + b * t.n + i;
  uint32_t* tree = t.nodes + b * (2 * t.n) * 8;
  uint32_t w[4][8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m6_wire_words(src[j * q], w[j]);
    if (t.store_leaves) mf_st8(tree + (t.n + 4 * i + j) * 8, w[j]);
  }
  const b2digest d0 = b2_hash_pair<WIDE>(w[0], w[1]), d1 = b2_hash_pair<WIDE>(w[2], w[3]);
  mf_st8(tree + (t.n / 2 + 2 * i) * 8, d0.h);
  mf_st8(tree + (t.n / 2 + 2 * i + 1) * 8, d1.h);
  const b2digest d2 = b2_hash_pair<WIDE>(d0.h, d1.h);
  mf_st8(tree + (t.n / 4 + i) * 8, d2.h);
  if (i == 0) {
    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    mf_st8(tree, z);  // nodes[0]: the reference keeps b'' there
  }
}

// ---- the fold ----------------------------------------------------------------------------------------------------------------------
// x / 2 for canonical x: (x + p) / 2 when x is odd, the sum's 65th bit included; canonical
F64_HD uint64_t m6_half(uint64_t x, const f64_mod& M) {
  const uint64_t s = x + ((x & 1u) ? M.p : 0u);
  return (s >> 1) | ((uint64_t)(s < x) << 63);
}
// the challenge of tree b in Montgomery form
F64_HD uint64_t m6_challenge(const M6Fold& a, const f64_mod& M, uint64_t b) {
  uint32_t limbs[8];
  if (a.nodes) {
    uint32_t w[8];
    mf_ld8(a.nodes + (b * 2 * a.n + 1) * 8, w);  // special_x = field(m[1]) (fri.py:229), unreduced bytes
#pragma unroll
    for (int i = 0; i < 8; ++i) limbs[i] = __builtin_bswap32(w[7 - i]);
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) limbs[i] = a.special_x[i];
  }
  return f64_to_mont(f64_from_limbs(limbs, M), M);
}
F64_HD uint64_t m6_fold_row(const M6Fold& a, const f64_mod& M, uint64_t sx_mont, uint64_t b, uint64_t i) {
  const uint64_t q = a.n >> 2;
  const uint64_t* v = a.values + b * a.n + i;
  uint64_t v0 = v[0], v1 = v[q], v2 = v[2 * q], v3 = v[3 * q];
  if (a.canon_in) {
    v0 = f64_canon(v0, M);
    v1 = f64_canon(v1, M);
    v2 = f64_canon(v2, M);
    v3 = f64_canon(v3, M);
  }
  const uint64_t j = i << a.round_shift;  // below n0 / 4
  uint64_t t = sx_mont;
  if (j) {
    const uint64_t e = (1ull << a.log_n0) - j;  // w0^-j = w0^(n0 - j)
    t = f64_mul(sx_mont, f64_mul(a.hi[e >> a.log_h], a.lo[e & ((1ull << a.log_h) - 1)], M), M);
  }
  const uint64_t u0 = f64_add(v0, v2, M), u1 = f64_sub(v0, v2, M), u2 = f64_add(v1, v3, M);
  const uint64_t u3 = f64_mul(f64_sub(v1, v3, M), a.inv_i, M);
  const uint64_t G0 = f64_add(u0, u2, M), G2 = f64_sub(u0, u2, M), G1 = f64_add(u1, u3, M), G3 = f64_sub(u1, u3, M);
  uint64_t acc = f64_add(f64_mul(G3, t, M), G2, M);
  acc = f64_add(f64_mul(acc, t, M), G1, M);
  acc = f64_add(f64_mul(acc, t, M), G0, M);
  return m6_half(m6_half(acc, M), M);
}
// one fold row per work item: a round's column, and sh_mod64_fri_fold
F64_HD void m6_fold_item(const M6Fold& a, const f64_mod& M, uint64_t g) {
  const uint64_t q = a.n >> 2, b = g / q, i = g - b * q;
  a.column[b * q + i] = m6_fold_row(a, M, m6_challenge(a, M, b), b, i);
}

// ---- the gather: mk_branch (merkle_tree.py:59-68) for the 5 branches of every sample of every round, and the final layer -------------
F64_HD void m6_gather_item(const M6Gather& a, uint64_t g0) {
  uint32_t w[8];
  if (g0 >= a.work_total) {  // the final layer: [x.to_bytes() for x in values] (fri.py:214)
    const uint64_t g = g0 - a.work_total;
    if (g >= a.final_n * a.batch) return;
    const uint64_t b = g / a.final_n, i = g - b * a.final_n;
    m6_wire_words(a.final_values[g], w);
    mf_st8(reinterpret_cast<uint32_t*>(a.proof + b * a.proof_stride + a.final_off) + 8 * i, w);
    return;
  }
  uint32_t ri = 0;
  while (ri + 1 < a.rounds && g0 >= a.r[ri + 1].work_begin) ++ri;
  const M6Round& rd = a.r[ri];
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
  const uint64_t* vals;
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
    // branch entries 0 and 1 are the leaf and its sibling leaf: permuted slot pi (or pi ^ 1) holds the word at (pi & 3) n/4 + (pi >> 2)
    const uint64_t ps = pi ^ lev;
    m6_wire_words(vals[(ps & 3) * ld4 + (ps >> 2)], w);
  } else {
    mf_ld8(tree + (((pi + leaves) >> (lev - 1)) ^ 1) * 8, w);
  }
  mf_st8(out + 8 + ((uint64_t)s * per_sample + slot) * 8, w);
}
