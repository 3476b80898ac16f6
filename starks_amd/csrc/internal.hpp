// internal.hpp -- declarations shared by the translation units of libstarkhip.so (not installed).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp256.cuh"
#include "knobs.hpp"

struct NttPassArgs {
  const fp* src;
  fp* dst;
  uint64_t total;     // number of columns (column pass: batch*P*S) or rows (row pass: batch*P)
  uint32_t log_n;     // log2 of the transform length
  uint32_t log_S;     // column pass: log2 stride between successive points of a column
  uint32_t log_P;     // row pass: log2 number of rows per transform (n / R)
  const fp2* wR;      // w^(n/R * k), k < R/2, each with its second image w * 2^128 mod p (fp256.cuh: fp_mul2)
  // column pass: table of g = w^P, order R*S:  g^e = lo[e & mask] (* hi[e >> lb] unless direct)
  const fp* tw_lo;
  const fp* tw_hi;
  uint32_t tw_lb;
  uint32_t tw_direct;
  // row pass: radix logs of the earlier passes (digits k_1 .. k_{m-1} of the row number, k_1 first)
  uint32_t ndig;
  uint32_t dig_log[3];
  const fp* scale;    // row pass: optional factor applied to every output (n^-1 of a one-pass inverse)
  uint64_t src_n;     // first pass only: the source holds src_n <= n elements per vector, the rest of each vector is zero
                      // (fft_1d's zero padding, fft.py:323-324, never materialised); 0 = the source holds n per vector
  const fp* tw2;      // column passes: the same twiddles as [k][j2] rows, tw2[k * S + j2] = g^(j2 * k) -- one coalesced load per
                      // element; null: use the power table (tw_lo / tw_hi)
  uint32_t pass_index; // 0 = the first pass of the transform (experiments: STARKHIP_TILE_LOGS picks a tile size per pass)
  uint32_t xcd_per;   // 0: tile = blockIdx.x.  Else workgroups are dealt to the 8 XCDs round-robin and tile = (blockIdx.x & 7) *
                      // xcd_per + (blockIdx.x >> 3): adjacent tiles run on the SAME XCD (they share 128-byte lines when T < 4)
};

// ---- ntt.hip ----------------------------------------------------------------------------------
// Launch one tile pass (radix 2^log_R) in the cell shk_ntt_choose_cell (knobs.hpp) picks under the knobs of the process.  Returns
// hipSuccess or the launch error.
hipError_t shk_launch_ntt_pass(int log_R, bool last, const NttPassArgs& a, hipStream_t st);
// The same pass in one named kernel instantiation (tests/native/ntt_ops.hip runs each on its own); hipErrorInvalidValue for a cell
// that does not exist (knobs.hpp: shk_ntt_cell_exists).  The caller answers for the arguments: nothing here checks them.
hipError_t shk_launch_ntt_cell(const ShkNttCell& cell, int log_R, bool last, const NttPassArgs& a, hipStream_t st);
hipError_t shk_launch_ntt_tiny(const fp* src, fp* dst, uint32_t n, uint32_t batch, const fp* scale, hipStream_t st);

// ---- kernels.hip: conversions, powers, Merkle, FRI fold, sampling, branch gather ------------------
hipError_t shk_wire_to_limb(const uint8_t* d_wire, fp* d_limbs, uint64_t n, hipStream_t st);
hipError_t shk_limb_to_wire(const fp* d_limbs, uint8_t* d_wire, uint64_t n, hipStream_t st);
hipError_t shk_fill_seeded(fp* d, uint64_t n, uint64_t seed, hipStream_t st);
hipError_t shk_fill_mimc_units(fp* wit, fp* inputs, uint64_t steps, uint32_t first_unit, uint32_t batch, uint32_t constant,
                               hipStream_t st);
hipError_t shk_pointwise_mul(const fp* a, const fp* b, fp* out, uint64_t n, hipStream_t st);
// out[i] = g^i for i < n, g given by its two-level table (lo, hi, lb)
hipError_t shk_powers(const fp* lo, const fp* hi, uint32_t lb, fp* out, uint64_t n, hipStream_t st);
hipError_t shk_tw2(const fp* lo, const fp* hi, uint32_t lb, fp* out, uint32_t log_R, uint32_t log_S, hipStream_t st);
// zero-pad: dst[b][0..n_in) = src[b][0..n_in), dst[b][n_in..n) = 0
hipError_t shk_pad_copy(const fp* src, fp* dst, uint64_t n_in, uint64_t n, uint32_t batch, hipStream_t st);
// Merkle tree of `batch` arrays of n limb-form values (or n raw 32-byte leaves when raw_leaves).
// store_leaves = false leaves nodes[n, 2n) unwritten (limb-form input only): for callers that gather leaves from the values
hipError_t shk_merkelize(const void* d_leaves, bool raw_leaves, uint64_t n, uint32_t batch, uint32_t* d_nodes,
                         hipStream_t st, bool store_leaves = true);
hipError_t shk_merkle_upper_levels(uint64_t n, uint32_t batch, uint32_t* d_nodes, hipStream_t st);
// packed leaves (merkle_tree.py:94-119): d_evals [k][n][32 B] wire; d_leaves [n][k][32 B] permuted; d_nodes [n][32 B]
hipError_t shk_merkelize_packed(const uint8_t* d_evals, uint64_t n, uint32_t k, uint8_t* d_leaves, uint32_t* d_nodes,
                                hipStream_t st);
struct FoldArgs {
  const fp* values;        // [batch][n]
  const uint32_t* nodes;   // [batch][2n][8 words]; challenge = node 1 (nullptr: use special_x)
  const uint32_t* special_x;  // 8 wire words (used when nodes == nullptr)
  fp* column;              // [batch][n/4]
  uint64_t n;
  uint32_t batch;
  // powers of the ROUND-0 generator w0 (order n0): w0^e = lo[e & mask] * hi[e >> lb]
  const fp* tw_lo;
  const fp* tw_hi;
  uint32_t tw_lb;
  uint32_t log_n0;
  uint32_t round_shift;    // this round's generator is w0^(2^round_shift)
  fp inv_i;                // (w0^(n0/4))^-1: inverse of the primitive 4th root of unity
};
hipError_t shk_fri_fold(const FoldArgs& a, hipStream_t st);
// the fold and the Merkle tree of its column (nodes layout of shk_merkelize without the leaf level): [batch][2 * n/4][8 words]
hipError_t shk_fri_fold_and_tree(const FoldArgs& a, uint32_t* d_nodes2, hipStream_t st);
// Query sampling + branch gather of ALL rounds of a FRI commit in two launches (fri.py:246-254 per round): every round keeps
// its values and its tree until the end of the commit, so nothing on the serial chain tree -> challenge -> fold -> tree waits
// for the 40 x 5 branch copies of the round before.
constexpr uint32_t SHK_FRI_MAX_ROUNDS = 12;  // domain <= 2^26 (the column of round 0 must stay below 2^24 rows, utils.py:69)
struct FriRound {
  const fp* values;          // [batch][n]   the values under nodes_m  (leaves are re-derived from them)
  const fp* column;          // [batch][n/4] the values under nodes_m2
  const uint32_t* nodes_m;   // [batch][2n][8]   tree of the values
  const uint32_t* nodes_m2;  // [batch][2q][8]   tree of the column (q = n/4)
  uint64_t n;
  uint64_t round_off;        // byte offset of this round inside a proof
  uint32_t samples;
  uint32_t ys_off;           // this round's slice of the ys scratch: ys[(ys_off + b * samples) ...]
  uint64_t work_begin;       // gather: first work item of this round (prefix sum of (samples * slots + 1) * batch)
};
struct FriSampleArgs {
  FriRound r[SHK_FRI_MAX_ROUNDS];
  uint32_t rounds;
  uint32_t batch;
  uint32_t exclude;
  uint32_t* ys;              // scratch, sum over rounds of batch * samples
  uint8_t* proof;            // [batch][proof_stride] device proof buffers
  uint64_t proof_stride;
  uint64_t work_total;
  // the final layer (fri.py:212-214), written by the same gather launch: canonical wire form of final_values[b][0..final_n) at
  // proof[b] + final_off
  const fp* final_values;
  uint64_t final_n;
  uint64_t final_off;
};
hipError_t shk_fri_sample_and_gather_all(const FriSampleArgs& a, hipStream_t st);
// ys[b][0..samples) = get_pseudorandom_indices(node 1 of tree b, modulus, samples, exclude) (utils.py:60-90);
// trees are tree_words u32 apart
hipError_t shk_sample_indices(const uint32_t* d_nodes, uint64_t tree_words, uint32_t modulus, uint32_t batch,
                              uint32_t samples, uint32_t exclude, uint32_t* d_ys, hipStream_t st);
// the sampling launch of shk_fri_sample_and_gather_all alone (reads r[].nodes_m2, n, samples, ys_off; batch, exclude, ys): the commit
// over another modulus samples with it and gathers with its own kernel (modfri.hip)
hipError_t shk_fri_sample_all(const FriSampleArgs& a, hipStream_t st);

// ---- stark.hip: constraint / boundary quotients, packed tree, linear combination, spot checks (stark.py:233-279) ----
constexpr uint32_t SHK_STARK_MAX_WIDTH = 9;  // get_pseudorandom_ks returns None from 10 on (stark.py:106-126)
constexpr uint32_t SHK_STARK_MAX_TERMS = 256;
struct StarkArgs {
  const fp* p_evals;  // [batch * width][n]  trace polynomials on the G2 domain
  fp* d_work;         // [batch * width][n]  D evaluations
  fp* b_work;         // [batch * width][n]  B evaluations
  const fp* q_evals;  // [batch * width][steps]  Q_c = X P_c'(X) on G1
  const fp* wit;      // [batch * width][steps]  the witness itself = the trace polynomials on G1 (read contiguously by the
                      // trace-point kernel instead of every ext-th entry of p_evals)
  const fp* iab;      // [batch * width][3]  boundary interpolant a + b X: a, b, b 2^128 (b as an fp_mul2 pair)
  uint64_t n;         // precision = steps * ext
  uint64_t steps;
  uint32_t ext;
  uint32_t width;
  uint32_t batch;
  const fp* tw_lo;    // powers of G2: G2^e = lo[e & mask] (* hi[e >> lb] when hi)
  const fp* tw_hi;
  uint32_t tw_lb;
  // per-(steps, ext) tables over the domain (cached by the context, shared by every proof of every batch):
  const fp* inv_z2;     // [n]   1 / ((x_i - 1)(x_i - x_last)), 0 at the two roots
  const fp* xpow;       // [n]   x_i = G2^i
  const fp* fz;         // [n]   (x_i - x_last) / (x_i^steps - 1) = 1 / Z(x_i), 0 on the trace points (i % ext == 0)
                        // (as fp_mul2 pairs the two factor tables measured 1 % slower: 64 B more table traffic per point)
  const fp* inv_omega;  // [ext] 1 / (omega^j - 1), omega = G2^steps, entry 0 = 0
  fp x_last;          // G2^((steps - 1) ext)  (stark.py:212)
  fp g1;              // G2^ext = 1 / x_last
  fp inv_steps;       // 1 / steps
  fp inv_1_m_last;    // 1 / (1 - x_last)
  uint32_t* bad;      // [batch] bad[b] is set to 1 when a transition constraint of proof b fails on the trace
  // step polynomials: term t = coef[t] * prod_v X_v^exps[t][v] (exps rows are width + 1 bytes: the last one flags
  // coef == 1); terms of dimension c: [term_begin[c], term_begin[c+1])
  const fp* term_coef;
  const uint8_t* term_exps;
  uint32_t term_begin[SHK_STARK_MAX_WIDTH + 1];
  // their partial derivatives: d step_c / d X_v = terms [dterm_begin[c * width + v], dterm_begin[c * width + v + 1])
  const fp* dterm_coef;
  const uint8_t* dterm_exps;
  const uint32_t* dterm_begin;
};
hipError_t shk_stark_interp(const fp* trace, const fp* inputs, uint64_t steps, uint32_t cols, const fp& inv_last_m1, fp* iab,
                            hipStream_t st);
hipError_t shk_stark_qprep(const fp* pcoef, fp* q, uint64_t steps, uint64_t cols, hipStream_t st);
// the three domain tables, out = [3][n]: inv_z2, xpow, fz (inv_omega = the [ext] table, already on the device)
hipError_t shk_stark_domain_tables(fp* out, uint64_t n, uint32_t ext, const fp* tw_lo, const fp* tw_hi, uint32_t tw_lb, const fp& x_last,
                                   const fp* inv_omega, hipStream_t st);
// D = C / Z and B = (P - I) / Z2 on the whole domain and the packed-leaf Merkle tree over (P, D, B), in one pass over the domain (the
// quotients are hashed where they are computed)
hipError_t shk_stark_quotients_and_merkelize(const StarkArgs& a, uint32_t* d_nodes, hipStream_t st);
hipError_t shk_stark_scalars(const uint32_t* d_mnodes, uint64_t tree_words, uint32_t width, uint32_t batch, const fp& cpow,
                             fp* d_scal, hipStream_t st);
// l = the Fiat-Shamir linear combination of P, D, B (scalars as (s, s 2^128) pairs) and the Merkle tree of l
// (merkelize(l_evaluations)): the combination is fused with the tree's first three levels
hipError_t shk_stark_lincomb_tree(const StarkArgs& a, const fp* d_scal, fp* d_l, uint32_t* d_lnodes, hipStream_t st);
hipError_t shk_stark_gather(const StarkArgs& a, const uint32_t* d_mnodes, const uint32_t* d_lnodes, const fp* d_lvals,
                            const uint32_t* d_ys, uint32_t samples, uint8_t* d_proof, uint64_t stride, hipStream_t st);

// ---- multi_inv.hip: batch inversion and four-point interpolation (poly_utils.py:301-320, 412-440; inv_items.cuh) ----------------
// scratch: shk_multi_inv_scratch(n) / shk_multi_interp_4_scratch(rows) elements (0 when the items fit one tile)
uint64_t shk_multi_inv_scratch(uint64_t n);
uint64_t shk_multi_interp_4_scratch(uint64_t rows);
// out[i] = in[i]^-1, 0 for in[i] == 0 mod p; in may equal out; n >= 1
hipError_t shk_multi_inv(const fp* in, fp* out, uint64_t n, fp* scratch, hipStream_t st);
// xs, ys, coeffs: [rows][4]; coeffs may equal xs or ys; rows >= 1
hipError_t shk_multi_interp_4(const fp* xs, const fp* ys, fp* coeffs, uint64_t rows, fp* scratch, hipStream_t st);

// ---- poly_arith.hip: products, division, zpoly, lagrange_interp (polynomial.py:116-150, poly_utils.py:322-369; poly_items.cuh) ----
#include "poly_items.cuh"
hipError_t shk_pa_copy(const PaCopy& c, const fp* src, fp* dst, hipStream_t st);
// hz: [nodes][2^log2d] transformed Z-nodes -> oz [nodes/2][2^log2d] (parents, before the inverse transform); hn / on the same for
// the numerators (either pair may be null)
hipError_t shk_pa_tree(const fp* hz, fp* oz, const fp* hn, fp* on, uint32_t log2d, uint64_t nodes, hipStream_t st);
// hd: [children/2][2^log2d] transformed parent remainders; hr: [children][2^log2d] transformed rev(Z) of the children, replaced
// in place by parent * sibling
hipError_t shk_pa_mid(const fp* hd, fp* hr, uint32_t log2d, uint64_t children, hipStream_t st);
hipError_t shk_pa_newton(const fp* F, fp* G, uint64_t n, hipStream_t st);
hipError_t shk_pa_inv1(const fp* src, fp* dst, hipStream_t st);
hipError_t shk_pa_deriv_rev(const fp* top, fp* out, uint64_t N, uint64_t n, hipStream_t st);
hipError_t shk_pa_weights(const fp* ys, const fp* inv, fp* out, uint64_t n, uint64_t N, hipStream_t st);
hipError_t shk_pa_sub(const fp* a, const fp* b, fp* out, uint64_t n, hipStream_t st);

// ---- poly_eval.hip: evaluation at arbitrary points (polynomial.py:158-164; poly_items.cuh: pa_eval_direct, pa_eval_tree) ----------
// tbl[b m + i] = x_i^(2^b), b <= lgS
hipError_t shk_pe_pow_table(const fp* xs, uint64_t m, uint32_t lgS, fp* tbl, hipStream_t st);
// dst[b][w][i]: workgroup w's sum for point i of polynomial b (canonical when s.W = 1); coefs [batch][n]
hipError_t shk_pe_direct(const PeDirect& s, const fp* coefs, const fp* tbl, fp* dst, hipStream_t st);
// out[b][i] = the canonical sum of part[b][0, W)[i]
hipError_t shk_pe_sum(const PeDirect& s, const fp* part, fp* out, hipStream_t st);
// dst [batch C][N] = the reversed chunks of coefs [batch][n] (pe_chunk_rev_item)
hipError_t shk_pe_chunks(const fp* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, fp* dst, hipStream_t st);
// a[r][i] *= b[i], r < rows, i < len
hipError_t shk_pe_bcast_mul(fp* a, const fp* b, uint64_t rows, uint64_t len, hipStream_t st);
// out[b][i] = sum_j leaves[b C + j][i] (x_i^N)^j, canonical
hipError_t shk_pe_combine(const fp* leaves, const fp* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, fp* out, hipStream_t st);

// ---- modntt.hip: the transform over any odd modulus below 2^256 (fft.py:256-345 with a run-time modulus; modntt_items.cuh) --------
#include "modntt_items.cuh"
// one tile pass of the plan (mn_pass); the modulus block is an argument of the launch
hipError_t shk_mn_pass(const MnPass& a, const fpm_mod& M, hipStream_t st);
// t.tw[e] = w^e in Montgomery form, e < t.count
hipError_t shk_mn_tw(const MnTw& t, const fpm_mod& M, hipStream_t st);
// out[i] = x[i] y[i] mod p, plain form, canonical
hipError_t shk_mn_pointwise(const fpm* x, const fpm* y, fpm* out, uint64_t n, const fpm_mod& M, hipStream_t st);

// ---- modfri.hip: the FRI commit over any odd modulus below 2^256 (fri.py:189-266; modfri_items.cuh, which the two files that use
// these include themselves: it brings blake2s.cuh) -------------------------------------------------------------------------------------
struct MfTree;
struct MfFold;
struct MfGather;
// the leaf-kernel levels of the trees of t.values: nodes [n/4, n), and [n, 2n) when store_leaves; shk_merkle_upper_levels does the rest
hipError_t shk_mf_leaves(const MfTree& t, hipStream_t st);
// a.column = the fold of a.values, one thread per row
hipError_t shk_mf_fold(const MfFold& a, const fpm_mod& M, hipStream_t st);
hipError_t shk_mf_gather(const MfGather& a, hipStream_t st);

// ---- modstark.hip: the STARK prover's middle over any prime modulus below 2^256 (stark.py:233-279; modstark_items.cuh, which the two
// files that use these include themselves) ---------------------------------------------------------------------------------------------
struct MsArgs;
struct MsInv;
struct MsTables;
struct MsGather;
// a.out[i] = a.in[i]^-1, Montgomery form in and out, 0 for 0
hipError_t shk_ms_batch_inv(const MsInv& a, const fpm_mod& M, hipStream_t st);
// t.table = inv_z2 | fz | xpow of (p, steps, ext); t.den is [2][n] of scratch; pm2 = p - 2
hipError_t shk_ms_tables(const MsTables& t, const fpm& pm2, const fpm_mod& M, hipStream_t st);
hipError_t shk_ms_interp(const MsArgs& a, const fpm_mod& M, hipStream_t st);
hipError_t shk_ms_qprep(const fpm* pcoef, fpm* q, uint64_t steps, uint64_t cols, const fpm_mod& M, hipStream_t st);
// D = C / Z and B = (P - I) / Z2 on the whole domain, then the packed-leaf Merkle tree over (P, D, B)
hipError_t shk_ms_quotients_and_merkelize(const MsArgs& a, const fpm_mod& M, uint32_t* d_nodes, hipStream_t st);
// d_scal [batch][width][3]: alpha_j, alpha_j beta, alpha_j gamma in Montgomery form
hipError_t shk_ms_scalars(const uint32_t* d_mnodes, uint64_t tree_words, uint32_t width, uint32_t batch, const fpm& cpow, fpm* d_scal,
                          const fpm_mod& M, hipStream_t st);
hipError_t shk_ms_lincomb(const MsArgs& a, const fpm* d_scal, fpm* d_l, const fpm_mod& M, hipStream_t st);
hipError_t shk_ms_gather(const MsArgs& a, const MsGather& ga, hipStream_t st);

// ---- ntt64.hip: the transform over any odd modulus below 2^64 on packed 64-bit words (ntt64_items.cuh) ------------------------------
#include "ntt64_items.cuh"
// one tile pass of the plan (n64_pass); the modulus block is an argument of the launch
hipError_t shk_n64_pass(const N64Pass& a, const f64_mod& M, hipStream_t st);
// t.tab = lo | hi | stw, Montgomery form (n64_tw_item)
hipError_t shk_n64_tw(const N64Tw& t, const f64_mod& M, hipStream_t st);
// out[i] = x[i] y[i] mod p, plain form, canonical
hipError_t shk_n64_pointwise(const uint64_t* x, const uint64_t* y, uint64_t* out, uint64_t n, const f64_mod& M, hipStream_t st);
// words[i] = (8 x u32 limbs i) mod p; limbs[i] = words[i] zero-extended
hipError_t shk_n64_from_limbs(const void* limbs, uint64_t* words, uint64_t count, const f64_mod& M, hipStream_t st);
hipError_t shk_n64_to_limbs(const uint64_t* words, void* limbs, uint64_t count, hipStream_t st);

// ---- mod64fri.hip: the FRI commit over any odd modulus below 2^64 on packed words (fri.py:189-266; mod64fri_items.cuh, which the two
// files that use these include themselves: it brings blake2s.cuh) ----------------------------------------------------------------------
struct M6Tree;
struct M6Fold;
struct M6Gather;
// the leaf-kernel levels of the trees of t.values: nodes [n/4, n), and [n, 2n) when store_leaves; shk_merkle_upper_levels does the rest
hipError_t shk_m6_leaves(const M6Tree& t, hipStream_t st);
// a.column = the fold of a.values, one thread per row
hipError_t shk_m6_fold(const M6Fold& a, const f64_mod& M, hipStream_t st);
hipError_t shk_m6_gather(const M6Gather& a, hipStream_t st);

// ---- mod64stark.hip: the STARK prover's middle over any prime modulus below 2^64 on packed words (stark.py:233-279;
// mod64stark_items.cuh, which the two files that use these include themselves) ------------------------------------------------------------
struct M6sArgs;
struct M6sTables;
struct M6sGather;
// t.table = inv_z2 | fz | xpow of (p, steps, ext); t.den is [2][n] of scratch
hipError_t shk_m6s_tables(const M6sTables& t, const f64_mod& M, hipStream_t st);
hipError_t shk_m6s_interp(const M6sArgs& a, const f64_mod& M, hipStream_t st);
hipError_t shk_m6s_qprep(const uint64_t* pcoef, uint64_t* q, uint64_t steps, uint64_t cols, const f64_mod& M, hipStream_t st);
// D = C / Z and B = (P - I) / Z2 on the whole domain, then the packed-leaf Merkle tree over (P, D, B)
hipError_t shk_m6s_quotients_and_merkelize(const M6sArgs& a, const f64_mod& M, uint32_t* d_nodes, hipStream_t st);
// d_scal [batch][width][3]: alpha_j, alpha_j beta, alpha_j gamma in Montgomery form
hipError_t shk_m6s_scalars(const uint32_t* d_mnodes, uint64_t tree_words, uint32_t width, uint32_t batch, uint64_t cpow, uint64_t* d_scal,
                           const f64_mod& M, hipStream_t st);
hipError_t shk_m6s_lincomb(const M6sArgs& a, const uint64_t* d_scal, uint64_t* d_l, const f64_mod& M, hipStream_t st);
hipError_t shk_m6s_gather(const M6sArgs& a, const M6sGather& ga, hipStream_t st);

// ---- modpoly.hip: polynomial arithmetic and batch inversion over any prime modulus below 2^256 (modpoly_items.cuh; every array holds
// PLAIN values, the modulus block is an argument of every launch) ------------------------------------------------------------------------
hipError_t shk_mp_copy(const PaCopy& c, const fpm* src, fpm* dst, const fpm_mod& M, hipStream_t st);
// 32-byte big-endian wire values <-> limbs: a byte swap, its own inverse, nothing is reduced; src may equal dst
hipError_t shk_mp_swap(const void* src, void* dst, uint64_t n, hipStream_t st);
hipError_t shk_mp_tree(const fpm* hz, fpm* oz, const fpm* hn, fpm* on, uint32_t log2d, uint64_t nodes, const fpm_mod& M, hipStream_t st);
hipError_t shk_mp_mid(const fpm* hd, fpm* hr, uint32_t log2d, uint64_t children, const fpm_mod& M, hipStream_t st);
hipError_t shk_mp_newton(const fpm* F, fpm* G, uint64_t n, const fpm_mod& M, hipStream_t st);
hipError_t shk_mp_inv1(const fpm* src, fpm* dst, const fpm_mod& M, hipStream_t st);
hipError_t shk_mp_deriv_rev(const fpm* top, fpm* out, uint64_t N, uint64_t n, const fpm_mod& M, hipStream_t st);
hipError_t shk_mp_weights(const fpm* ys, const fpm* inv, fpm* out, uint64_t n, uint64_t N, const fpm_mod& M, hipStream_t st);
hipError_t shk_mp_sub(const fpm* a, const fpm* b, fpm* out, uint64_t n, const fpm_mod& M, hipStream_t st);
// scratch: elements of the levels above the items (0 when they fit one tile)
uint64_t shk_mp_multi_inv_scratch(uint64_t n);
uint64_t shk_mp_multi_interp_4_scratch(uint64_t rows);
// out[i] = in[i]^-1, 0 for in[i] == 0 mod p; in may equal out; n >= 1
hipError_t shk_mp_multi_inv(const fpm* in, fpm* out, uint64_t n, fpm* scratch, const fpm_mod& M, hipStream_t st);
// xs, ys, coeffs: [rows][4]; coeffs may equal xs or ys; rows >= 1
hipError_t shk_mp_multi_interp_4(const fpm* xs, const fpm* ys, fpm* coeffs, uint64_t rows, fpm* scratch, const fpm_mod& M, hipStream_t st);

// ---- modeval.hip: evaluation at arbitrary points over any prime modulus below 2^256 (modeval_items.cuh; poly_items.cuh: pa_eval_direct,
// pa_eval_tree).  Plain values everywhere but tbl, which holds Montgomery forms ---------------------------------------------------------
// tbl[b m + i] = x_i^(2^b) R, b <= lgS
hipError_t shk_me_pow_table(const fpm* xs, uint64_t m, uint32_t lgS, fpm* tbl, const fpm_mod& M, hipStream_t st);
// dst[b][w][i]: workgroup w's sum for point i of polynomial b, canonical; coefs [batch][n], any 256-bit values
hipError_t shk_me_direct(const PeDirect& s, const fpm* coefs, const fpm* tbl, fpm* dst, const fpm_mod& M, hipStream_t st);
hipError_t shk_me_sum(const PeDirect& s, const fpm* part, fpm* out, const fpm_mod& M, hipStream_t st);
hipError_t shk_me_chunks(const fpm* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, fpm* dst, hipStream_t st);
hipError_t shk_me_bcast_mul(fpm* a, const fpm* b, uint64_t rows, uint64_t len, const fpm_mod& M, hipStream_t st);
hipError_t shk_me_combine(const fpm* leaves, const fpm* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, fpm* out, const fpm_mod& M,
                          hipStream_t st);

// ---- mod64poly.hip: polynomial arithmetic and batch inversion over any prime modulus below 2^64 on packed 64-bit words
// (mod64poly_items.cuh; every array holds PLAIN words, the modulus block is an argument of every launch).  The pointwise product of two
// transforms is shk_n64_pointwise ------------------------------------------------------------------------------------------------------
hipError_t shk_m6p_copy(const PaCopy& c, const uint64_t* src, uint64_t* dst, const f64_mod& M, hipStream_t st);
// log2d >= 1 (rows of 2d >= 2 words)
hipError_t shk_m6p_tree(const uint64_t* hz, uint64_t* oz, const uint64_t* hn, uint64_t* on, uint32_t log2d, uint64_t nodes,
                        const f64_mod& M, hipStream_t st);
hipError_t shk_m6p_mid(const uint64_t* hd, uint64_t* hr, uint32_t log2d, uint64_t children, const f64_mod& M, hipStream_t st);
hipError_t shk_m6p_newton(const uint64_t* F, uint64_t* G, uint64_t n, const f64_mod& M, hipStream_t st);
hipError_t shk_m6p_inv1(const uint64_t* src, uint64_t* dst, const f64_mod& M, hipStream_t st);
hipError_t shk_m6p_deriv_rev(const uint64_t* top, uint64_t* out, uint64_t N, uint64_t n, const f64_mod& M, hipStream_t st);
hipError_t shk_m6p_weights(const uint64_t* ys, const uint64_t* inv, uint64_t* out, uint64_t n, uint64_t N, const f64_mod& M,
                           hipStream_t st);
hipError_t shk_m6p_sub(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n, const f64_mod& M, hipStream_t st);
// scratch: words of the levels above the items (0 when they fit one tile)
uint64_t shk_m6p_multi_inv_scratch(uint64_t n);
uint64_t shk_m6p_multi_interp_4_scratch(uint64_t rows);
// out[i] = in[i]^-1, 0 for in[i] == 0 mod p; in may equal out; n >= 1
hipError_t shk_m6p_multi_inv(const uint64_t* in, uint64_t* out, uint64_t n, uint64_t* scratch, const f64_mod& M, hipStream_t st);
// xs, ys, coeffs: [rows][4]; coeffs may equal xs or ys; rows >= 1
hipError_t shk_m6p_multi_interp_4(const uint64_t* xs, const uint64_t* ys, uint64_t* coeffs, uint64_t rows, uint64_t* scratch,
                                  const f64_mod& M, hipStream_t st);

// ---- mod64eval.hip: evaluation at arbitrary points over any prime modulus below 2^64 on packed 64-bit words (mod64eval_items.cuh;
// poly_items.cuh: pa_eval_direct, pa_eval_tree).  Plain words everywhere but tbl, which holds Montgomery forms ---------------------------
// tbl[b m + i] = x_i^(2^b) R, b <= lgS
hipError_t shk_m6e_pow_table(const uint64_t* xs, uint64_t m, uint32_t lgS, uint64_t* tbl, const f64_mod& M, hipStream_t st);
// dst[b][w][i]: workgroup w's sum for point i of polynomial b, canonical; coefs [batch][n], any 64-bit values
hipError_t shk_m6e_direct(const PeDirect& s, const uint64_t* coefs, const uint64_t* tbl, uint64_t* dst, const f64_mod& M, hipStream_t st);
hipError_t shk_m6e_sum(const PeDirect& s, const uint64_t* part, uint64_t* out, const f64_mod& M, hipStream_t st);
// N a power of two, at least 2; dst 16-byte aligned (a workspace buffer)
hipError_t shk_m6e_chunks(const uint64_t* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, uint64_t* dst, hipStream_t st);
// len even; a and b 16-byte aligned (workspace buffers)
hipError_t shk_m6e_bcast_mul(uint64_t* a, const uint64_t* b, uint64_t rows, uint64_t len, const f64_mod& M, hipStream_t st);
hipError_t shk_m6e_combine(const uint64_t* leaves, const uint64_t* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, uint64_t* out,
                           const f64_mod& M, hipStream_t st);
