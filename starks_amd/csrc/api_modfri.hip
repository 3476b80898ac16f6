// api_modfri.hip -- the FRI commit (fri.py:189-266) over any odd modulus below 2^256 on the host side, and its entry points: the
// transform is api_modntt.hip's, the leaf level, the fold and the gather are modfri.hip's, the tree levels above the leaf kernels and
// the index sampler are the MiMC path's (kernels.hip).  Every check runs on the host before anything is launched.
#include "ctx.hpp"
#include "modfri_items.cuh"
using namespace shk;

namespace {
// the fields of a fold that come from the round-0 domain
MfFold fold_args(const ModCall& mc, const fpm* tw, uint64_t n) {
  MfFold fa;
  memset(&fa, 0, sizeof fa);
  fa.n = n;
  fa.tw = tw;
  fa.log_n0 = (uint32_t)mc.log_n;
  fa.inv_i = fpm_pow(mc.root_mont, 3 * (n / 4), mc.M);  // I^-1 = I^3, I = root^(n/4)
  return fa;
}

// every host check of a commit; on SH_OK mc holds the call's constants
int modfri_check(sh_ctx* c, const uint8_t modulus[32], const uint8_t root[32], uint64_t n_coeffs, uint64_t n, uint64_t maxdeg_plus_1,
                 uint32_t exclude, uint32_t samples, uint32_t batch, ModCall* mc, const char* who) {
  SH_TRY(mod_prepare(c, modulus, root, n, batch, false, false, mc, who));
  if (n_coeffs > n) {
    c->err = std::string(who) + ": more coefficients than the domain has points";
    return SH_ERR_INVALID;
  }
  const char* why = "";
  const int rc = fri_validate(n, maxdeg_plus_1, exclude, samples, &why);  // the MiMC commit's own rule, with its reason
  if (rc != SH_OK) {
    c->err = std::string(who) + ": " + why;
    return rc;
  }
  if (maxdeg_plus_1 > 16 && batch > 65535) {
    c->err = std::string(who) + ": a commit with rounds takes at most 65535 polynomials per call";
    return SH_ERR_UNSUPPORTED;
  }
  return SH_OK;
}

// the commit on coefficients that are on the device: src = [batch][n_coeffs], wire form when wire_in, else limbs
int modfri_run(sh_ctx* c, const ModCall& mc, const void* src, bool wire_in, uint64_t n_coeffs, uint64_t n, uint64_t maxdeg_plus_1,
               uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* d_proof) {
  const fpm* tw = nullptr;
  SH_TRY(mod_table(c, mc, &tw));
  FriBuffers fb;  // the MiMC commit's arenas: an element is 32 bytes there and here
  SH_TRY(fri_buffers(c, n, batch, samples, &fb));
  // values = fft(f) over the whole domain (fri.py:207-208): plain, canonical
  SH_TRY(mod_run(c, mc, tw, src, n_coeffs, fb.vals, batch, wire_in, false));
  return modfri_rounds(c, mc, tw, fb, n, maxdeg_plus_1, exclude, samples, batch, d_proof, fri_proof_len(n, maxdeg_plus_1, samples), false);
}
}  // namespace

namespace shk {
// The rounds of the commit (fri.py:212-266) on the plain canonical evaluations in fb.vals (and, when have_tree, their Merkle tree in
// fb.tree: the generic STARK prover has built it for its spot checks); proof b is written at d_proof + b * stride.
int modfri_rounds(sh_ctx* c, const ModCall& mc, const fpm* tw, FriBuffers fb, uint64_t n, uint64_t maxdeg_plus_1, uint32_t exclude,
                  uint32_t samples, uint32_t batch, uint8_t* d_proof, uint64_t stride, bool have_tree) {
  fpm* vals = reinterpret_cast<fpm*>(fb.vals);
  fpm* next = reinterpret_cast<fpm*>(fb.next);
  uint32_t* tree = fb.tree;
  uint32_t* tree2 = fb.tree2;
  MfFold fa = n >= 4 ? fold_args(mc, tw, n) : MfFold{};
  fa.batch = batch;
  FriSampleArgs sa;  // what the sampler reads
  memset(&sa, 0, sizeof sa);
  sa.batch = batch;
  sa.exclude = exclude;
  sa.ys = fb.ys;
  MfGather ga;
  memset(&ga, 0, sizeof ga);
  ga.batch = batch;
  ga.ys = fb.ys;
  ga.proof = d_proof;
  ga.proof_stride = stride;
  uint64_t nn = n, md = maxdeg_plus_1, off = 0;
  uint32_t round = 0, ys_off = 0;
  while (md > 16) {  // at most SHK_FRI_MAX_ROUNDS rounds of at least 16 points: fri_validate has refused anything else
    const uint32_t s = round == 0 ? samples : 40;
    if (round == 0 && !have_tree) {  // m = merkelize(values), fri.py:224; a later round's m is the round before's m2
      MfTree t = {vals, tree, nn, batch, 0};
      HIP_TRY(c, shk_mf_leaves(t, c->stream));
      HIP_TRY(c, shk_merkle_upper_levels(nn, batch, tree, c->stream));
    }
    fa.values = vals;
    fa.nodes = tree;
    fa.column = next;
    fa.n = nn;
    fa.round_shift = 2 * round;
    HIP_TRY(c, shk_mf_fold(fa, mc.M, c->stream));  // column, fri.py:235-240
    MfTree t2 = {next, tree2, nn / 4, batch, 0};   // m2 = merkelize(column), fri.py:243
    HIP_TRY(c, shk_mf_leaves(t2, c->stream));
    HIP_TRY(c, shk_merkle_upper_levels(nn / 4, batch, tree2, c->stream));
    const uint64_t lg = (uint64_t)ilog2(nn);
    sa.r[round].nodes_m2 = tree2;
    sa.r[round].n = nn;
    sa.r[round].samples = s;
    sa.r[round].ys_off = ys_off;
    MfRound& r = ga.r[round];
    r.values = vals;
    r.column = next;
    r.nodes_m = tree;
    r.nodes_m2 = tree2;
    r.n = nn;
    r.round_off = off;
    r.samples = s;
    r.ys_off = ys_off;
    r.work_begin = ga.work_total;
    ga.work_total += ((uint64_t)s * ((lg - 1) + 4 * (lg + 1)) + 1) * batch;
    ys_off += batch * s;
    off += 32 + (uint64_t)s * 32 * ((lg - 1) + 4 * (lg + 1));
    // fri.py:260-266: the inverse transform over root^4 and the transform back are the identity on the column; every round's column
    // and tree stay in the arenas until the gather
    vals = next;
    tree = tree2;
    next = next + (size_t)batch * (nn / 4);
    tree2 = tree2 + (size_t)batch * 2 * (nn / 4) * 8;
    nn >>= 2;
    md >>= 2;
    ++round;
  }
  sa.rounds = ga.rounds = round;
  ga.final_values = vals;  // fri.py:212-214
  ga.final_n = nn;
  ga.final_off = off;
  HIP_TRY(c, shk_fri_sample_all(sa, c->stream));  // fri.py:246-247, all rounds in one launch
  HIP_TRY(c, shk_mf_gather(ga, c->stream));       // fri.py:251-254 and the final layer
  return SH_OK;
}
}  // namespace shk

extern "C" {

int sh_dev_mod_fri_prove(sh_ctx* c, const uint8_t modulus[32], const void* d_coeffs, uint64_t n_coeffs, uint64_t n,
                         const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, uint32_t batch,
                         void* d_proof) {
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !root || !d_proof || (n_coeffs && !d_coeffs)) {
    c->err = "sh_dev_mod_fri_prove: null pointer";
    return SH_ERR_INVALID;
  }
  ModCall mc;
  SH_TRY(modfri_check(c, modulus, root, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, &mc, "sh_dev_mod_fri_prove"));
  SH_TRY(enter(c));
  return modfri_run(c, mc, d_coeffs, false, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, reinterpret_cast<uint8_t*>(d_proof));
}

int sh_mod_fri_prove(sh_ctx* c, const uint8_t modulus[32], const uint8_t* coeffs, uint64_t n_coeffs, uint64_t n,
                     const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, uint32_t batch,
                     uint8_t* proof, uint64_t proof_cap) {
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !root || !proof || (n_coeffs && !coeffs)) {
    c->err = "sh_mod_fri_prove: null pointer";
    return SH_ERR_INVALID;
  }
  ModCall mc;
  SH_TRY(modfri_check(c, modulus, root, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, &mc, "sh_mod_fri_prove"));
  const uint64_t stride = fri_proof_len(n, maxdeg_plus_1, samples);
  if (proof_cap < stride * batch) {
    c->err = "sh_mod_fri_prove: proof_cap is below batch * sh_fri_proof_len(n, maxdeg_plus_1, samples)";
    return SH_ERR_TOO_SMALL;
  }
  SH_TRY(enter(c));
  void *w = nullptr, *dp = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)batch * n_coeffs * 32, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_PROOF, (size_t)stride * batch, &dp));
  SH_TRY(h2d(c, w, coeffs, (size_t)batch * n_coeffs * 32));
  SH_TRY(modfri_run(c, mc, w, true, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, reinterpret_cast<uint8_t*>(dp)));
  return d2h(c, proof, dp, (size_t)stride * batch);
}

int sh_mod_fri_fold(sh_ctx* c, const uint8_t modulus[32], const uint8_t* values, uint64_t n, const uint8_t root[32],
                    const uint8_t special_x[32], uint8_t* column) {
  if (!c) return SH_ERR_INVALID;
  if (!modulus || !values || !root || !special_x || !column) {
    c->err = "sh_mod_fri_fold: null pointer";
    return SH_ERR_INVALID;
  }
  ModCall mc;
  SH_TRY(mod_prepare(c, modulus, root, n, 1, false, false, &mc, "sh_mod_fri_fold"));
  if (n < 4) {
    c->err = "sh_mod_fri_fold: a fold takes at least 4 values";
    return SH_ERR_INVALID;
  }
  SH_TRY(enter(c));
  const fpm* tw = nullptr;
  SH_TRY(mod_table(c, mc, &tw));
  void *v = nullptr, *col = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)n * 32, &v));
  SH_TRY(ws_get(c, sh_ctx::WS_COL_B, (size_t)(n / 4) * 32, &col));
  SH_TRY(h2d(c, v, values, (size_t)n * 32));
  MfFold fa = fold_args(mc, tw, n);
  fa.values = reinterpret_cast<const fpm*>(v);
  fa.special_x = fpm_from_wire_bytes(special_x);  // nodes stay null: the challenge is special_x, any 256-bit value
  fa.column = reinterpret_cast<fpm*>(col);
  fa.batch = 1;
  fa.wire_io = 1;
  HIP_TRY(c, shk_mf_fold(fa, mc.M, c->stream));
  return d2h(c, column, col, (size_t)(n / 4) * 32);
}

int sh_dev_merkelize_plain(sh_ctx* c, const void* d_values, uint64_t n, uint32_t batch, void* d_nodes) {
  if (!c) return SH_ERR_INVALID;
  if (!d_values || !d_nodes || !is_pow2(n) || n < 4 || batch == 0 || batch > 65535) {
    c->err = "sh_dev_merkelize_plain: n must be a power of two >= 4, batch in 1 .. 65535, the buffers non-null";
    return SH_ERR_INVALID;
  }
  SH_TRY(enter(c));
  MfTree t = {reinterpret_cast<const fpm*>(d_values), reinterpret_cast<uint32_t*>(d_nodes), n, batch, 1};
  HIP_TRY(c, shk_mf_leaves(t, c->stream));
  HIP_TRY(c, shk_merkle_upper_levels(n, batch, t.nodes, c->stream));
  return SH_OK;
}
}  // extern "C"
