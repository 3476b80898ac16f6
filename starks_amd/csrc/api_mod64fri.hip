// api_mod64fri.hip -- the FRI commit (fri.py:189-266) over any odd modulus below 2^64 on packed 64-bit words, on the host side, and
// its entry points: the transform is api_ntt64.hip's, the leaf level, the fold and the gather are mod64fri.hip's, the tree levels above
// the leaf kernels and the index sampler are the MiMC path's (kernels.hip).  Every check runs on the host before anything is launched.
// The proof bytes are sh_mod_fri_prove's over the same modulus on the same values.
#include "ctx.hpp"
#include "mod64fri_items.cuh"
using namespace shk;

namespace {
// the fields of a fold that come from the round-0 domain of n points (n >= 4)
M6Fold fold_args(const Mod64Call& mc, const uint64_t* tab, uint64_t n) {
  M6Fold fa;
  memset(&fa, 0, sizeof fa);
  fa.n = n;
  fa.log_n0 = (uint32_t)mc.log_n;
  fa.log_h = (uint32_t)n64_log_h(mc.log_n);
  fa.lo = tab;
  fa.hi = tab + (1ull << fa.log_h);
  fa.inv_i = f64_pow(mc.root_mont, 3 * (n / 4), mc.M);  // I^-1 = I^3, I = root^(n/4)
  return fa;
}

// every host check of a commit; on SH_OK mc holds the call's constants
int mod64fri_check(sh_ctx* c, uint64_t modulus, uint64_t root, uint64_t n_coeffs, uint64_t n, uint64_t maxdeg_plus_1, uint32_t exclude,
                   uint32_t samples, uint32_t batch, Mod64Call* mc, const char* who) {
  if (!is_pow2(n)) {
    c->err = std::string(who) + ": n must be a power of two";
    return SH_ERR_INVALID;
  }
  if (batch == 0) {
    c->err = std::string(who) + ": batch must be at least 1";
    return SH_ERR_INVALID;
  }
  SH_TRY(mod64_prepare(c, modulus, root, n, batch, false, false, mc, who));
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

// the commit on coefficient words that are on the device: src = [batch][n_coeffs], any 64-bit values
int mod64fri_run(sh_ctx* c, const Mod64Call& mc, const void* src, uint64_t n_coeffs, uint64_t n, uint64_t maxdeg_plus_1,
                 uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* d_proof) {
  const uint64_t* tab = nullptr;
  SH_TRY(mod64_table(c, mc, &tab));
  Fri64Buffers fb;
  SH_TRY(mod64fri_buffers(c, n, batch, samples, &fb));
  // values = fft(f) over the whole domain (fri.py:207-208): plain, canonical
  SH_TRY(mod64_run(c, mc, tab, src, n_coeffs, fb.vals, batch));
  return mod64fri_rounds(c, mc, tab, fb, n, maxdeg_plus_1, exclude, samples, batch, d_proof, fri_proof_len(n, maxdeg_plus_1, samples),
                         false);
}
}  // namespace

namespace shk {
// fri_buffers (api_fri.hip) with 8 bytes per value
int mod64fri_buffers(sh_ctx* c, uint64_t n, uint32_t batch, uint32_t samples, Fri64Buffers* b) {
  void *va, *vb, *ta, *tb, *misc;
  SH_TRY(ws_get(c, sh_ctx::WS_COL_A, (size_t)batch * n * 8, &va));
  SH_TRY(ws_get(c, sh_ctx::WS_COL_B, (size_t)batch * (n / 3 + 2) * 8, &vb));
  SH_TRY(ws_get(c, sh_ctx::WS_TREE_A, (size_t)batch * 2 * n * 32, &ta));
  SH_TRY(ws_get(c, sh_ctx::WS_TREE_B, (size_t)batch * 2 * (n / 3 + 2) * 32, &tb));
  SH_TRY(ws_get(c, sh_ctx::WS_MISC, (size_t)batch * ((samples > 40 ? samples : 40) + 40 * SHK_FRI_MAX_ROUNDS) * 4 + 64, &misc));
  b->vals = reinterpret_cast<uint64_t*>(va);
  b->next = reinterpret_cast<uint64_t*>(vb);
  b->tree = reinterpret_cast<uint32_t*>(ta);
  b->tree2 = reinterpret_cast<uint32_t*>(tb);
  b->ys = reinterpret_cast<uint32_t*>(misc);
  return SH_OK;
}

// The rounds of the commit (fri.py:212-266) on the plain canonical words in fb.vals (and, when have_tree, their Merkle tree in
// fb.tree); proof b is written at d_proof + b * stride.  modfri_rounds (api_modfri.hip) with 8-byte values.
int mod64fri_rounds(sh_ctx* c, const Mod64Call& mc, const uint64_t* tab, Fri64Buffers fb, uint64_t n, uint64_t maxdeg_plus_1,
                    uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* d_proof, uint64_t stride, bool have_tree) {
  uint64_t* vals = fb.vals;
  uint64_t* next = fb.next;
  uint32_t* tree = fb.tree;
  uint32_t* tree2 = fb.tree2;
  M6Fold fa = n >= 4 ? fold_args(mc, tab, n) : M6Fold{};
  fa.batch = batch;
  FriSampleArgs sa;  // what the sampler reads
  memset(&sa, 0, sizeof sa);
  sa.batch = batch;
  sa.exclude = exclude;
  sa.ys = fb.ys;
  M6Gather ga;
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
      M6Tree t = {vals, tree, nn, batch, 0};
      HIP_TRY(c, shk_m6_leaves(t, c->stream));
      HIP_TRY(c, shk_merkle_upper_levels(nn, batch, tree, c->stream));
    }
    fa.values = vals;
    fa.nodes = tree;
    fa.column = next;
    fa.n = nn;
    fa.round_shift = 2 * round;
    HIP_TRY(c, shk_m6_fold(fa, mc.M, c->stream));  // column, fri.py:235-240
    M6Tree t2 = {next, tree2, nn / 4, batch, 0};   // m2 = merkelize(column), fri.py:243
    HIP_TRY(c, shk_m6_leaves(t2, c->stream));
    HIP_TRY(c, shk_merkle_upper_levels(nn / 4, batch, tree2, c->stream));
    const uint64_t lg = (uint64_t)ilog2(nn);
    sa.r[round].nodes_m2 = tree2;
    sa.r[round].n = nn;
    sa.r[round].samples = s;
    sa.r[round].ys_off = ys_off;
    M6Round& r = ga.r[round];
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
  HIP_TRY(c, shk_m6_gather(ga, c->stream));       // fri.py:251-254 and the final layer
  return SH_OK;
}
}  // namespace shk

extern "C" {

int sh_dev_mod64_fri_prove(sh_ctx* c, uint64_t modulus, const void* d_coeffs, uint64_t n_coeffs, uint64_t n, uint64_t root,
                           uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, uint32_t batch, void* d_proof) {
  if (!c) return SH_ERR_INVALID;
  if (!d_proof || (n_coeffs && !d_coeffs)) {
    c->err = "sh_dev_mod64_fri_prove: null pointer";
    return SH_ERR_INVALID;
  }
  Mod64Call mc;
  SH_TRY(mod64fri_check(c, modulus, root, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, &mc, "sh_dev_mod64_fri_prove"));
  SH_TRY(enter(c));
  return mod64fri_run(c, mc, d_coeffs, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, reinterpret_cast<uint8_t*>(d_proof));
}

int sh_mod64_fri_prove(sh_ctx* c, uint64_t modulus, const uint64_t* coeffs, uint64_t n_coeffs, uint64_t n, uint64_t root,
                       uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* proof, uint64_t proof_cap) {
  if (!c) return SH_ERR_INVALID;
  if (!proof || (n_coeffs && !coeffs)) {
    c->err = "sh_mod64_fri_prove: null pointer";
    return SH_ERR_INVALID;
  }
  Mod64Call mc;
  SH_TRY(mod64fri_check(c, modulus, root, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, &mc, "sh_mod64_fri_prove"));
  const uint64_t stride = fri_proof_len(n, maxdeg_plus_1, samples);
  if (proof_cap < stride * batch) {
    c->err = "sh_mod64_fri_prove: proof_cap is below batch * sh_fri_proof_len(n, maxdeg_plus_1, samples)";
    return SH_ERR_TOO_SMALL;
  }
  SH_TRY(enter(c));
  void *w = nullptr, *dp = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)batch * n_coeffs * 8, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_PROOF, (size_t)stride * batch, &dp));
  SH_TRY(h2d(c, w, coeffs, (size_t)batch * n_coeffs * 8));
  SH_TRY(mod64fri_run(c, mc, w, n_coeffs, n, maxdeg_plus_1, exclude, samples, batch, reinterpret_cast<uint8_t*>(dp)));
  return d2h(c, proof, dp, (size_t)stride * batch);
}

int sh_mod64_fri_fold(sh_ctx* c, uint64_t modulus, const uint64_t* values, uint64_t n, uint64_t root, const uint8_t special_x[32],
                      uint64_t* column) {
  if (!c) return SH_ERR_INVALID;
  if (!values || !special_x || !column) {
    c->err = "sh_mod64_fri_fold: null pointer";
    return SH_ERR_INVALID;
  }
  if (!is_pow2(n) || n < 4) {
    c->err = "sh_mod64_fri_fold: n must be a power of two, and a fold takes at least 4 values";
    return SH_ERR_INVALID;
  }
  Mod64Call mc;
  SH_TRY(mod64_prepare(c, modulus, root, n, 1, false, false, &mc, "sh_mod64_fri_fold"));
  SH_TRY(enter(c));
  const uint64_t* tab = nullptr;
  SH_TRY(mod64_table(c, mc, &tab));
  void *v = nullptr, *col = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)n * 8, &v));
  SH_TRY(ws_get(c, sh_ctx::WS_COL_B, (size_t)(n / 4) * 8, &col));
  SH_TRY(h2d(c, v, values, (size_t)n * 8));
  M6Fold fa = fold_args(mc, tab, n);
  fa.values = reinterpret_cast<const uint64_t*>(v);
  for (int i = 0; i < 8; ++i) {  // nodes stay null: the challenge is special_x, any 256-bit value, big-endian bytes -> limbs
    const uint8_t* b = special_x + 4 * (7 - i);
    fa.special_x[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
  }
  fa.column = reinterpret_cast<uint64_t*>(col);
  fa.batch = 1;
  fa.canon_in = 1;
  HIP_TRY(c, shk_m6_fold(fa, mc.M, c->stream));
  return d2h(c, column, col, (size_t)(n / 4) * 8);
}

int sh_dev_mod64_merkelize(sh_ctx* c, const void* d_words, uint64_t n, uint32_t batch, void* d_nodes) {
  if (!c) return SH_ERR_INVALID;
  if (!d_words || !d_nodes || !is_pow2(n) || n < 4 || batch == 0 || batch > 65535) {
    c->err = "sh_dev_mod64_merkelize: n must be a power of two >= 4, batch in 1 .. 65535, the buffers non-null";
    return SH_ERR_INVALID;
  }
  SH_TRY(enter(c));
  M6Tree t = {reinterpret_cast<const uint64_t*>(d_words), reinterpret_cast<uint32_t*>(d_nodes), n, batch, 1};
  HIP_TRY(c, shk_m6_leaves(t, c->stream));
  HIP_TRY(c, shk_merkle_upper_levels(n, batch, t.nodes, c->stream));
  return SH_OK;
}
}  // extern "C"
