// api_fri.hip -- Merkle trees, the FRI fold and the FRI commit (fri.py:189-266) on the host side, and their entry points.
#include "ctx.hpp"
using namespace shk;

namespace {
// the fields of a fold that come from the plan of its n-point round-0 domain; the caller adds the buffers, the batch and, in later
// rounds, n and round_shift
FoldArgs fold_args(const NttPlan* pl, uint64_t n) {
  FoldArgs fa;
  memset(&fa, 0, sizeof fa);
  fa.n = n;
  fa.tw_lo = pl->base.lo;
  fa.tw_hi = pl->base.hi;
  fa.tw_lb = pl->base.lb;
  fa.log_n0 = (uint32_t)pl->log_n;
  fa.inv_i = h_pow(pl->root, 3 * (n / 4));  // I^-1 = I^3, I = root^(n/4)
  return fa;
}

// FRI commit on device-resident coefficients; see starkhip.h for the layout.
int run_fri(sh_ctx* c, const fp* d_coeffs, uint64_t n, const uint8_t root[32], uint64_t maxdeg_plus_1,
            uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* d_proof, uint64_t n_coeffs = 0) {
  if (!d_coeffs || !d_proof || batch == 0 || !is_pow2(n)) return SH_ERR_INVALID;
  NttPlan* pl = nullptr;
  SH_TRY(plan_for(c, root, n, false, &pl));
  SH_TRY(fri_validate(n, maxdeg_plus_1, exclude, samples));
  FriBuffers fb;
  SH_TRY(fri_buffers(c, n, batch, samples, &fb));
  // values = fft(f) over the whole domain (fri.py:207-208)
  SH_TRY(run_ntt(c, pl, d_coeffs, fb.vals, batch, n_coeffs));  // n_coeffs != 0: [batch][n_coeffs], zero padding implicit
  return fri_rounds(c, pl, fb, n, maxdeg_plus_1, exclude, samples, batch, d_proof,
                    fri_proof_len(n, maxdeg_plus_1, samples), false);
}
}  // namespace

namespace shk {
uint64_t fri_proof_len(uint64_t n, uint64_t maxdeg_plus_1, uint32_t samples) {
  uint64_t total = 0;
  bool first = true;
  while (maxdeg_plus_1 > 16 && n >= 16) {
    const uint64_t lg = (uint64_t)ilog2(n);
    total += 32 + (uint64_t)(first ? samples : 40) * 32 * ((lg - 1) + 4 * (lg + 1));
    n >>= 2;
    maxdeg_plus_1 >>= 2;
    first = false;
  }
  return total + 32 * n;
}

// every round's parameters are checked before anything is launched; `why`, when given, receives the reason of a refusal
int fri_validate(uint64_t n, uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, const char** why) {
  const char* sink = "";
  const char*& reason = why ? *why : sink;
  uint64_t nn = n, md = maxdeg_plus_1;
  bool first = true;
  uint32_t rounds = 0;
  while (md > 16) {
    reason = "more rounds than a commit holds (SHK_FRI_MAX_ROUNDS)";
    if (++rounds > SHK_FRI_MAX_ROUNDS) return SH_ERR_UNSUPPORTED;  // FriSampleArgs holds that many rounds (checked BEFORE any launch)
    reason = "a round with fewer than 16 points (maxdeg_plus_1 is too large for n)";
    if (nn < 16) return SH_ERR_INVALID;            // the reference cannot merkelize a column of < 4 values
    reason = "a column of 2^24 rows or more cannot be sampled (utils.py:69)";
    if ((nn >> 2) >= (1ull << 24)) return SH_ERR_UNSUPPORTED;  // assert modulus < 2**24 (utils.py:69)
    const uint32_t s = first ? samples : 40;
    reason = "samples must be at least 1";
    if (s == 0) return SH_ERR_INVALID;
    reason = "exclude_multiples_of = 1 divides by zero in the reference (utils.py:90)";
    if (exclude == 1) return SH_ERR_INVALID;       // division by zero in the reference (utils.py:90)
    reason = "exclude_multiples_of leaves no row to sample";
    if (exclude && ((nn >> 2) * (exclude - 1)) / exclude == 0) return SH_ERR_INVALID;
    nn >>= 2;
    md >>= 2;
    first = false;
  }
  reason = "";
  return SH_OK;
}

int fri_buffers(sh_ctx* c, uint64_t n, uint32_t batch, uint32_t samples, FriBuffers* b) {
  void *va, *vb, *ta, *tb, *misc;
  SH_TRY(ws_get(c, sh_ctx::WS_COL_A, (size_t)batch * n * sizeof(fp), &va));
  SH_TRY(ws_get(c, sh_ctx::WS_COL_B, (size_t)batch * (n / 3 + 2) * sizeof(fp), &vb));
  SH_TRY(ws_get(c, sh_ctx::WS_TREE_A, (size_t)batch * 2 * n * 32, &ta));
  SH_TRY(ws_get(c, sh_ctx::WS_TREE_B, (size_t)batch * 2 * (n / 3 + 2) * 32, &tb));
  SH_TRY(ws_get(c, sh_ctx::WS_MISC, (size_t)batch * ((samples > 40 ? samples : 40) + 40 * SHK_FRI_MAX_ROUNDS) * 4 + 64, &misc));
  b->vals = reinterpret_cast<fp*>(va);
  b->next = reinterpret_cast<fp*>(vb);
  b->tree = reinterpret_cast<uint32_t*>(ta);
  b->tree2 = reinterpret_cast<uint32_t*>(tb);
  b->ys = reinterpret_cast<uint32_t*>(misc);
  return SH_OK;
}

// The rounds of the FRI commit (fri.py:212-266) on the evaluations in fb.vals (and, when have_tree, their Merkle
// tree in fb.tree); proof b is written at d_proof + b * stride.
int fri_rounds(sh_ctx* c, NttPlan* pl, FriBuffers fb, uint64_t n, uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples,
               uint32_t batch, uint8_t* d_proof, uint64_t stride, bool have_tree) {
  fp* vals = fb.vals;
  fp* next = fb.next;
  uint32_t* tree = fb.tree;
  uint32_t* tree2 = fb.tree2;
  uint64_t nn = n, md = maxdeg_plus_1, off = 0;
  uint32_t round = 0;
  FoldArgs fa = fold_args(pl, n);
  fa.batch = batch;
  FriSampleArgs sa;
  memset(&sa, 0, sizeof sa);
  sa.batch = batch;
  sa.exclude = exclude;
  sa.ys = fb.ys;
  sa.proof = d_proof;
  sa.proof_stride = stride;
  uint32_t ys_off = 0;
  while (md > 16) {  // at most SHK_FRI_MAX_ROUNDS rounds: fri_validate has refused anything longer before the first launch
    const uint32_t s = round == 0 ? samples : 40;
    if (!have_tree) HIP_TRY(c, shk_merkelize(vals, false, nn, batch, tree, c->stream, false));  // m = merkelize(values), fri.py:224
    fa.values = vals;
    fa.nodes = tree;
    fa.column = next;
    fa.n = nn;
    fa.round_shift = 2 * round;
    HIP_TRY(c, shk_fri_fold_and_tree(fa, tree2, c->stream));                    // column and m2, fri.py:235-243
    // fri.py:246-254 (the 40 sampled rows and their 5 branches each): recorded, done for all rounds at the end
    const uint64_t lg = (uint64_t)ilog2(nn);
    FriRound& r = sa.r[round];
    r.values = vals;
    r.column = next;
    r.nodes_m = tree;
    r.nodes_m2 = tree2;
    r.n = nn;
    r.round_off = off;
    r.samples = s;
    r.ys_off = ys_off;
    r.work_begin = sa.work_total;
    sa.work_total += ((uint64_t)s * ((lg - 1) + 4 * (lg + 1)) + 1) * batch;
    ys_off += batch * s;
    off += 32 + (uint64_t)s * 32 * ((lg - 1) + 4 * (lg + 1));
    // Next round (fri.py:260-266): the reference inverse-transforms the column over root^4 and transforms it
    // back, which is the identity on the column; its tree m of round r+1 is this round's m2.  The column and its tree
    // stay where they are (the arenas), the round after writes behind them.
    vals = next;
    tree = tree2;
    next = next + (size_t)batch * (nn / 4);
    tree2 = tree2 + (size_t)batch * 2 * (nn / 4) * 8;
    have_tree = true;
    nn >>= 2;
    md >>= 2;
    ++round;
  }
  sa.rounds = round;
  sa.final_values = vals;  // fri.py:212-214
  sa.final_n = nn;
  sa.final_off = off;
  HIP_TRY(c, shk_fri_sample_and_gather_all(sa, c->stream));
  return SH_OK;
}
}  // namespace shk

extern "C" {

int sh_dev_merkelize(sh_ctx* c, const void* d_values, uint64_t n, uint32_t batch, void* d_nodes) {
  if (!c || !d_values || !d_nodes || !is_pow2(n) || n < 4 || batch == 0) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, shk_merkelize(d_values, false, n, batch, reinterpret_cast<uint32_t*>(d_nodes), c->stream));
  return SH_OK;
}
int sh_dev_fri_fold(sh_ctx* c, const void* d_values, const void* d_nodes, uint64_t n, uint32_t batch,
                    const uint8_t root[32], void* d_column) {
  if (!c || !d_values || !d_nodes || !d_column || !root || n < 4) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  NttPlan* pl = nullptr;
  SH_TRY(plan_for(c, root, n, false, &pl));
  FoldArgs fa = fold_args(pl, n);
  fa.values = reinterpret_cast<const fp*>(d_values);
  fa.nodes = reinterpret_cast<const uint32_t*>(d_nodes);
  fa.column = reinterpret_cast<fp*>(d_column);
  fa.batch = batch;
  HIP_TRY(c, shk_fri_fold(fa, c->stream));
  return SH_OK;
}
int sh_dev_fri_prove(sh_ctx* c, const void* d_coeffs, uint64_t n, const uint8_t root[32], uint64_t maxdeg_plus_1,
                     uint32_t exclude, uint32_t samples, uint32_t batch, void* d_proof) {
  if (!c || !root) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  return run_fri(c, reinterpret_cast<const fp*>(d_coeffs), n, root, maxdeg_plus_1, exclude, samples, batch,
                 reinterpret_cast<uint8_t*>(d_proof));
}

int sh_dev_fri_prove_coeffs(sh_ctx* c, const void* d_coeffs, uint64_t n_coeffs, uint64_t n, const uint8_t root[32],
                            uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, uint32_t batch, void* d_proof) {
  if (!c || !root || n_coeffs == 0 || n_coeffs > n) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  return run_fri(c, reinterpret_cast<const fp*>(d_coeffs), n, root, maxdeg_plus_1, exclude, samples, batch,
                 reinterpret_cast<uint8_t*>(d_proof), n_coeffs);
}

int sh_merkelize(sh_ctx* c, const uint8_t* leaves, uint64_t n, uint8_t* nodes) {
  if (!c || !leaves || !nodes || !is_pow2(n) || n < 4) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  void *w = nullptr, *t = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, (size_t)n * 32, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_TREE_A, (size_t)2 * n * 32, &t));
  SH_TRY(h2d(c, w, leaves, (size_t)n * 32));
  HIP_TRY(c, shk_merkelize(w, true, n, 1, reinterpret_cast<uint32_t*>(t), c->stream));
  return d2h(c, nodes, t, (size_t)2 * n * 32);
}

int sh_merkelize_packed(sh_ctx* c, const uint8_t* evals, uint64_t n, uint32_t k, uint8_t* nodes, uint8_t* leaves) {
  if (!c || !evals || !nodes || !leaves || !is_pow2(n) || n < 4 || k == 0) return SH_ERR_INVALID;
  HIP_TRY(c, hipSetDevice(c->device));
  void *w = nullptr, *t = nullptr, *l = nullptr;
  const size_t ebytes = (size_t)n * k * 32;
  SH_TRY(ws_get(c, sh_ctx::WS_WIRE, ebytes, &w));
  SH_TRY(ws_get(c, sh_ctx::WS_TREE_A, (size_t)2 * n * 32, &t));
  SH_TRY(ws_get(c, sh_ctx::WS_X, ebytes, &l));
  SH_TRY(h2d(c, w, evals, ebytes));
  HIP_TRY(c, shk_merkelize_packed(reinterpret_cast<const uint8_t*>(w), n, k, reinterpret_cast<uint8_t*>(l),
                                  reinterpret_cast<uint32_t*>(t), c->stream));
  SH_TRY(d2h(c, nodes, t, (size_t)n * 32));
  return d2h(c, leaves, l, ebytes);
}

int sh_fri_fold(sh_ctx* c, const uint8_t* values, uint64_t n, const uint8_t root[32], const uint8_t special_x[32],
                uint8_t* column) {
  if (!c || !values || !root || !special_x || !column || !is_pow2(n) || n < 4) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  NttPlan* pl = nullptr;
  SH_TRY(plan_for(c, root, n, false, &pl));
  fp* v = nullptr;
  SH_TRY(upload_padded(c, values, n, n, 1, sh_ctx::WS_X, &v));
  void *col = nullptr, *sx = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_COL_B, (size_t)(n / 4) * sizeof(fp), &col));
  SH_TRY(ws_get(c, sh_ctx::WS_MISC, 64, &sx));
  HIP_TRY(c, hipMemcpyAsync(sx, special_x, 32, hipMemcpyHostToDevice, c->stream));
  FoldArgs fa = fold_args(pl, n);
  fa.values = v;
  fa.special_x = reinterpret_cast<const uint32_t*>(sx);  // nodes stay null: the challenge is special_x
  fa.column = reinterpret_cast<fp*>(col);
  fa.batch = 1;
  HIP_TRY(c, shk_fri_fold(fa, c->stream));
  return download_wire(c, reinterpret_cast<fp*>(col), column, n / 4);
}

uint64_t sh_fri_proof_len(uint64_t n, uint64_t maxdeg_plus_1, uint32_t samples) {
  return fri_proof_len(n, maxdeg_plus_1, samples);
}

int sh_fri_prove(sh_ctx* c, const uint8_t* coeffs, uint64_t n_coeffs, uint64_t n, const uint8_t root[32],
                 uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* proof,
                 uint64_t proof_cap) {
  if (!c || !root || !proof || (n_coeffs && !coeffs) || batch == 0 || n_coeffs > n || !is_pow2(n)) return SH_ERR_INVALID;
  SH_TRY(enter(c));
  const uint64_t stride = fri_proof_len(n, maxdeg_plus_1, samples);
  if (proof_cap < stride * batch) return SH_ERR_TOO_SMALL;
  fp* x = nullptr;
  uint64_t n_short = 0;
  SH_TRY(upload_short(c, coeffs, n_coeffs, n, batch, sh_ctx::WS_X, &x, &n_short));
  void* dp = nullptr;
  SH_TRY(ws_get(c, sh_ctx::WS_PROOF, (size_t)stride * batch, &dp));
  SH_TRY(run_fri(c, x, n, root, maxdeg_plus_1, exclude, samples, batch, reinterpret_cast<uint8_t*>(dp), n_short));
  return d2h(c, proof, dp, (size_t)stride * batch);
}
}  // extern "C"
