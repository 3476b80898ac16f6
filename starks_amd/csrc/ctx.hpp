// ctx.hpp -- host-only internals of libstarkhip.so: the context, the plan cache and every helper that more than one of the host files
// (ctx.hip, api_*.hip) uses.  Kernel translation units include internal.hpp, never this header.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <utility>
#include <string>
#include <vector>

#include "../../include/starkhip.h"
#include "internal.hpp"
#include "knobs.hpp"
#include "verify_items.cuh"
#include "witness_items.cuh"
#include "modwitness_items.cuh"
#include "mod64witness_items.cuh"

// witness.hip
hipError_t shk_stark_witness_slice(const WitnessArgs& a, uint32_t width, hipStream_t st);
// modwitness.hip: rows [a.k0, a.k1) over M (inl: convert on the store path); the closing Montgomery -> plain pass of the default form
hipError_t shk_mod_witness_slice(const ModWitnessArgs& a, const fpm_mod& M, uint32_t width, bool inl, hipStream_t st);
hipError_t shk_mod_witness_finish(fpm* wit, uint64_t count, const fpm_mod& M, hipStream_t st);
// mod64witness.hip: their twins on packed 64-bit words
hipError_t shk_mod64_witness_slice(const Mod64WitnessArgs& a, const f64_mod& M, uint32_t width, bool inl, hipStream_t st);
hipError_t shk_mod64_witness_finish(uint64_t* wit, uint64_t count, const f64_mod& M, hipStream_t st);
// verify_dev.hip
hipError_t shk_verify_batch(const VbPlan& p, const uint8_t* proofs, uint32_t batch, const uint8_t* roots, const fp* inputs,
                            const fp* outputs, uint64_t io_stride, const fp* coef, const uint8_t* exps, uint32_t row,
                            const uint32_t* tbegin, uint32_t* ys, uint32_t* flags, int32_t* status, hipStream_t st);

namespace shk {

// ---- plans ------------------------------------------------------------------------------------------
struct PowTable {  // g^e for e < order: lo[e & mask] * hi[e >> lb]; hi == nullptr when stored in full
  fp* lo = nullptr;
  fp* hi = nullptr;
  uint32_t lb = 0;
};

struct NttPlan {
  uint64_t n = 0;
  int log_n = 0;
  bool scaled = false;       // multiply by n^-1 (inverse transform)
  fp root;                   // effective root (already inverted for inverse transforms)
  std::vector<int> radix;    // log2 radix of each pass
  std::vector<const fp2*> wR;  // per pass: powers of root^(n/R), R/2 entries, as (w, w 2^128) pairs
  std::vector<fp*> tw2;      // per column pass: the same twiddles as rows, tw2[k * S + j2] = g^(j2 k) (null: table too large)
  std::vector<PowTable> tw;  // per column pass d: table of root^(P_d) (times n^-1 on pass 0 when scaled)
  PowTable base;             // unscaled table of root (sh_power_cycle, FRI fold)
  fp* scale = nullptr;       // n^-1 on the device (one-pass scaled plans)
  std::vector<void*> owned;  // device allocations to free
  size_t bytes = 0;          // sum of the owned allocations (plan-cache budget)
  uint64_t last_use = 0;     // ctx tick of the most recent lookup (LRU eviction)
};

}  // namespace shk

struct sh_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t io_in = nullptr, io_out = nullptr;  // copy streams of the pipelined host-buffer transforms (created on first use)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t io_ev = nullptr;  // orders sh_dev_download_async's copies behind the ctx stream
  std::string err;
  std::map<std::string, shk::NttPlan*> plans;
  // plan cache accounting: least-recently-used plans are evicted on entry of a public call once the tables held exceed
  // the byte budget (STARKHIP_PLAN_CACHE_MB, default 16 GiB of the 288 GB) or the plan count its cap
  size_t plan_bytes = 0, plan_budget = (size_t)16 << 30;
  uint64_t tick = 0, plans_built = 0, plans_evicted = 0;
  enum {
    WS_WIRE = 0, WS_X, WS_Y, WS_NTT, WS_TREE_A, WS_TREE_B, WS_COL_A, WS_COL_B, WS_MISC, WS_PROOF,
    WS_ST_TRACE, WS_ST_P, WS_ST_D, WS_ST_B, WS_ST_Q, WS_ST_SMALL, WS_ST_MTREE,
    WS_VB, WS_VB_IO,  // batch verifiers: sampled indices + per-proof flags; the host-buffer forms' uploads
    WS_INV,           // multi_inv / multi_interp_4: the tile products of the levels above the items
    WS_PA_TREE, WS_PA_1, WS_PA_2, WS_PA_3, WS_PA_4, WS_PA_5,  // polynomial arithmetic: the product tree, transforms, remainders
    WS_COUNT
  };
  void* ws[WS_COUNT] = {};
  size_t ws_cap[WS_COUNT] = {};
  // pinned staging for host <-> device copies of caller (pageable) buffers: two slots, double buffered
  uint8_t* pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_busy[2] = {false, false};
  // STARK prover state: 1/((x_i - 1)(x_i - x_last)) and 1/(omega^j - 1) per (steps, ext); the step-polynomial terms last
  // uploaded (and their partial derivatives); the constraint flag
  std::map<std::pair<uint64_t, uint32_t>, void*> inv_z2;  // the three domain tables of (steps, ext): [3][n] (shk_stark_domain_tables)
  std::map<std::pair<uint64_t, uint32_t>, void*> inv_omega;
  std::vector<uint8_t> terms_key;
  void* terms_dev = nullptr;   // [terms][derivative terms]: see TermLayout
  uint32_t terms_begin[SHK_STARK_MAX_WIDTH + 1] = {};
  uint32_t terms_degree = 0;
  // the generic prover's term image (api_modstark.hip), beside the MiMC path's: keyed by modulus plus term bytes
  std::vector<uint8_t> mod_terms_key;
  void* mod_terms_dev = nullptr;  // ModTermLayout
  uint32_t mod_terms_begin[SHK_STARK_MAX_WIDTH + 1] = {};
  // the packed-word prover's term image (api_mod64stark.hip), a buffer of its own: packed and generic calls over one system alternate
  // without re-uploading
  std::vector<uint8_t> mod64_terms_key;
  void* mod64_terms_dev = nullptr;  // Mod64TermLayout
  uint32_t mod64_terms_begin[SHK_STARK_MAX_WIDTH + 1] = {};
  uint32_t* bad_flag = nullptr;  // [bad_cap] per-proof constraint flags of the calls since the last sh_stark_status*
  uint32_t bad_cap = 0;
};

#define HIP_TRY(ctx, expr)                                                                   \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) {                                                                  \
      char buf_[256];                                                                        \
      snprintf(buf_, sizeof buf_, "%s at %s:%d", hipGetErrorString(e_), __FILE__, __LINE__); \
      (ctx)->err = buf_;                                                                     \
      return e_ == hipErrorOutOfMemory ? SH_ERR_NOMEM : SH_ERR_HIP;                          \
    }                                                                                        \
  } while (0)

#define SH_TRY(expr)              \
  do {                            \
    int rc_ = (expr);             \
    if (rc_ != SH_OK) return rc_; \
  } while (0)

// Everything below is shared between the host files.  It lives in one named namespace: the library is loaded into the same
// process as torch, where a global `enter`, `trim` or `h2d` of default visibility could be interposed.
namespace shk {

// ---- host field helpers (the same fp256.cuh code the device runs) -----------------------------------
inline fp h_from_wire(const uint8_t b[32]) {
  uint32_t w[8];
  memcpy(w, b, 32);
  return fp_canon(fp_from_wire_words(w));
}
inline void h_to_wire(const fp& a, uint8_t b[32]) {
  uint32_t w[8];
  fp_to_wire_words(fp_canon(a), w);
  memcpy(b, w, 32);
}
inline fp h_pow(fp a, uint64_t e) { return fp_pow_u64(a, e); }
inline fp h_pow_limbs(const fp& a, const uint32_t e[8]) {
  fp r = fp_one(), b = a;
  for (int i = 0; i < 256; ++i) {
    if ((e[i / 32] >> (i % 32)) & 1) r = fp_mul(r, b);
    b = fp_sqr(b);
  }
  return r;
}
inline fp h_inv(const fp& a) {  // a^(p-2); modp.py:71-79 uses extended Euclid, the residue is the same
  static const uint32_t e[8] = {0xffffffffu, 0xfffffea0u, 0xffffffffu, 0xffffffffu,
                                0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};  // p - 2
  return h_pow_limbs(a, e);
}
// 7^((p - 1) / 2^lg): the reference's choice of generator everywhere (stark.py:205, test_fft.py:120)
inline fp h_root_of_order_pow2(int lg) {
  const uint32_t pm1[8] = {0u, 0xfffffea1u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  uint32_t e[8];
  for (int i = 0; i < 8; ++i) {
    const int lo = i + lg / 32, sh = lg % 32;
    uint64_t v = lo < 8 ? pm1[lo] : 0;
    if (sh) v = (v >> sh) | ((uint64_t)(lo + 1 < 8 ? pm1[lo + 1] : 0) << (32 - sh));
    e[i] = (uint32_t)v;
  }
  return h_pow_limbs(fp_from_u32(7u), e);
}
inline int ilog2(uint64_t n) {
  int k = 0;
  while ((1ull << k) < n) ++k;
  return k;
}
inline bool is_pow2(uint64_t n) { return n && !(n & (n - 1)); }

// [a, a + na) and [b, b + nb) share a byte but are not the same buffer
inline bool partial_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 != b0 && a0 < b0 + nb && b0 < a0 + na;
}
// [a, a + na) and [b, b + nb) share a byte (empty ranges share none)
inline bool any_overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return na && nb && a0 < b0 + nb && b0 < a0 + na;
}

// ---- ctx.hip: workspaces, staged copies, entry, the plan cache ------------------------------------------
int ws_get(sh_ctx* c, int slot, size_t bytes, void** out);
bool host_is_pinned(const void* h);
int h2d(sh_ctx* c, void* d, const void* h, size_t bytes, bool staged = false);
int d2h(sh_ctx* c, void* h, const void* d, size_t bytes);
int enter(sh_ctx* c);
// The plan cache: c->plans maps a key to an NttPlan that owns its device tables (a generic-modulus table is such a plan too).
// plan_find bumps last_use on a hit and returns nullptr on a miss.  A miss builds the plan inside a PlanHolder: every exit
// before plan_commit (error codes AND the early returns of HIP_TRY / SH_TRY) frees what was built.  plan_commit takes the
// plan from the holder and registers it: last_use, plan_bytes, plans_built, plans[key].
NttPlan* plan_find(sh_ctx* c, const std::string& key);
struct PlanHolder {
  NttPlan* p = new NttPlan();
  PlanHolder() = default;
  PlanHolder(const PlanHolder&) = delete;
  ~PlanHolder();
};
int plan_alloc(sh_ctx* c, NttPlan* pl, size_t bytes, void** out);
NttPlan* plan_commit(sh_ctx* c, const std::string& key, PlanHolder* h);
int upload_padded(sh_ctx* c, const uint8_t* in, uint64_t n_in, uint64_t n, uint32_t batch, int slot, fp** out);
int upload_short(sh_ctx* c, const uint8_t* in, uint64_t n_in, uint64_t n, uint32_t batch, int slot, fp** out, uint64_t* n_short);
int download_wire(sh_ctx* c, const fp* d, uint8_t* out, uint64_t count);

// ---- api_ntt.hip ----------------------------------------------------------------------------------------
int get_plan(sh_ctx* c, const fp& root_eff, uint64_t n, bool scaled, NttPlan** out);
int plan_for(sh_ctx* c, const uint8_t root[32], uint64_t n, bool inverse, NttPlan** out);
int run_ntt(sh_ctx* c, NttPlan* pl, const fp* d_in, fp* d_out, uint32_t batch, uint64_t n_in = 0);

// ---- api_fri.hip ----------------------------------------------------------------------------------------
// vals / tree: round 0 (the evaluations and their tree); next / tree2: the arenas of the later rounds, round r >= 1 at element
// offset batch * (n/4 + n/16 + ... + n/4^(r-1)) -- every round's column and tree stay until the commit's single sampling +
// gather pass at the end.
struct FriBuffers {
  fp *vals, *next;
  uint32_t *tree, *tree2, *ys;
};
uint64_t fri_proof_len(uint64_t n, uint64_t maxdeg_plus_1, uint32_t samples);
int fri_validate(uint64_t n, uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples, const char** why = nullptr);
int fri_buffers(sh_ctx* c, uint64_t n, uint32_t batch, uint32_t samples, FriBuffers* b);
int fri_rounds(sh_ctx* c, NttPlan* pl, FriBuffers fb, uint64_t n, uint64_t maxdeg_plus_1, uint32_t exclude, uint32_t samples,
               uint32_t batch, uint8_t* d_proof, uint64_t stride, bool have_tree);

// ---- api_modntt.hip -------------------------------------------------------------------------------------
// everything the host derives from (modulus, root, n, direction) before a launch; nothing here touches the device
struct ModCall {
  fpm_mod M;
  fpm root_mont;  // the effective root (inverted for an inverse transform), Montgomery form
  fpm scale;      // plain form: 1, or n^-1 for an inverse
  int log_n;
};
// every check of a generic-modulus call, on the host; `who` opens the sh_last_error text
int mod_prepare(sh_ctx* c, const uint8_t modulus[32], const uint8_t root[32], uint64_t n, uint64_t batch, bool inverse, bool scaled,
                ModCall* mc, const char* who = "sh_mod_ntt");
// the table of (modulus, effective root, n): w^e in Montgomery form, e < n / 2, held in the plan cache
int mod_table(sh_ctx* c, const ModCall& mc, const fpm** out);
// src [batch][n_in] (wire form when wire_in) -> dst [batch][n] (wire form when wire_out); src may be dst when n_in == n
int mod_run(sh_ctx* c, const ModCall& mc, const fpm* tw, const void* src, uint64_t n_in, void* dst, uint32_t batch, bool wire_in,
            bool wire_out);

// ---- api_modfri.hip -------------------------------------------------------------------------------------
// the commit rounds over mc's modulus on the evaluations in fb.vals (tw = mod_table of the n-point forward transform); with have_tree
// the tree of round 0 is already in fb.tree.  The FRI-only entries pass have_tree = false and stride = fri_proof_len.
int modfri_rounds(sh_ctx* c, const ModCall& mc, const fpm* tw, FriBuffers fb, uint64_t n, uint64_t maxdeg_plus_1, uint32_t exclude,
                  uint32_t samples, uint32_t batch, uint8_t* d_proof, uint64_t stride, bool have_tree);

// ---- api_ntt64.hip --------------------------------------------------------------------------------------
// everything the host derives from (modulus, root, n, direction) before a packed-word launch; nothing here touches the device
struct Mod64Call {
  f64_mod M;
  uint64_t root_mont;  // the effective root (inverted for an inverse transform), Montgomery form
  uint64_t scale;      // plain form: 1, or n^-1 for an inverse
  int log_n;
};
// every check of a packed-word call, on the host; `who` opens the sh_last_error text
int mod64_prepare(sh_ctx* c, uint64_t modulus, uint64_t root, uint64_t n, uint64_t batch, bool inverse, bool scaled, Mod64Call* mc,
                  const char* who = "sh_mod64_ntt");
// the tables of (modulus, effective root, n) -- lo | hi | stw in one allocation, Montgomery form --, held in the plan cache
int mod64_table(sh_ctx* c, const Mod64Call& mc, const uint64_t** out);
// src [batch][n_in] -> dst [batch][n], any 64-bit words in, plain canonical words out; src may be dst when n_in == n
int mod64_run(sh_ctx* c, const Mod64Call& mc, const uint64_t* tab, const void* src, uint64_t n_in, void* dst, uint32_t batch);

// ---- api_mod64fri.hip -----------------------------------------------------------------------------------
// FriBuffers with 8-byte values: the same workspace slots, the tree arenas as they are there
struct Fri64Buffers {
  uint64_t *vals, *next;
  uint32_t *tree, *tree2, *ys;
};
int mod64fri_buffers(sh_ctx* c, uint64_t n, uint32_t batch, uint32_t samples, Fri64Buffers* b);
// the commit rounds over mc's modulus on the plain canonical words in fb.vals (tab = mod64_table of the n-point forward transform); with
// have_tree the tree of round 0 is already in fb.tree.  The FRI-only entries pass have_tree = false and stride = fri_proof_len.
int mod64fri_rounds(sh_ctx* c, const Mod64Call& mc, const uint64_t* tab, Fri64Buffers fb, uint64_t n, uint64_t maxdeg_plus_1,
                    uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* d_proof, uint64_t stride, bool have_tree);

// ---- modverify.hip --------------------------------------------------------------------------------------
// the host verifier behind sh_mod_fri_verify: serial, no context, no GPU
int mod_fri_verify(const uint8_t modulus[32], const uint8_t* proof, uint64_t proof_len, const uint8_t merkle_root[32], uint64_t n,
                   const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude_multiples_of, uint32_t samples);

// the host verifier behind sh_mod_stark_verify (stark.py:281-388 over IntegersModP(p)): serial, no context, no GPU
int mod_stark_verify(const uint8_t modulus[32], const uint8_t* proof, uint64_t proof_len, const uint8_t* inputs, const uint8_t* outputs,
                     uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps,
                     const uint32_t* term_counts, uint32_t samples);

// ---- api_modstark.hip -----------------------------------------------------------------------------------
// Device layout of the step-polynomial description over a run-time modulus (one allocation, ctx->mod_terms_dev): TermLayout's, with
// Montgomery-form coefficients and exponent rows of `width` bytes (TermLayout's rows have width + 1)
struct ModTermLayout {
  static constexpr size_t MAXT = SHK_STARK_MAX_TERMS, MAXD = SHK_STARK_MAX_TERMS * SHK_STARK_MAX_WIDTH;
  static constexpr size_t coef = 0;                                    // fpm[MAXT]
  static constexpr size_t dcoef = coef + MAXT * sizeof(fpm);           // fpm[MAXD]
  static constexpr size_t exps = dcoef + MAXD * sizeof(fpm);           // u8[MAXT][width]
  static constexpr size_t dexps = exps + MAXT * SHK_STARK_MAX_WIDTH;   // u8[MAXD][width]
  static constexpr size_t dbegin = (dexps + MAXD * SHK_STARK_MAX_WIDTH + 3) & ~(size_t)3;  // u32[W * W + 1]
  static constexpr size_t total = dbegin + 4 * (SHK_STARK_MAX_WIDTH * SHK_STARK_MAX_WIDTH + 1);
};
// Parse + upload the step polynomials' terms over M into ctx->mod_terms_dev / mod_terms_begin; skipped when modulus and terms equal
// the previous generic call's, prover or verifier: a prove -> verify pair over one system uploads once.  total = the sum of counts.
int mod_stark_terms(sh_ctx* c, const fpm_mod& M, uint32_t width, const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts,
                    uint64_t total);

// ---- api_mod64stark.hip ---------------------------------------------------------------------------------
// ModTermLayout on packed words (one allocation, ctx->mod64_terms_dev): Montgomery-form coefficient words, exponent rows of `width` bytes
struct Mod64TermLayout {
  static constexpr size_t MAXT = SHK_STARK_MAX_TERMS, MAXD = SHK_STARK_MAX_TERMS * SHK_STARK_MAX_WIDTH;
  static constexpr size_t coef = 0;                                    // u64[MAXT]
  static constexpr size_t dcoef = coef + MAXT * sizeof(uint64_t);      // u64[MAXD]
  static constexpr size_t exps = dcoef + MAXD * sizeof(uint64_t);      // u8[MAXT][width]
  static constexpr size_t dexps = exps + MAXT * SHK_STARK_MAX_WIDTH;   // u8[MAXD][width]
  static constexpr size_t dbegin = (dexps + MAXD * SHK_STARK_MAX_WIDTH + 3) & ~(size_t)3;  // u32[W * W + 1]
  static constexpr size_t total = dbegin + 4 * (SHK_STARK_MAX_WIDTH * SHK_STARK_MAX_WIDTH + 1);
};

// ---- api_stark.hip --------------------------------------------------------------------------------------
// Device layout of the step-polynomial description (one allocation, ctx->terms_dev)
struct TermLayout {
  static constexpr size_t MAXT = SHK_STARK_MAX_TERMS, MAXD = SHK_STARK_MAX_TERMS * SHK_STARK_MAX_WIDTH;
  static constexpr size_t coef = 0;                                  // fp[MAXT]
  static constexpr size_t dcoef = coef + MAXT * sizeof(fp);          // fp[MAXD]
  static constexpr size_t ROW = SHK_STARK_MAX_WIDTH + 1;             // exponent rows: width bytes + 1 flag (coef == 1)
  static constexpr size_t exps = dcoef + MAXD * sizeof(fp);          // u8[MAXT][width + 1]
  static constexpr size_t dexps = exps + MAXT * ROW;                 // u8[MAXD][width + 1]
  static constexpr size_t dbegin = (dexps + MAXD * ROW + 3) & ~(size_t)3;  // u32[W * W + 1]
  static constexpr size_t total = dbegin + 4 * (SHK_STARK_MAX_WIDTH * SHK_STARK_MAX_WIDTH + 1);
};
int stark_terms(sh_ctx* c, uint32_t width, const uint8_t* coefs, const uint8_t* exps, const uint32_t* counts);
// the flat proof's bytes before the FRI part; the shape rule of both provers (degree = the step polynomials'); the per-proof flags
uint64_t stark_header_len(uint64_t n, uint32_t width, uint32_t samples);
int stark_check_shape(uint64_t steps, uint32_t ext, uint32_t width, uint32_t degree, uint32_t samples);
int bad_flags(sh_ctx* c, uint32_t batch);

}  // namespace shk
