// knobs.hpp -- the experiment knobs of the launch path and the plan choice that depends on them.  Host-only, plain C++
// (no HIP types): the library includes it, and tests/native/knobs_tsan.cpp compiles it with g++ -fsanitize=thread.
//
// Every STARKHIP_* variable that shapes a launch is read from the environment ONCE per process, inside std::call_once, into
// one immutable ShkKnobs; afterwards the launch path only reads that object.  Contexts on several host threads (include/
// starkhip.h: contexts are independent) therefore share no mutable state here.  (STARKHIP_LIB / STARKHIP_DEVICE are read by
// the Python binding, STARKHIP_PLAN_CACHE_MB gives a new context its initial plan budget.)
//
//   STARKHIP_NTT_RADICES="10,10"   log2 radices of the passes (digits 2..11, at most 4), for the sizes they sum to
//   STARKHIP_TILE_LOG=9|10|11      elements per tile (log2) of every pass of radix <= 2^8 (default 10; the first pass of a
//                                  long transform 11, ntt.hip); setting it switches that first-pass rule off
//   STARKHIP_TILE_LOG_BIG=10|11|12 the same for the radix 2^9 .. 2^11 passes (default 11)
//   STARKHIP_TILE_LOGS="11,10,10"  per pass 0, 1, 2, ... (9..12; 0 = the rules above)
//   STARKHIP_XCD_SWZ=0|1|2         workgroup -> tile mapping over the 8 XCDs (ntt_kernels.cuh:shk_launch_tile_kernel)
//   STARKHIP_TW2_MAX_LOG=k         row-major inter-pass twiddle tables up to 2^k entries (default 24), else the power-table lookup
//   STARKHIP_PLAN_CACHE_MB=m       initial plan-cache budget of a context
//   STARKHIP_NTT_NARROW_TILES=k    passes of at most k 1024-element tiles (and radix <= 2^10) run in the one-butterfly-per-thread form
//                                  (ntt_narrow_pass_kernel; default 256 = the CUs of the chip; 0 = never)
//   STARKHIP_WITNESS_GROUP=1|2|4|8|16  lanes per unit of the witness generator (witness.hip; default: chosen from the term table)
//   STARKHIP_WITNESS_SLICE=k       steps per witness dispatch (default: about 2^13 sequential products per dispatch, at least 1)
//                                  (over another modulus, modwitness.hip: about 2^12, modwitness_items.cuh; on packed 64-bit words,
//                                  mod64witness.hip: about 2^14, mod64witness_items.cuh).  Both apply to all three paths
//   STARKHIP_WITNESS_STORE=pass|inline  how the generic and the packed-word witness generator reach plain form: one closing pass over
//                                  the witness (default), or a conversion on the kernel's store path (modwitness_items.cuh,
//                                  mod64witness_items.cuh; tools/mod_witness_time.py, tools/mod64_witness_time.py)
//   STARKHIP_EVAL_PATH=direct|tree  the path of every sh_poly_eval call (default: chosen per call, poly_items.cuh:pe_direct_preferred)
//   STARKHIP_MODNTT_TILE_LOG=2..10 elements per tile (log2) of the generic transform (modntt_items.cuh; default 10): small values force
//                                  plans of many passes at small n (tests/test_gpu_modntt.py)
//   STARKHIP_MOD64_TILE_LOG=2..13  elements per tile (log2) of the packed-word transform (ntt64_items.cuh; default 12); the largest
//                                  radix log of a plan is t - min(4, t / 2) (tests/test_gpu_ntt64.py); 12 against 13:
//                                  tools/mod64_ntt_time.py, profiles/r12_mod64_ntt.json
// All of them exist for the parity tests over alternate plans (tests/test_gpu_parity.py::test_alternate_ntt_plans_parity,
// tools/stress_plans.py) and for A/B measurements; the defaults are the measured best.
#pragma once
#include <stdlib.h>

#include <mutex>
#include <string>

struct ShkKnobs {
  int tile_log = 10;         // passes of radix <= 2^8
  bool tile_forced = false;  // STARKHIP_TILE_LOG was given
  int tile_log_big = 11;     // passes of radix >= 2^9
  int tile_logs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int xcd_swz = 1;
  int tw2_max_log = 24;
  long plan_cache_mb = -1;   // -1: not given
  int n_radices = 0;         // 0: not given (or malformed)
  int radices[4] = {0, 0, 0, 0};
  int radix_sum = 0;
  long narrow_tiles = 256;   // 0: the narrow form is never used
  int witness_group = 0;     // 0: not given
  long witness_slice = 0;    // 0: not given
  bool witness_inline = false;  // generic witness generator: convert on the store path instead of in a closing pass
  int eval_path = 0;         // 0: chosen per call, 1: direct, 2: tree
  int modntt_tile_log = 10;  // generic transform: 2 .. 10
  int mod64_tile_log = 12;   // packed-word transform: 2 .. 13
};

namespace shk_knobs_detail {
inline void parse_list(const char* e, int* out, int n, long lo, long hi, int dflt) {
  int i = 0;
  for (const char* p = e; p && *p && i < n; ++i) {
    char* end = nullptr;
    const long x = strtol(p, &end, 10);
    if (end == p) break;
    out[i] = (x >= lo && x <= hi) ? (int)x : dflt;
    p = (*end == ',') ? end + 1 : end;
  }
}
inline void parse(ShkKnobs* k) {
  if (const char* e = getenv("STARKHIP_TILE_LOG")) {
    const int v = atoi(e);
    k->tile_forced = true;
    if (v == 9 || v == 10 || v == 11) k->tile_log = v;
  }
  if (const char* e = getenv("STARKHIP_TILE_LOG_BIG")) {
    const int v = atoi(e);
    if (v == 10 || v == 11 || v == 12) k->tile_log_big = v;
  }
  parse_list(getenv("STARKHIP_TILE_LOGS"), k->tile_logs, 8, 9, 12, 0);
  if (const char* e = getenv("STARKHIP_XCD_SWZ")) {
    const int v = atoi(e);
    k->xcd_swz = (v < 0 || v > 2) ? 0 : v;
  }
  if (const char* e = getenv("STARKHIP_TW2_MAX_LOG")) {
    const int v = atoi(e);
    k->tw2_max_log = v < 0 ? 0 : v > 28 ? 28 : v;
  }
  if (const char* e = getenv("STARKHIP_PLAN_CACHE_MB")) {
    const long v = atol(e);
    if (v >= 0) k->plan_cache_mb = v;
  }
  if (const char* e = getenv("STARKHIP_NTT_NARROW_TILES")) {
    const long v = atol(e);
    k->narrow_tiles = v < 0 ? 0 : v;
  }
  if (const char* e = getenv("STARKHIP_WITNESS_GROUP")) {
    const int v = atoi(e);
    if (v == 1 || v == 2 || v == 4 || v == 8 || v == 16) k->witness_group = v;
  }
  if (const char* e = getenv("STARKHIP_WITNESS_SLICE")) {
    const long v = atol(e);
    if (v > 0) k->witness_slice = v;
  }
  if (const char* e = getenv("STARKHIP_WITNESS_STORE")) k->witness_inline = std::string(e) == "inline";
  if (const char* e = getenv("STARKHIP_EVAL_PATH")) {
    const std::string v(e);
    k->eval_path = v == "direct" ? 1 : v == "tree" ? 2 : 0;
  }
  if (const char* e = getenv("STARKHIP_MODNTT_TILE_LOG")) {
    const int v = atoi(e);
    if (v >= 2 && v <= 10) k->modntt_tile_log = v;
  }
  if (const char* e = getenv("STARKHIP_MOD64_TILE_LOG")) {
    const int v = atoi(e);
    if (v >= 2 && v <= 13) k->mod64_tile_log = v;
  }
  if (const char* e = getenv("STARKHIP_NTT_RADICES")) {
    int r[4] = {0, 0, 0, 0}, cnt = 0, sum = 0;
    bool ok = true;
    for (const char* p = e; *p && ok;) {
      char* end = nullptr;
      const long v = strtol(p, &end, 10);
      if (end == p || v < 2 || v > 11 || cnt == 4) {
        ok = false;
        break;
      }
      r[cnt++] = (int)v;
      sum += (int)v;
      if (*end && *end != ',') ok = false;
      p = (*end == ',') ? end + 1 : end;
    }
    if (ok && cnt >= 1) {
      k->n_radices = cnt;
      k->radix_sum = sum;
      for (int i = 0; i < 4; ++i) k->radices[i] = r[i];
    }
  }
}
}  // namespace shk_knobs_detail

inline const ShkKnobs& shk_knobs() {
  static ShkKnobs knobs;
  static std::once_flag once;
  std::call_once(once, [] { shk_knobs_detail::parse(&knobs); });
  return knobs;
}

// ---- which kernel a pass runs in ("cell") ------------------------------------------------------------------------------------------
// One instantiation of the pass kernels of ntt_kernels.cuh is named by (form, tile_log, log_R, LAST): ntt_pass_kernel<log_R,
// tile_log - log_R, LAST> (SHK_NTT_TILE) or ntt_narrow_pass_kernel<log_R, tile_log - log_R, LAST> (SHK_NTT_NARROW).  xcd: the launch
// maps adjacent tiles to the same XCD (tile form only; a property of the launch, not of the instantiation).
enum { SHK_NTT_NONE = -1, SHK_NTT_TILE = 0, SHK_NTT_NARROW = 1 };
struct ShkNttCell {
  int form;
  int tile_log;
  bool xcd;
};
// what the choice depends on, out of NttPassArgs (internal.hpp)
struct ShkNttPassShape {
  unsigned long long total;  // columns or rows of the launch
  unsigned log_n, log_S, pass_index;
};
// narrow passes of at most this many 1024-element tiles run as 512-element tiles of 256 threads (radix <= 2^8)
#ifndef SHK_NARROW_HALF_TILES
#define SHK_NARROW_HALF_TILES 128
#endif

// The instantiations that exist; ntt.hip compiles exactly these (shk_launch_ntt_cell).  Tile form: 2048-element tiles for every
// radix, 1024 up to radix 2^10, 512 up to 2^8 (a thread holds four elements of at least one row: log_R <= tile_log), 4096 from
// radix 2^4 (STARKHIP_TILE_LOGS = 12 has always been ignored below that; the two kernels per LAST that used to be compiled for
// radix 2^2 and 2^3 could not be launched).  Narrow form: 1024 elements up to radix 2^10, 512 up to 2^8.
constexpr bool shk_ntt_cell_exists(int form, int tile_log, int log_R) {
  if (log_R < 2 || log_R > 11) return false;
  if (form == SHK_NTT_NARROW) return tile_log == 10 ? log_R <= 10 : tile_log == 9 && log_R <= 8;
  if (form != SHK_NTT_TILE) return false;
  return tile_log == 12 ? log_R >= 4 : tile_log == 11 ? true : tile_log == 10 ? log_R <= 10 : tile_log == 9 && log_R <= 8;
}

// The cell of one pass (radix 2^log_R, row pass when last) under the knobs kn.  form SHK_NTT_NONE: no such radix.
//   narrow form: at most kn.narrow_tiles 1024-element tiles, radix <= 2^10, and no tile size forced for this pass (STARKHIP_TILE_LOGS);
//       up to SHK_NARROW_HALF_TILES of them and radix <= 2^8: 512-element tiles -- the launch then has at most one wave per SIMD.
//   else tile form.  Radix <= 2^8: the pass's STARKHIP_TILE_LOGS entry (4096 from radix 2^4 only, else it is ignored); else 2048 for
//       the FIRST column pass of a long transform (P = 1, radix 2^8, n / R >= 2^16) unless STARKHIP_TILE_LOG is given: twice the
//       columns per row are worth + 3.6 % on a 2^24-point transform (profiles/r03_first_pass_tile_2p24.txt), below that distance
//       and at radix 2^7 the 1024-element tiles stay ahead; else STARKHIP_TILE_LOG (default 1024).
//       Radix >= 2^9 (the two-pass plans of 2^17 .. 2^20 points): the pass's STARKHIP_TILE_LOGS entry when it is 10 .. 12 (1024 up to
//       radix 2^10 only), else STARKHIP_TILE_LOG_BIG under the same limit (default 2048: 64 KiB, two workgroups per CU).
//   xcd (ntt_kernels.cuh: shk_launch_tile_kernel): from 64 tiles up, when STARKHIP_XCD_SWZ is 2, or 1 and a tile has fewer than 4 columns.
inline ShkNttCell shk_ntt_choose_cell(const ShkKnobs& kn, int log_R, bool last, const ShkNttPassShape& a) {
  if (log_R < 2 || log_R > 11) return {SHK_NTT_NONE, 0, false};
  const int f = a.pass_index < 8 ? kn.tile_logs[a.pass_index] : 0;
  if (log_R <= 10) {
    const int log_T = 10 - log_R;
    const unsigned long long tiles = (a.total + ((1ull << log_T) - 1)) >> log_T;
    if (kn.narrow_tiles > 0 && tiles != 0 && tiles <= (unsigned long long)kn.narrow_tiles && !f)
      return {SHK_NTT_NARROW, (log_R <= 8 && tiles <= SHK_NARROW_HALF_TILES) ? 9 : 10, false};
  }
  int tl;
  if (log_R <= 8) {
    if ((f == 12 && log_R >= 4) || f == 11 || f == 10 || f == 9) tl = f;
    else if (!last && log_R == 8 && a.log_S + 8 == a.log_n && a.log_S >= 16 && !kn.tile_forced) tl = 11;
    else tl = kn.tile_log == 10 ? 10 : kn.tile_log == 9 ? 9 : 11;
  } else {
    if (f == 12 || f == 11 || (f == 10 && log_R <= 10)) tl = f;
    else if (log_R <= 10 && kn.tile_log_big == 10) tl = 10;
    else tl = kn.tile_log_big <= 11 ? 11 : 12;
  }
  const int log_t = tl - log_R;
  const unsigned long long tiles = (a.total + ((1ull << log_t) - 1)) >> log_t;
  return {SHK_NTT_TILE, tl, kn.xcd_swz && (kn.xcd_swz == 2 || log_t < 2) && tiles >= 64};
}

// The passes of a 2^log_n-point transform: log2 radices into out[0..4), returns their number.
//   n <= 2^8: one pass.  2^9 .. 2^16: two passes of 1024-element tiles.  2^17 .. 2^20: two passes of radix 2^8 .. 2^10 over
//   2048-element tiles -- (9, 8), (9, 9), (9, 10), (10, 10) -- measured ahead of three passes there (one inter-pass twiddle
//   product and one read + write of the vector fewer; 2^20: 12.3 / 15.5 / 16.5 against 10.6 / 15.2 / 15.9 G elements/s at
//   1 / 8 / 32 vectors).  From 2^21 up: ceil(log_n / 8) passes of near-equal radix <= 2^8 (two-pass plans measured behind).
inline int shk_choose_radices(int log_n, int out[4]) {
  const ShkKnobs& k = shk_knobs();
  if (k.n_radices && k.radix_sum == log_n) {
    for (int i = 0; i < k.n_radices; ++i) out[i] = k.radices[i];
    return k.n_radices;
  }
  if (log_n <= 8) {
    out[0] = log_n;
    return 1;
  }
  if (log_n >= 17 && log_n <= 20) {
    out[0] = log_n == 20 ? 10 : 9;
    out[1] = log_n - out[0];
    return 2;
  }
  const int m = (log_n + 7) / 8, base = log_n / m, rem = log_n % m;
  if (m > 4) return 0;
  for (int i = 0; i < m; ++i) out[i] = base + (i < rem ? 1 : 0);
  return m;
}
