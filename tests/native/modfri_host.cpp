// Host driver of tests/test_modfri_host.py: the FRI commit over a run-time modulus walked on the host exactly as api_modfri.hip issues
// it -- the transform through modntt_items.cuh, the leaf, fold and gather items of modfri_items.cuh over the grids the library launches,
// the upper tree levels with b2_hash_pair, the index sampler restated from utils.py:60-90 (the library's is the MiMC path's kernel).
//   prove <dir>   mod, in, cases (lines "log_n n_coeffs batch maxdeg_plus_1 exclude samples tile_log offset root": the case reads batch
//                 n_coeffs values of `in` from value `offset` on, root = 64 hex digits) -> out (the flat proofs, concatenated)
//                 exit 2: modulus rejected, 3: root rejected, 4: shape rejected
//   fold <dir> <log_n> <round_shift>   mod, root (of order n << round_shift), values (n wire values), sx (k challenges) -> out = k columns
//   tree <dir> <log_n> <batch>         values (batch n wire values, hashed as they are) -> out = batch trees of 2n nodes, leaf level included
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "modfri_items.cuh"

static std::vector<uint8_t> slurp(const std::string& path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return v;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}
static void spit(const std::string& path, const std::vector<uint8_t>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  fwrite(v.data(), 1, v.size(), f);
  fclose(f);
}

constexpr uint64_t WIDE_THREADS = 1ull << 19;  // modfri.hip: MF_WIDE_THREADS (the two forms are one function on the host)

// api_modntt.hip's mod_run: src wire form, dst plain limbs
static void transform(const fpm_mod& M, const fpm* tw, int log_n, int tile_log, const uint8_t* src, uint64_t n_in, fpm* dst, uint64_t batch) {
  const uint64_t n = 1ull << log_n;
  int radix[MN_MAX_PASSES];
  const int m = mn_plan(log_n, tile_log, radix);
  std::vector<fpm> work(batch * n), lds((size_t)1 << tile_log);
  for (int d = 0; d < m; ++d) {
    MnPass a = mn_pass(log_n, tile_log, radix, m, d, batch);
    a.tw = tw;
    a.src = d == 0 ? (const void*)src : (const void*)work.data();
    a.dst = d + 1 == m ? (void*)dst : (void*)work.data();
    if (d == 0) {
      a.n_in = n_in;
      a.wire_in = 1;
    }
    const uint64_t tiles = mn_tiles(a);
    for (uint64_t wg = 0; wg < tiles; ++wg) {
      for (uint32_t tid = 0; tid < MN_WG; ++tid) mn_load_item(a, M, wg, tid, lds.data());
      for (uint32_t s = 1; s <= a.log_R; ++s)
        for (uint32_t tid = 0; tid < MN_WG; ++tid) mn_stage_item(a, M, s, wg, tid, lds.data());
      for (uint32_t tid = 0; tid < MN_WG; ++tid) mn_store_item(a, M, wg, tid, lds.data());
    }
  }
}

// shk_merkle_upper_levels: levels log2(n) - 3 .. 0 from the nodes [n/4, n) the leaf kernels wrote
static void upper_levels(uint32_t* nodes, uint64_t n, uint64_t batch) {
  for (uint64_t b = 0; b < batch; ++b) {
    uint32_t* tree = nodes + b * 2 * n * 8;
    for (uint64_t i = n / 4 - 1; i >= 1; --i) {
      const b2digest d = b2_hash_pair(tree + 2 * i * 8, tree + (2 * i + 1) * 8);
      memcpy(tree + i * 8, d.h, 32);
    }
  }
}
static void leaves(const MfTree& t) {
  const uint64_t q = t.n >> 2, per_tree = (q + MF_WG - 1) / MF_WG;
  const bool wide = q * t.batch >= WIDE_THREADS;
  for (uint64_t blk = 0; blk < per_tree * t.batch; ++blk)
    for (uint32_t tid = 0; tid < MF_WG; ++tid) {
      const uint64_t b = blk / per_tree, i = (blk - b * per_tree) * MF_WG + tid;
      if (b < t.batch && i < q) wide ? mf_leaves_item<true>(t, b, i) : mf_leaves_item<false>(t, b, i);
    }
}
static void fold(const MfFold& a, const fpm_mod& M) {
  const uint64_t work = (a.n >> 2) * a.batch, blocks = (work + MF_WG - 1) / MF_WG;
  for (uint64_t g = 0; g < blocks * MF_WG; ++g)
    if (g < work) mf_fold_item(a, M, g);
}

// get_pseudorandom_indices (utils.py:60-90)
static void sample(const uint32_t* root, uint32_t modulus, uint32_t count, uint32_t exclude, uint32_t* ys) {
  std::vector<uint8_t> data(32);
  memcpy(data.data(), root, 32);
  while (data.size() < 4 * (size_t)count) {
    uint32_t m[16] = {};
    memcpy(m, data.data() + data.size() - 32, 32);
    const b2digest d = b2_hash_short(m, 32);
    data.insert(data.end(), reinterpret_cast<const uint8_t*>(d.h), reinterpret_cast<const uint8_t*>(d.h) + 32);
  }
  const uint32_t real = exclude ? (uint32_t)((uint64_t)modulus * (exclude - 1) / exclude) : modulus;
  for (uint32_t i = 0; i < count; ++i) {
    const uint8_t* p = data.data() + 4 * i;
    const uint32_t v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    const uint32_t x = v % real;
    ys[i] = exclude ? x + 1 + x / (exclude - 1) : x;
  }
}

static uint64_t proof_len(uint64_t n, uint64_t md, uint32_t samples) {  // api_fri.hip: fri_proof_len
  uint64_t total = 0;
  bool first = true;
  while (md > 16 && n >= 16) {
    uint64_t lg = 0;
    while ((1ull << lg) < n) ++lg;
    total += 32 + (uint64_t)(first ? samples : 40) * 32 * ((lg - 1) + 4 * (lg + 1));
    n >>= 2;
    md >>= 2;
    first = false;
  }
  return total + 32 * n;
}

static bool shape_ok(uint64_t n, uint64_t md, uint32_t exclude, uint32_t samples) {  // api_fri.hip: fri_validate
  uint32_t rounds = 0;
  bool first = true;
  while (md > 16) {
    if (++rounds > MF_MAX_ROUNDS || n < 16 || (n >> 2) >= (1ull << 24) || (first ? samples : 40) == 0 || exclude == 1) return false;
    if (exclude && ((n >> 2) * (exclude - 1)) / exclude == 0) return false;
    n >>= 2;
    md >>= 2;
    first = false;
  }
  return true;
}

// api_modfri.hip's modfri_run
static int prove(const fpm_mod& M, const fpm& root, int log_n, int tile_log, const uint8_t* coeffs, uint64_t n_coeffs, uint64_t md,
                 uint32_t exclude, uint32_t samples, uint32_t batch, std::vector<uint8_t>* out) {
  const uint64_t n = 1ull << log_n;
  if (!mn_check_root(root, n, M)) return 3;
  if (n_coeffs > n || batch == 0 || !shape_ok(n, md, exclude, samples)) return 4;
  const fpm root_mont = fpm_to_mont(root, M);
  MnTw t;
  mn_tw_args(root_mont, log_n, M, &t);
  std::vector<fpm> tw(t.count ? t.count : 1);
  t.tw = tw.data();
  for (uint64_t e = 0; e < t.count; ++e) mn_tw_item(t, M, e);
  // the arenas of fri_buffers
  std::vector<fpm> vals_a(batch * n), vals_b(batch * (n / 3 + 2));
  std::vector<uint32_t> tree_a(batch * 2 * n * 8), tree_b(batch * 2 * (n / 3 + 2) * 8);
  std::vector<uint32_t> ys_buf(batch * ((samples > 40 ? samples : 40) + 40 * MF_MAX_ROUNDS) + 16);
  transform(M, tw.data(), log_n, tile_log, coeffs, n_coeffs, vals_a.data(), batch);
  const uint64_t stride = proof_len(n, md, samples);
  std::vector<uint8_t> proof(stride * batch);
  fpm* vals = vals_a.data();
  fpm* next = vals_b.data();
  uint32_t* tree = tree_a.data();
  uint32_t* tree2 = tree_b.data();
  MfFold fa;
  memset(&fa, 0, sizeof fa);
  fa.tw = tw.data();
  fa.log_n0 = (uint32_t)log_n;
  if (n >= 4) fa.inv_i = fpm_pow(root_mont, 3 * (n / 4), M);
  fa.batch = batch;
  MfGather ga;
  memset(&ga, 0, sizeof ga);
  ga.batch = batch;
  ga.ys = ys_buf.data();
  ga.proof = proof.data();
  ga.proof_stride = stride;
  uint64_t nn = n, off = 0;
  uint32_t round = 0, ys_off = 0;
  while (md > 16) {
    const uint32_t s = round == 0 ? samples : 40;
    if (round == 0) {
      MfTree tr = {vals, tree, nn, batch, 0};
      leaves(tr);
      upper_levels(tree, nn, batch);
    }
    fa.values = vals;
    fa.nodes = tree;
    fa.column = next;
    fa.n = nn;
    fa.round_shift = 2 * round;
    fold(fa, M);
    MfTree tr2 = {next, tree2, nn / 4, batch, 0};
    leaves(tr2);
    upper_levels(tree2, nn / 4, batch);
    for (uint32_t b = 0; b < batch; ++b)  // fri_sample_all_kernel
      sample(tree2 + (uint64_t)b * 2 * (nn / 4) * 8 + 8, (uint32_t)(nn / 4), s, exclude, ys_buf.data() + ys_off + (uint64_t)b * s);
    uint64_t lg = 0;
    while ((1ull << lg) < nn) ++lg;
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
    vals = next;
    tree = tree2;
    next = next + (size_t)batch * (nn / 4);
    tree2 = tree2 + (size_t)batch * 2 * (nn / 4) * 8;
    nn >>= 2;
    md >>= 2;
    ++round;
  }
  ga.rounds = round;
  ga.final_values = vals;
  ga.final_n = nn;
  ga.final_off = off;
  const uint64_t work = ga.work_total + ga.final_n * batch, blocks = (work + MF_WG - 1) / MF_WG;
  for (uint64_t g = 0; g < blocks * MF_WG; ++g)
    if (g < work) mf_gather_item(ga, g);
  out->insert(out->end(), proof.begin(), proof.end());
  return 0;
}

static bool unhex(const char* hex, uint8_t out[32]) {
  if (strlen(hex) != 64) return false;
  for (int i = 0; i < 32; ++i) {
    unsigned v;
    if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  const std::string mode = argv[1], dir = std::string(argv[2]) + "/";
  std::vector<uint8_t> out;
  if (mode == "tree" && argc == 5) {
    const int log_n = atoi(argv[3]);
    const uint64_t n = 1ull << log_n, batch = strtoull(argv[4], nullptr, 10);
    const std::vector<uint8_t> vb = slurp(dir + "values");
    if (n < 4 || vb.size() != batch * n * 32) return 1;
    std::vector<fpm> v(batch * n);
    for (uint64_t i = 0; i < batch * n; ++i) v[i] = fpm_from_wire_bytes(&vb[32 * i]);
    std::vector<uint32_t> nodes(batch * 2 * n * 8);
    MfTree t = {v.data(), nodes.data(), n, (uint32_t)batch, 1};
    leaves(t);
    upper_levels(nodes.data(), n, batch);
    out.resize(nodes.size() * 4);
    memcpy(out.data(), nodes.data(), out.size());
    spit(dir + "out", out);
    return 0;
  }
  const std::vector<uint8_t> mod = slurp(dir + "mod");
  if (mod.size() != 32) return 1;
  fpm_mod M;
  if (!fpm_mod_init(mod.data(), &M)) return 2;
  if (mode == "prove") {
    const std::vector<uint8_t> in = slurp(dir + "in");
    FILE* f = fopen((dir + "cases").c_str(), "r");
    if (!f) return 1;
    int log_n, tile_log;
    unsigned long long n_coeffs, batch, md, offset;
    unsigned exclude, samples;
    char hex[65];
    int rc = 0;
    while (rc == 0 && fscanf(f, "%d %llu %llu %llu %u %u %d %llu %64s", &log_n, &n_coeffs, &batch, &md, &exclude, &samples, &tile_log,
                             &offset, hex) == 9) {
      uint8_t rb[32];
      if (in.size() < (offset + batch * n_coeffs) * 32 || !unhex(hex, rb)) {
        rc = 1;
        break;
      }
      rc = prove(M, fpm_from_wire_bytes(rb), log_n, tile_log, in.data() + offset * 32, n_coeffs, md, exclude, samples, (uint32_t)batch, &out);
    }
    fclose(f);
    if (rc) return rc;
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "fold" && argc == 5) {
    const int log_n = atoi(argv[3]);
    const uint32_t shift = (uint32_t)atoi(argv[4]);
    const uint64_t n = 1ull << log_n, n0 = n << shift;
    const std::vector<uint8_t> rootb = slurp(dir + "root"), vb = slurp(dir + "values"), sx = slurp(dir + "sx");
    if (rootb.size() != 32 || vb.size() != n * 32 || n < 4 || sx.size() % 32) return 1;
    const fpm root = fpm_from_wire_bytes(rootb.data());
    if (!mn_check_root(root, n0, M)) return 3;
    const fpm root_mont = fpm_to_mont(root, M);
    MnTw t;
    mn_tw_args(root_mont, log_n + (int)shift, M, &t);
    std::vector<fpm> tw(t.count);
    t.tw = tw.data();
    for (uint64_t e = 0; e < t.count; ++e) mn_tw_item(t, M, e);
    std::vector<fpm> col(n / 4);
    MfFold fa;
    memset(&fa, 0, sizeof fa);
    fa.values = reinterpret_cast<const fpm*>(vb.data());  // wire form, as sh_mod_fri_fold uploads it
    fa.column = col.data();
    fa.tw = tw.data();
    fa.n = n;
    fa.batch = 1;
    fa.log_n0 = (uint32_t)(log_n + (int)shift);
    fa.round_shift = shift;
    fa.wire_io = 1;
    fa.inv_i = fpm_pow(root_mont, 3 * (n0 / 4), M);
    for (size_t k = 0; k < sx.size(); k += 32) {
      fa.special_x = fpm_from_wire_bytes(&sx[k]);
      const uint64_t work = n / 4;
      fold(fa, M);
      const uint8_t* p = reinterpret_cast<const uint8_t*>(col.data());
      out.insert(out.end(), p, p + work * 32);
    }
    spit(dir + "out", out);
    return 0;
  }
  return 1;
}
