// Host driver of tests/test_mod64fri_host.py: the FRI commit on packed 64-bit words walked on the host exactly as api_mod64fri.hip
// issues it -- the transform through ntt64_items.cuh, the leaf, fold and gather items of mod64fri_items.cuh over the grids the library
// launches, the upper tree levels with b2_hash_pair, the index sampler restated from utils.py:60-90 (the library's is the MiMC path's
// kernel).  <p> and roots are decimal; values are native 8-byte words.
//   prove <dir> <p>   in, cases (lines "log_n n_coeffs batch maxdeg_plus_1 exclude samples tile_log offset root": the case reads batch
//                     n_coeffs words of `in` from word `offset` on) -> out (the flat proofs, concatenated)
//                     exit 2: modulus rejected, 3: root rejected, 4: shape rejected
//   fold <dir> <p> <log_n> <round_shift> <root>   root of order n << round_shift; values (n words, any 64-bit value), sx (k challenges
//                     of 32 big-endian bytes) -> out = k columns of n / 4 words
//   tree <dir> <p> <log_n> <batch>    values (batch n words, hashed as they are) -> out = batch trees of 2n nodes, leaf level included
// Every buffer an item reads or writes is a heap array of exactly the arena's size: an index outside it is caught by ASan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mod64fri_items.cuh"

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
static std::vector<uint64_t> slurp_words(const std::string& path) {
  const std::vector<uint8_t> v = slurp(path);
  std::vector<uint64_t> w(v.size() / 8);
  if (!w.empty()) memcpy(w.data(), v.data(), w.size() * 8);
  return w;
}
static void spit(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (bytes) fwrite(p, 1, bytes, f);
  fclose(f);
}

constexpr uint64_t WIDE_THREADS = 1ull << 19;  // mod64fri.hip: M6_WIDE_THREADS (the two forms are one function on the host)

// api_ntt64.hip's mod64_table: lo | hi | stw of (root, n) under the plan of tile_log
static std::vector<uint64_t> table(const f64_mod& M, uint64_t root_mont, int log_n, int tile_log) {
  std::vector<uint64_t> tab;
  if (!log_n) return tab;
  int radix[N64_MAX_PASSES];
  n64_plan(log_n, tile_log, radix);
  N64Tw t;
  n64_tw_args(root_mont, log_n, radix[0], M, &t);
  tab.resize(n64_table_entries(t));
  t.tab = tab.data();
  for (uint64_t i = 0; i < tab.size(); ++i) n64_tw_item(t, M, i);
  return tab;
}

// api_ntt64.hip's mod64_run, forward
static void transform(const f64_mod& M, uint64_t root_mont, const std::vector<uint64_t>& tab, int log_n, int tile_log, const uint64_t* src,
                      uint64_t n_in, uint64_t* dst, uint64_t batch) {
  const uint64_t n = 1ull << log_n;
  int radix[N64_MAX_PASSES];
  const int m = n64_plan(log_n, tile_log, radix);
  N64Tw t = {};
  if (log_n) n64_tw_args(root_mont, log_n, radix[0], M, &t);
  std::vector<uint64_t> work(m > 1 ? batch * n : 0);
  for (int d = 0; d < m; ++d) {
    N64Pass a = n64_pass(log_n, tile_log, radix, m, d, batch);
    a.lo = log_n ? tab.data() : nullptr;
    a.hi = log_n ? tab.data() + t.n_lo : nullptr;
    a.stw = log_n ? tab.data() + t.n_lo + t.n_hi : nullptr;
    a.src = d == 0 ? src : work.data();
    a.dst = d + 1 == m ? dst : work.data();
    if (d == 0) a.n_in = n_in;
    std::vector<uint64_t> lds(n64_tile_elems(a));
    const uint64_t tiles = n64_tiles(a);
    const uint32_t groups = n64_groups(a.log_R);
    for (uint64_t wg = 0; wg < tiles; ++wg) {
      for (uint32_t tid = 0; tid < N64_WG; ++tid) n64_load_item(a, M, wg, tid, lds.data());
      for (uint32_t g = 0; g < groups; ++g)
        for (uint32_t tid = 0; tid < N64_WG; ++tid) n64_group_any(a, M, g, wg, tid, lds.data());
      for (uint32_t tid = 0; tid < N64_WG; ++tid) n64_store_item(a, M, wg, tid, lds.data());
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
static void leaves(const M6Tree& t) {
  const uint64_t q = t.n >> 2, per_tree = (q + MF_WG - 1) / MF_WG;
  const bool wide = q * t.batch >= WIDE_THREADS;
  for (uint64_t blk = 0; blk < per_tree * t.batch; ++blk)
    for (uint32_t tid = 0; tid < MF_WG; ++tid) {
      const uint64_t b = blk / per_tree, i = (blk - b * per_tree) * MF_WG + tid;
      if (b < t.batch && i < q) wide ? m6_leaves_item<true>(t, b, i) : m6_leaves_item<false>(t, b, i);
    }
}
static void fold(const M6Fold& a, const f64_mod& M) {
  const uint64_t work = (a.n >> 2) * a.batch, blocks = (work + MF_WG - 1) / MF_WG;
  for (uint64_t g = 0; g < blocks * MF_WG; ++g)
    if (g < work) m6_fold_item(a, M, g);
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

// api_mod64fri.hip's fold_args
static M6Fold fold_args(const f64_mod& M, uint64_t root_mont, const std::vector<uint64_t>& tab, int log_n0) {
  M6Fold fa;
  memset(&fa, 0, sizeof fa);
  fa.log_n0 = (uint32_t)log_n0;
  fa.log_h = (uint32_t)n64_log_h(log_n0);
  fa.lo = tab.data();
  fa.hi = tab.data() + (1ull << fa.log_h);
  fa.inv_i = f64_pow(root_mont, 3 * ((1ull << log_n0) / 4), M);
  return fa;
}

// api_mod64fri.hip's mod64fri_run
static int prove(const f64_mod& M, uint64_t root, int log_n, int tile_log, const uint64_t* coeffs, uint64_t n_coeffs, uint64_t md,
                 uint32_t exclude, uint32_t samples, uint32_t batch, std::vector<uint8_t>* out) {
  const uint64_t n = 1ull << log_n;
  if (!n64_check_root(root, n, M)) return 3;
  if (n_coeffs > n || batch == 0 || !shape_ok(n, md, exclude, samples)) return 4;
  const uint64_t root_mont = f64_to_mont(root, M);
  const std::vector<uint64_t> tab = table(M, root_mont, log_n, tile_log);
  // the arenas of mod64fri_buffers
  std::vector<uint64_t> vals_a(batch * n), vals_b(batch * (n / 3 + 2));
  std::vector<uint32_t> tree_a(batch * 2 * n * 8), tree_b(batch * 2 * (n / 3 + 2) * 8);
  std::vector<uint32_t> ys_buf(batch * ((samples > 40 ? samples : 40) + 40 * MF_MAX_ROUNDS) + 16);
  const std::vector<uint64_t> src(coeffs, coeffs + batch * n_coeffs);  // exactly the words the case may read
  transform(M, root_mont, tab, log_n, tile_log, src.data(), n_coeffs, vals_a.data(), batch);
  const uint64_t stride = proof_len(n, md, samples);
  std::vector<uint8_t> proof(stride * batch);
  uint64_t* vals = vals_a.data();
  uint64_t* next = vals_b.data();
  uint32_t* tree = tree_a.data();
  uint32_t* tree2 = tree_b.data();
  M6Fold fa;
  memset(&fa, 0, sizeof fa);
  if (n >= 4) fa = fold_args(M, root_mont, tab, log_n);
  fa.batch = batch;
  M6Gather ga;
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
      M6Tree tr = {vals, tree, nn, batch, 0};
      leaves(tr);
      upper_levels(tree, nn, batch);
    }
    fa.values = vals;
    fa.nodes = tree;
    fa.column = next;
    fa.n = nn;
    fa.round_shift = 2 * round;
    fold(fa, M);
    M6Tree tr2 = {next, tree2, nn / 4, batch, 0};
    leaves(tr2);
    upper_levels(tree2, nn / 4, batch);
    for (uint32_t b = 0; b < batch; ++b)  // fri_sample_all_kernel
      sample(tree2 + (uint64_t)b * 2 * (nn / 4) * 8 + 8, (uint32_t)(nn / 4), s, exclude, ys_buf.data() + ys_off + (uint64_t)b * s);
    uint64_t lg = 0;
    while ((1ull << lg) < nn) ++lg;
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
    if (g < work) m6_gather_item(ga, g);
  out->insert(out->end(), proof.begin(), proof.end());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) return 1;
  const std::string mode = argv[1], dir = std::string(argv[2]) + "/";
  f64_mod M;
  if (!f64_mod_init(strtoull(argv[3], nullptr, 10), &M)) return 2;
  if (mode == "tree" && argc == 6) {
    const int log_n = atoi(argv[4]);
    const uint64_t n = 1ull << log_n, batch = strtoull(argv[5], nullptr, 10);
    const std::vector<uint64_t> v = slurp_words(dir + "values");
    if (n < 4 || v.size() != batch * n) return 1;
    std::vector<uint32_t> nodes(batch * 2 * n * 8);
    M6Tree t = {v.data(), nodes.data(), n, (uint32_t)batch, 1};
    leaves(t);
    upper_levels(nodes.data(), n, batch);
    spit(dir + "out", nodes.data(), nodes.size() * 4);
    return 0;
  }
  if (mode == "prove") {
    const std::vector<uint64_t> in = slurp_words(dir + "in");
    FILE* f = fopen((dir + "cases").c_str(), "r");
    if (!f) return 1;
    int log_n, tile_log;
    unsigned long long n_coeffs, batch, md, offset, root;
    unsigned exclude, samples;
    std::vector<uint8_t> out;
    int rc = 0;
    while (rc == 0 && fscanf(f, "%d %llu %llu %llu %u %u %d %llu %llu", &log_n, &n_coeffs, &batch, &md, &exclude, &samples, &tile_log,
                             &offset, &root) == 9) {
      if (in.size() < offset + batch * n_coeffs) {
        rc = 1;
        break;
      }
      rc = prove(M, root, log_n, tile_log, in.data() + offset, n_coeffs, md, exclude, samples, (uint32_t)batch, &out);
    }
    fclose(f);
    if (rc) return rc;
    spit(dir + "out", out.data(), out.size());
    return 0;
  }
  if (mode == "fold" && argc == 7) {
    const int log_n = atoi(argv[4]);
    const uint32_t shift = (uint32_t)atoi(argv[5]);
    const uint64_t n = 1ull << log_n, n0 = n << shift, root = strtoull(argv[6], nullptr, 10);
    const std::vector<uint64_t> v = slurp_words(dir + "values");
    const std::vector<uint8_t> sx = slurp(dir + "sx");
    if (v.size() != n || n < 4 || sx.size() % 32) return 1;
    if (!n64_check_root(root, n0, M)) return 3;
    const uint64_t root_mont = f64_to_mont(root, M);
    const std::vector<uint64_t> tab = table(M, root_mont, log_n + (int)shift, N64_DEFAULT_TILE_LOG);
    std::vector<uint64_t> col(n / 4), out;
    M6Fold fa = fold_args(M, root_mont, tab, log_n + (int)shift);
    fa.values = v.data();  // any 64-bit value, as sh_mod64_fri_fold uploads it
    fa.column = col.data();
    fa.n = n;
    fa.batch = 1;
    fa.round_shift = shift;
    fa.canon_in = 1;
    for (size_t k = 0; k < sx.size(); k += 32) {
      for (int i = 0; i < 8; ++i) {
        const uint8_t* b = &sx[k] + 4 * (7 - i);
        fa.special_x[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
      }
      fold(fa, M);
      out.insert(out.end(), col.begin(), col.end());
    }
    spit(dir + "out", out.data(), out.size() * 8);
    return 0;
  }
  return 1;
}
