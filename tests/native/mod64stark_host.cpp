// Host driver of tests/test_mod64stark_host.py: the STARK prover on packed 64-bit words walked on the host exactly as api_mod64stark.hip
// issues it -- the transforms through ntt64_items.cuh, the items of mod64stark_items.cuh over the grids mod64stark.hip launches, the trees
// of plain words and the commit rounds through mod64fri_items.cuh, the upper tree levels with b2_hash_pair, the index sampler restated
// from utils.py:60-90 (the library's is the MiMC path's kernel).  <p> is decimal; values are native 8-byte words.
//   prove <dir> <p>   cases (lines "steps ext width samples batch tile_log"), in (per case, in order: the witness [batch][width][steps]
//                     and the inputs [batch][width] as words, width counts as u32 little-endian, the terms' coefficients in 32-byte wire
//                     form, their exponent rows) -> out (the flat proofs, concatenated), flags (one byte per proof: its constraint flag)
//                     exit 2: modulus rejected, 3: G2 of the wrong order, 4: shape rejected
//   inv <dir> <p>     values (words below p) -> out = their inverses modulo p (words, 0 for 0) through m6s_batch_inv_item
// Every buffer an item reads or writes is a heap array of exactly the arena's size: an index outside it is caught by ASan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mod64stark_items.cuh"

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

// api_ntt64.hip's mod64_run: src [batch][n_in] -> dst [batch][n], the last pass times `scale` (plain); src may be dst when n_in == n
static void transform(const f64_mod& M, uint64_t root_mont, const std::vector<uint64_t>& tab, int log_n, int tile_log, uint64_t scale,
                      const uint64_t* src, uint64_t n_in, uint64_t* dst, uint64_t batch) {
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
    if (d + 1 == m) a.scale = scale;
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
// a launch of mod64stark.hip (and of mod64fri.hip's fold and gather): ceil(items / 256) workgroups of 256 threads, the kernel's guard
template <class F>
static void launch(uint64_t items, F&& body) {
  const uint64_t blocks = (items + M6S_WG - 1) / M6S_WG;
  for (uint64_t g = 0; g < blocks * M6S_WG; ++g)
    if (g < items) body(g);
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

static uint64_t fri_len(uint64_t n, uint64_t md, uint32_t samples) {  // api_fri.hip: fri_proof_len
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
static bool fri_shape_ok(uint64_t n, uint64_t md, uint32_t exclude, uint32_t samples) {  // api_fri.hip: fri_validate
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
static bool pow2(uint64_t x) { return x && !(x & (x - 1)); }
static bool shape_ok(uint64_t steps, uint32_t ext, uint32_t width, uint32_t degree, uint32_t samples) {  // api_stark.hip: stark_check_shape
  if (!pow2(steps) || !pow2(ext) || steps < 2 || ext < 2 || width == 0 || samples == 0 || width > M6S_MAX_WIDTH) return false;
  if (steps > (1ull << 24) || steps * ext >= (1ull << 24)) return false;
  if ((uint64_t)degree * (steps - 1) + 1 >= steps * ext) return false;
  return fri_shape_ok(steps * ext, steps * degree, ext, 40);
}

// api_mod64fri.hip's mod64fri_rounds with have_tree: the commit on vals_a / tree_a
static void fri_rounds(const f64_mod& M, uint64_t root_mont, const std::vector<uint64_t>& tab, int log_n, std::vector<uint64_t>& vals_a,
                       std::vector<uint32_t>& tree_a, uint64_t md, uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* proof,
                       uint64_t stride) {
  const uint64_t n = 1ull << log_n;
  std::vector<uint64_t> vals_b(batch * (n / 3 + 2));
  std::vector<uint32_t> tree_b(batch * 2 * (n / 3 + 2) * 8);
  std::vector<uint32_t> ys_buf(batch * ((samples > 40 ? samples : 40) + 40 * MF_MAX_ROUNDS) + 16);
  uint64_t* vals = vals_a.data();
  uint64_t* next = vals_b.data();
  uint32_t* tree = tree_a.data();
  uint32_t* tree2 = tree_b.data();
  M6Fold fa;
  memset(&fa, 0, sizeof fa);
  fa.log_n0 = (uint32_t)log_n;
  fa.log_h = (uint32_t)n64_log_h(log_n);
  fa.lo = tab.data();
  fa.hi = tab.data() + (1ull << fa.log_h);
  fa.inv_i = f64_pow(root_mont, 3 * (n / 4), M);
  fa.batch = batch;
  M6Gather ga;
  memset(&ga, 0, sizeof ga);
  ga.batch = batch;
  ga.ys = ys_buf.data();
  ga.proof = proof;
  ga.proof_stride = stride;
  uint64_t nn = n, off = 0;
  uint32_t round = 0, ys_off = 0;
  while (md > 16) {
    const uint32_t s = round == 0 ? samples : 40;
    fa.values = vals;
    fa.nodes = tree;
    fa.column = next;
    fa.n = nn;
    fa.round_shift = 2 * round;
    launch((nn >> 2) * batch, [&](uint64_t g) { m6_fold_item(fa, M, g); });
    M6Tree tr2 = {next, tree2, nn / 4, batch, 0};
    leaves(tr2);
    upper_levels(tree2, nn / 4, batch);
    for (uint32_t b = 0; b < batch; ++b)
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
  launch(ga.work_total + ga.final_n * batch, [&](uint64_t g) { m6_gather_item(ga, g); });
}

template <int W>
static void quotients(const M6sArgs& a, const f64_mod& M) {
  launch(a.steps * a.batch, [&](uint64_t g) { m6s_trace_item<W>(a, M, g); });
  launch(a.n * a.batch, [&](uint64_t g) { m6s_quot_item<W>(a, M, g / a.n, g & (a.n - 1)); });
}

// api_mod64stark.hip's run_mod64_stark
static int prove(const f64_mod& M, uint64_t steps, uint32_t ext, uint32_t width, uint32_t samples, uint32_t batch, int tile_log,
                 const uint64_t* wit_words, const uint64_t* in_words, const uint32_t* counts, const uint8_t* coefs, const uint8_t* exps,
                 uint64_t total, std::vector<uint8_t>* out, std::vector<uint8_t>* flags) {
  if (total == 0 || total > M6S_MAX_TERMS || batch == 0) return 4;
  const uint32_t degree = m6s_terms_degree(exps, width, total);
  if (!shape_ok(steps, ext, width, degree, samples)) return 4;
  const uint64_t n = steps * ext, cols = (uint64_t)batch * width;
  int log_n = 0, log_s = 0;
  while ((1ull << log_n) < n) ++log_n;
  while ((1ull << log_s) < steps) ++log_s;
  const uint64_t g2 = m6s_g2(M, log_n);
  if (!n64_check_root(f64_from_mont(g2, M), n, M)) return 3;
  const uint64_t g1 = f64_pow(g2, ext, M), g1_inv = f64_pow(g1, steps - 1, M);
  const uint64_t x_last = f64_pow(g2, (steps - 1) * ext, M);
  const uint64_t inv_last_m1 = f64_pow(f64_sub(x_last, M.one, M), M.p - 2, M);
  const uint64_t cpow = f64_pow(f64_pow(g2, steps, M), n - 1, M);
  const uint64_t inv_steps = n64_inv_n(log_s, M);
  // the term image
  std::vector<uint64_t> cf(total), dcf(total * width + 1);
  std::vector<uint8_t> ex(total * width), dex(total * width * width + 1);
  std::vector<uint32_t> dbeg(width * width + 1);
  M6sArgs a;
  memset(&a, 0, sizeof a);
  m6s_terms_build(M, width, coefs, exps, counts, total, cf.data(), dcf.data(), ex.data(), dex.data(), dbeg.data(), a.term_begin);
  // the upload: the words as they are
  std::vector<uint64_t> wit(wit_words, wit_words + cols * steps), inputs(in_words, in_words + cols);
  // the transforms' tables and the domain tables
  const std::vector<uint64_t> tab_n = table(M, g2, log_n, tile_log), tab_is = table(M, g1_inv, log_s, tile_log),
                              tab_fs = table(M, g1, log_s, tile_log);
  std::vector<uint64_t> den(2 * n), tables(3 * n);
  M6sTables mt;
  memset(&mt, 0, sizeof mt);
  mt.den = den.data();
  mt.table = tables.data();
  mt.log_h = (uint32_t)n64_log_h(log_n);
  mt.lo = tab_n.data();
  mt.hi = tab_n.data() + (1ull << mt.log_h);
  mt.n = n;
  mt.steps = steps;
  mt.ext = ext;
  mt.x_last = x_last;
  launch(n, [&](uint64_t i) { m6s_den_item(mt, M, i); });
  M6sInv inv;
  inv.in = den.data();
  inv.out = tables.data();
  inv.count = 2 * n;
  inv.chunks = (inv.count + M6S_INV_CHUNK - 1) / M6S_INV_CHUNK;
  launch(inv.chunks, [&](uint64_t g) { m6s_batch_inv_item(inv, M, g); });
  launch(n, [&](uint64_t i) { m6s_tables_item(mt, M, i); });

  std::vector<uint64_t> P(cols * n), D(cols * n), B(cols * n), Q(cols * steps), iab(cols * 2), scal(cols * 3), l(batch * n);
  std::vector<uint32_t> bad(batch, 0), mtree(batch * 2 * n * 8), ltree(batch * 2 * n * 8), ys(batch * samples);
  a.p_evals = P.data();
  a.d_work = D.data();
  a.b_work = B.data();
  a.q_evals = Q.data();
  a.wit = wit.data();
  a.inputs = inputs.data();
  a.iab = iab.data();
  a.n = n;
  a.steps = steps;
  a.ext = ext;
  a.width = width;
  a.batch = batch;
  a.inv_z2 = tables.data();
  a.fz = tables.data() + n;
  a.xpow = tables.data() + 2 * n;
  a.x_last = x_last;
  a.g1 = g1;
  a.inv_last_m1 = inv_last_m1;
  a.inv_1_m_last = f64_neg(inv_last_m1, M);
  a.inv_steps = inv_steps;
  a.bad = bad.data();
  a.term_coef = cf.data();
  a.term_exps = ex.data();
  a.dterm_coef = dcf.data();
  a.dterm_exps = dex.data();
  a.dterm_begin = dbeg.data();

  launch(cols, [&](uint64_t col) { m6s_interp_item(a, M, col); });
  transform(M, g1_inv, tab_is, log_s, tile_log, inv_steps, wit.data(), steps, Q.data(), cols);
  transform(M, g2, tab_n, log_n, tile_log, 1, Q.data(), steps, P.data(), cols);
  launch(cols * steps, [&](uint64_t g) { m6s_qprep_item(Q.data(), Q.data(), steps, g, M); });
  transform(M, g1, tab_fs, log_s, tile_log, 1, Q.data(), steps, Q.data(), cols);
  switch (width) {
    case 1: quotients<1>(a, M); break;
    case 2: quotients<2>(a, M); break;
    case 3: quotients<3>(a, M); break;
    case 4: quotients<4>(a, M); break;
    case 5: quotients<5>(a, M); break;
    case 6: quotients<6>(a, M); break;
    case 7: quotients<7>(a, M); break;
    case 8: quotients<8>(a, M); break;
    case 9: quotients<9>(a, M); break;
    default: return 4;
  }
  launch((n >> 2) * batch, [&](uint64_t g) { m6s_leaf_row_item<false>(a, mtree.data(), g / (n >> 2), g & ((n >> 2) - 1)); });
  upper_levels(mtree.data(), n, batch);
  for (uint64_t blk = 0; blk < (batch + 63) / 64; ++blk)
    for (uint32_t tid = 0; tid < 64; ++tid)
      if (blk * 64 + tid < batch) m6s_scalars_item(mtree.data(), 2 * n * 8, width, cpow, scal.data(), blk * 64 + tid, M);
  launch(n * batch, [&](uint64_t g) { m6s_lincomb_item(a, scal.data(), l.data(), M, g / n, g & (n - 1)); });
  M6Tree lt = {l.data(), ltree.data(), n, batch, 0};
  leaves(lt);
  upper_levels(ltree.data(), n, batch);
  for (uint32_t b = 0; b < batch; ++b)
    sample(ltree.data() + (uint64_t)b * 2 * n * 8 + 8, (uint32_t)n, samples, ext, ys.data() + (uint64_t)b * samples);
  const uint64_t header = 64 + (uint64_t)samples * 32 * (2 * (6 * width + (log_n - 1)) + (log_n + 1));
  const uint64_t stride = header + fri_len(n, steps * (uint64_t)degree, 40);
  std::vector<uint8_t> proof(stride * batch);
  M6sGather ga;
  memset(&ga, 0, sizeof ga);
  ga.mnodes = mtree.data();
  ga.lnodes = ltree.data();
  ga.lvals = l.data();
  ga.ys = ys.data();
  ga.samples = samples;
  ga.lg = (uint32_t)log_n;
  ga.proof = proof.data();
  ga.stride = stride;
  launch(m6s_gather_per_proof(width, samples, ga.lg) * batch, [&](uint64_t g) { m6s_gather_item(a, ga, g); });
  fri_rounds(M, g2, tab_n, log_n, l, ltree, steps * (uint64_t)degree, ext, 40, batch, proof.data() + header, stride);
  out->insert(out->end(), proof.begin(), proof.end());
  for (uint32_t b = 0; b < batch; ++b) flags->push_back(bad[b] ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) return 1;
  const std::string mode = argv[1], dir = std::string(argv[2]) + "/";
  f64_mod M;
  if (!f64_mod_init(strtoull(argv[3], nullptr, 10), &M)) return 2;
  if (mode == "inv") {
    const std::vector<uint8_t> vb = slurp(dir + "values");
    if (vb.size() % 8) return 1;
    const uint64_t count = vb.size() / 8;
    std::vector<uint64_t> in(count), res(count);
    if (count) memcpy(in.data(), vb.data(), vb.size());
    for (uint64_t i = 0; i < count; ++i) in[i] = f64_to_mont(in[i], M);
    M6sInv inv;
    inv.in = in.data();
    inv.out = res.data();
    inv.count = count;
    inv.chunks = (count + M6S_INV_CHUNK - 1) / M6S_INV_CHUNK;
    launch(inv.chunks, [&](uint64_t g) { m6s_batch_inv_item(inv, M, g); });
    for (uint64_t i = 0; i < count; ++i) res[i] = f64_from_mont(res[i], M);
    spit(dir + "out", res.data(), count * 8);
    return 0;
  }
  if (mode == "prove") {
    const std::vector<uint8_t> in = slurp(dir + "in");
    FILE* f = fopen((dir + "cases").c_str(), "r");
    if (!f) return 1;
    std::vector<uint8_t> out, flags;
    unsigned long long steps;
    unsigned ext, width, samples, batch;
    int tile_log, rc = 0;
    size_t off = 0;
    while (rc == 0 && fscanf(f, "%llu %u %u %u %u %d", &steps, &ext, &width, &samples, &batch, &tile_log) == 6) {
      if (width == 0 || width > M6S_MAX_WIDTH || batch == 0 || steps == 0 || steps > (1ull << 24)) {
        rc = 4;
        break;
      }
      const size_t wit_bytes = (size_t)batch * width * steps * 8, in_bytes = (size_t)batch * width * 8;
      if (in.size() < off + wit_bytes + in_bytes + 4 * width) {
        rc = 1;
        break;
      }
      std::vector<uint64_t> wit(wit_bytes / 8), inputs(in_bytes / 8);  // aligned copies of exactly the words the case may read
      memcpy(wit.data(), in.data() + off, wit_bytes);
      memcpy(inputs.data(), in.data() + off + wit_bytes, in_bytes);
      uint32_t counts[M6S_MAX_WIDTH];
      memcpy(counts, in.data() + off + wit_bytes + in_bytes, 4 * width);
      uint64_t total = 0;
      for (unsigned d = 0; d < width; ++d) total += counts[d];
      off += wit_bytes + in_bytes + 4 * width;
      if (total > M6S_MAX_TERMS || in.size() < off + total * 32 + total * width) {
        rc = 1;
        break;
      }
      const uint8_t* coefs = in.data() + off;
      const uint8_t* exps = coefs + total * 32;
      off += total * 32 + total * width;
      rc = prove(M, steps, ext, width, samples, batch, tile_log, wit.data(), inputs.data(), counts, coefs, exps, total, &out, &flags);
    }
    fclose(f);
    if (rc) return rc;
    spit(dir + "out", out.data(), out.size());
    spit(dir + "flags", flags.data(), flags.size());
    return 0;
  }
  return 1;
}
