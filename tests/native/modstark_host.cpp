// Host driver of tests/test_modstark_host.py: the STARK prover over a run-time modulus walked on the host exactly as api_modstark.hip
// issues it -- the transforms through modntt_items.cuh, the items of modstark_items.cuh over the grids modstark.hip launches, the trees
// of plain values and the commit rounds through modfri_items.cuh, the upper tree levels with b2_hash_pair, the index sampler restated
// from utils.py:60-90 (the library's is the MiMC path's kernel).
//   prove <dir>   mod, cases (lines "steps ext width samples batch tile_log"), in (per case, in order: the witness [batch][width][steps]
//                 and the inputs [batch][width] in wire form, width counts as u32 little-endian, the terms' coefficients in wire form,
//                 their exponent rows) -> out (the flat proofs, concatenated), flags (one byte per proof: its constraint flag)
//                 exit 2: modulus rejected, 3: G2 of the wrong order, 4: shape rejected
//   inv <dir>     mod, values (wire form) -> out = their inverses modulo p (wire form, 0 for 0) through ms_batch_inv_item
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

// the nine widths of the trace-point and quotient items, every field product inlined into them, take minutes to compile under the
// sanitizers: the host walk leaves inlining to the compiler (fpm.cuh)
#define FPM_HD __host__ __device__ inline
#include "modstark_items.cuh"

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

// api_modntt.hip's mod_run on limbs: src [batch][n_in] -> dst [batch][n]; src may be dst when n_in == n
static void transform(const fpm_mod& M, const fpm& root_mont, int log_n, int tile_log, const fpm& scale, const fpm* src, uint64_t n_in,
                      fpm* dst, uint64_t batch) {
  const uint64_t n = 1ull << log_n;
  MnTw t;
  mn_tw_args(root_mont, log_n, M, &t);
  std::vector<fpm> tw(t.count ? t.count : 1);
  t.tw = tw.data();
  for (uint64_t e = 0; e < t.count; ++e) mn_tw_item(t, M, e);
  int radix[MN_MAX_PASSES];
  const int m = mn_plan(log_n, tile_log, radix);
  std::vector<fpm> work(batch * n), lds((size_t)1 << tile_log);
  for (int d = 0; d < m; ++d) {
    MnPass a = mn_pass(log_n, tile_log, radix, m, d, batch);
    a.tw = tw.data();
    a.src = d == 0 ? (const void*)src : (const void*)work.data();
    a.dst = d + 1 == m ? (void*)dst : (void*)work.data();
    if (d == 0) a.n_in = n_in;
    if (d + 1 == m) a.scale = scale;
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
// a launch of modstark.hip: grid_for_items(items) workgroups of MS_WG threads, the guard of the kernel
template <class F>
static void launch(uint64_t items, F&& body) {
  const uint64_t blocks = (items + MS_WG - 1) / MS_WG;
  for (uint64_t g = 0; g < blocks * MS_WG; ++g)
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
  if (!pow2(steps) || !pow2(ext) || steps < 2 || ext < 2 || width == 0 || samples == 0 || width > MS_MAX_WIDTH) return false;
  if (steps > (1ull << 24) || steps * ext >= (1ull << 24)) return false;
  if ((uint64_t)degree * (steps - 1) + 1 >= steps * ext) return false;
  return fri_shape_ok(steps * ext, steps * degree, ext, 40);
}

// api_modfri.hip's modfri_rounds with have_tree: the commit on vals_a / tree_a
static void fri_rounds(const fpm_mod& M, const fpm* tw, int log_n, std::vector<fpm>& vals_a, std::vector<uint32_t>& tree_a, uint64_t md,
                       uint32_t exclude, uint32_t samples, uint32_t batch, uint8_t* proof, uint64_t stride) {
  const uint64_t n = 1ull << log_n;
  std::vector<fpm> vals_b(batch * (n / 3 + 2));
  std::vector<uint32_t> tree_b(batch * 2 * (n / 3 + 2) * 8);
  std::vector<uint32_t> ys_buf(batch * ((samples > 40 ? samples : 40) + 40 * MF_MAX_ROUNDS) + 16);
  fpm* vals = vals_a.data();
  fpm* next = vals_b.data();
  uint32_t* tree = tree_a.data();
  uint32_t* tree2 = tree_b.data();
  MfFold fa;
  memset(&fa, 0, sizeof fa);
  fa.tw = tw;
  fa.log_n0 = (uint32_t)log_n;
  fa.inv_i = fpm_pow(mn_ld(tw + 1), 3 * (n / 4), M);  // tw[1] = the root (n >= 4)
  fa.batch = batch;
  MfGather ga;
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
    launch((nn >> 2) * batch, [&](uint64_t g) { mf_fold_item(fa, M, g); });
    MfTree tr2 = {next, tree2, nn / 4, batch, 0};
    leaves(tr2);
    upper_levels(tree2, nn / 4, batch);
    for (uint32_t b = 0; b < batch; ++b)
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
  launch(ga.work_total + ga.final_n * batch, [&](uint64_t g) { mf_gather_item(ga, g); });
}

template <int W>
static void quotients(const MsArgs& a, const fpm_mod& M) {
  launch(a.steps * a.batch, [&](uint64_t g) { ms_trace_item<W>(a, M, g); });
  launch(a.n * a.batch, [&](uint64_t g) { ms_quot_item<W>(a, M, g / a.n, g & (a.n - 1)); });
}

// api_modstark.hip's run_mod_stark
static int prove(const fpm_mod& M, uint64_t steps, uint32_t ext, uint32_t width, uint32_t samples, uint32_t batch, int tile_log,
                 const uint8_t* wit_wire, const uint8_t* in_wire, const uint32_t* counts, const uint8_t* coefs, const uint8_t* exps,
                 uint64_t total, std::vector<uint8_t>* out, std::vector<uint8_t>* flags) {
  if (total == 0 || total > MS_MAX_TERMS || batch == 0) return 4;
  const uint32_t degree = ms_terms_degree(exps, width, total);
  if (!shape_ok(steps, ext, width, degree, samples)) return 4;
  const uint64_t n = steps * ext, cols = (uint64_t)batch * width;
  int log_n = 0, log_s = 0;
  while ((1ull << log_n) < n) ++log_n;
  while ((1ull << log_s) < steps) ++log_s;
  const fpm g2 = ms_g2(M, log_n), pm2 = ms_pm2(M);
  if (!mn_check_root(fpm_from_mont(g2, M), n, M)) return 3;
  const fpm one = fpm_from_words(M.one), g1 = fpm_pow(g2, ext, M), g1_inv = fpm_pow(g1, steps - 1, M);
  const fpm x_last = fpm_pow(g2, (steps - 1) * ext, M);
  const fpm inv_last_m1 = fpm_pow_limbs(fpm_sub(x_last, one, M), pm2.v, M);
  const fpm cpow = fpm_pow(fpm_pow(g2, steps, M), n - 1, M);
  const fpm inv_steps = mn_inv_n(log_s, M);
  // the term image
  std::vector<fpm> cf(total), dcf(total * width + 1);
  std::vector<uint8_t> ex(total * width), dex(total * width * width + 1);
  std::vector<uint32_t> dbeg(width * width + 1);
  MsArgs a;
  memset(&a, 0, sizeof a);
  ms_terms_build(M, width, coefs, exps, counts, total, cf.data(), dcf.data(), ex.data(), dex.data(), dbeg.data(), a.term_begin);
  // the upload: wire form -> limbs, nothing reduced
  std::vector<fpm> wit(cols * steps), inputs(cols);
  for (uint64_t i = 0; i < cols * steps; ++i) wit[i] = fpm_from_wire_bytes(wit_wire + 32 * i);
  for (uint64_t i = 0; i < cols; ++i) inputs[i] = fpm_from_wire_bytes(in_wire + 32 * i);
  // the n-point table and the domain tables
  MnTw t;
  mn_tw_args(g2, log_n, M, &t);
  std::vector<fpm> tw(t.count);
  t.tw = tw.data();
  for (uint64_t e = 0; e < t.count; ++e) mn_tw_item(t, M, e);
  std::vector<fpm> den(2 * n), table(3 * n);
  MsTables mt;
  memset(&mt, 0, sizeof mt);
  mt.den = den.data();
  mt.table = table.data();
  mt.tw = tw.data();
  mt.n = n;
  mt.steps = steps;
  mt.ext = ext;
  mt.log_n = (uint32_t)log_n;
  mt.x_last = x_last;
  launch(n, [&](uint64_t i) { ms_den_item(mt, M, i); });
  MsInv inv;
  inv.in = den.data();
  inv.out = table.data();
  inv.count = 2 * n;
  inv.chunks = (inv.count + MS_INV_CHUNK - 1) / MS_INV_CHUNK;
  inv.pm2 = pm2;
  launch(inv.chunks, [&](uint64_t g) { ms_batch_inv_item(inv, M, g); });
  launch(n, [&](uint64_t i) { ms_tables_item(mt, M, i); });

  std::vector<fpm> P(cols * n), D(cols * n), B(cols * n), Q(cols * steps), iab(cols * 2), scal(cols * 3), l(batch * n);
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
  a.log_n = (uint32_t)log_n;
  a.tw = tw.data();
  a.inv_z2 = table.data();
  a.fz = table.data() + n;
  a.xpow = table.data() + 2 * n;
  a.x_last = x_last;
  a.g1 = g1;
  a.inv_last_m1 = inv_last_m1;
  a.inv_1_m_last = fpm_neg(inv_last_m1, M);
  a.inv_steps = inv_steps;
  a.bad = bad.data();
  a.term_coef = cf.data();
  a.term_exps = ex.data();
  a.dterm_coef = dcf.data();
  a.dterm_exps = dex.data();
  a.dterm_begin = dbeg.data();

  launch(cols, [&](uint64_t col) { ms_interp_item(a, M, col); });
  transform(M, g1_inv, log_s, tile_log, inv_steps, wit.data(), steps, Q.data(), cols);
  transform(M, g2, log_n, tile_log, fpm_from_u32(1u), Q.data(), steps, P.data(), cols);
  launch(cols * steps, [&](uint64_t g) { ms_qprep_item(Q.data(), Q.data(), steps, g, M); });
  transform(M, g1, log_s, tile_log, fpm_from_u32(1u), Q.data(), steps, Q.data(), cols);
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
  launch((n >> 2) * batch, [&](uint64_t g) { ms_leaf_row_item<false>(a, mtree.data(), g / (n >> 2), g & ((n >> 2) - 1)); });
  upper_levels(mtree.data(), n, batch);
  for (uint64_t blk = 0; blk < (batch + 63) / 64; ++blk)
    for (uint32_t tid = 0; tid < 64; ++tid)
      if (blk * 64 + tid < batch) ms_scalars_item(mtree.data(), 2 * n * 8, width, cpow, scal.data(), blk * 64 + tid, M);
  launch(n * batch, [&](uint64_t g) { ms_lincomb_item(a, scal.data(), l.data(), M, g / n, g & (n - 1)); });
  MfTree lt = {l.data(), ltree.data(), n, batch, 0};
  leaves(lt);
  upper_levels(ltree.data(), n, batch);
  for (uint32_t b = 0; b < batch; ++b) sample(ltree.data() + (uint64_t)b * 2 * n * 8 + 8, (uint32_t)n, samples, ext, ys.data() + (uint64_t)b * samples);
  const uint64_t header = 64 + (uint64_t)samples * 32 * (2 * (6 * width + (log_n - 1)) + (log_n + 1));
  const uint64_t stride = header + fri_len(n, steps * (uint64_t)degree, 40);
  std::vector<uint8_t> proof(stride * batch);
  MsGather ga;
  memset(&ga, 0, sizeof ga);
  ga.mnodes = mtree.data();
  ga.lnodes = ltree.data();
  ga.lvals = l.data();
  ga.ys = ys.data();
  ga.samples = samples;
  ga.lg = (uint32_t)log_n;
  ga.proof = proof.data();
  ga.stride = stride;
  launch(ms_gather_per_proof(width, samples, ga.lg) * batch, [&](uint64_t g) { ms_gather_item(a, ga, g); });
  fri_rounds(M, tw.data(), log_n, l, ltree, steps * (uint64_t)degree, ext, 40, batch, proof.data() + header, stride);
  out->insert(out->end(), proof.begin(), proof.end());
  for (uint32_t b = 0; b < batch; ++b) flags->push_back(bad[b] ? 1 : 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  const std::string mode = argv[1], dir = std::string(argv[2]) + "/";
  const std::vector<uint8_t> mod = slurp(dir + "mod");
  if (mod.size() != 32) return 1;
  fpm_mod M;
  if (!fpm_mod_init(mod.data(), &M)) return 2;
  std::vector<uint8_t> out, flags;
  if (mode == "inv") {
    const std::vector<uint8_t> vb = slurp(dir + "values");
    if (vb.size() % 32) return 1;
    const uint64_t count = vb.size() / 32;
    std::vector<fpm> in(count), res(count);
    for (uint64_t i = 0; i < count; ++i) in[i] = fpm_to_mont(fpm_from_wire_bytes(&vb[32 * i]), M);
    MsInv inv;
    inv.in = in.data();
    inv.out = res.data();
    inv.count = count;
    inv.chunks = (count + MS_INV_CHUNK - 1) / MS_INV_CHUNK;
    inv.pm2 = ms_pm2(M);
    launch(inv.chunks, [&](uint64_t g) { ms_batch_inv_item(inv, M, g); });
    out.resize(count * 32);
    for (uint64_t i = 0; i < count; ++i) fpm_to_wire_bytes(fpm_from_mont(res[i], M), &out[32 * i]);
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "prove") {
    const std::vector<uint8_t> in = slurp(dir + "in");
    FILE* f = fopen((dir + "cases").c_str(), "r");
    if (!f) return 1;
    unsigned long long steps;
    unsigned ext, width, samples, batch;
    int tile_log, rc = 0;
    size_t off = 0;
    while (rc == 0 && fscanf(f, "%llu %u %u %u %u %d", &steps, &ext, &width, &samples, &batch, &tile_log) == 6) {
      if (width == 0 || width > MS_MAX_WIDTH || batch == 0 || steps == 0 || steps > (1ull << 24)) {
        rc = 4;
        break;
      }
      const size_t wit_bytes = (size_t)batch * width * steps * 32, in_bytes = (size_t)batch * width * 32;
      if (in.size() < off + wit_bytes + in_bytes + 4 * width) {
        rc = 1;
        break;
      }
      const uint8_t* wit = in.data() + off;
      const uint8_t* inputs = wit + wit_bytes;
      uint32_t counts[MS_MAX_WIDTH];
      memcpy(counts, inputs + in_bytes, 4 * width);
      uint64_t total = 0;
      for (unsigned d = 0; d < width; ++d) total += counts[d];
      off += wit_bytes + in_bytes + 4 * width;
      if (total > MS_MAX_TERMS || in.size() < off + total * 32 + total * width) {
        rc = 1;
        break;
      }
      const uint8_t* coefs = in.data() + off;
      const uint8_t* exps = coefs + total * 32;
      off += total * 32 + total * width;
      rc = prove(M, steps, ext, width, samples, batch, tile_log, wit, inputs, counts, coefs, exps, total, &out, &flags);
    }
    fclose(f);
    if (rc) return rc;
    spit(dir + "out", out);
    spit(dir + "flags", flags);
    return 0;
  }
  return 1;
}
