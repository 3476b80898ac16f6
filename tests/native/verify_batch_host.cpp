// The batch verifiers' decomposition (starks_amd/csrc/verify_items.cuh) run serially on the host: index sets, Merkle branches, FRI
// rows, spot checks, the final layer, then the OR per proof -- the items verify_dev.hip launches, in the same order, with the same plan.
// Prints one status per proof (0 = accepted, -9 = rejected), or the plan's code for the shape.  tests/test_verify_batch_host.py
// compares every line with sh_stark_verify / sh_fri_verify.
//   verify_batch_host stark DIR steps ext width samples batch   DIR: proofs inputs outputs coefs exps counts (raw files)
//   verify_batch_host fri   DIR n md exclude samples batch      DIR: proofs roots root
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "verify_items.cuh"

static std::vector<uint8_t> slurp(const std::string& path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return v;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

// get_pseudorandom_indices (utils.py:60-90): the chain sample_indices_quad computes with four lanes, one hash per 8 indices.  This is a
// serial host rewrite: the quad-lane kernel code (DPP, LDS) has no host form, so the index sets of the device path are covered only by
// tests/test_gpu_verify_batch.py, where every device status is compared with the host verifier's.
static void indices(const uint8_t* entropy, uint32_t modulus, uint32_t count, uint32_t exclude, uint32_t* ys) {
  uint32_t w[16] = {0};
  memcpy(w, entropy, 32);
  const uint32_t real = exclude ? (uint32_t)(((uint64_t)modulus * (exclude - 1)) / exclude) : modulus;
  for (uint32_t j = 0; j < count; ++j) {
    if (j && j % 8 == 0) {
      const b2digest d = b2_hash_short(w, 32);
      memcpy(w, d.h, 32);
    }
    const uint32_t x = __builtin_bswap32(w[j % 8]) % real;
    ys[j] = exclude ? x + 1 + x / (exclude - 1) : x;
  }
}

static bool check_branches(const uint8_t* proof, const uint8_t* ext_root, uint64_t off, uint64_t stride, uint64_t rep_stride, int64_t root_off,
                           uint32_t count, uint32_t reps, const uint32_t* set, uint32_t rep_add, uint64_t mod, uint32_t entries,
                           uint32_t leaf_bytes) {
  bool ok = true;
  const uint8_t* root = root_off < 0 ? ext_root : proof + root_off;
  for (uint32_t j = 0; j < reps; ++j)
    for (uint32_t i = 0; i < count; ++i)
      ok = vb_branch(proof + off + i * stride + j * rep_stride, root, ((uint64_t)set[i] + (uint64_t)j * rep_add) % mod, entries, leaf_bytes) && ok;
  return ok;
}

static bool verify_one(const VbPlan& p, const uint8_t* proof, const uint8_t* ext_root, const fp* in, const fp* out, const fp* coef,
                       const uint8_t* exps, uint32_t row, const uint32_t* tbegin) {
  std::vector<uint32_t> ys(p.ys_per_proof + 1);
  // 1. index sets
  if (p.stark) indices(proof + 32, (uint32_t)p.n, p.samples, p.exclude, ys.data());
  for (uint32_t r = 0; r < p.rounds; ++r)
    indices(proof + p.r[r].off, (uint32_t)(p.r[r].roudeg / 4), p.r[r].samples, p.exclude, ys.data() + p.r[r].set_off);
  bool ok = true;
  // 2. branches
  if (p.stark) {
    const uint64_t per = 2 * p.pb + p.lb;
    ok = check_branches(proof, ext_root, 64, per, p.pb, 0, p.samples, 2, ys.data(), p.ext, p.n, p.lg + 1, 96 * p.width) && ok;
    ok = check_branches(proof, ext_root, 64 + 2 * p.pb, per, 0, 32, p.samples, 1, ys.data(), 0, p.n, p.lg + 1, 32) && ok;
  }
  for (uint32_t r = 0; r < p.rounds; ++r) {
    const VbRound& rd = p.r[r];
    const uint64_t per = 32ull * (rd.l2 + 4ull * rd.l1);
    const uint32_t* set = ys.data() + rd.set_off;
    ok = check_branches(proof, ext_root, rd.off + 32, per, 0, (int64_t)rd.off, rd.samples, 1, set, 0, rd.roudeg / 4, rd.l2, 32) && ok;
    ok = check_branches(proof, ext_root, rd.off + 32 + 32ull * rd.l2, per, 32ull * rd.l1, rd.root_off, rd.samples, 4, set,
                        (uint32_t)(rd.roudeg / 4), rd.roudeg, rd.l1, 32) && ok;
  }
  // 3. FRI rows
  for (uint32_t r = 0; r < p.rounds; ++r) {
    const VbRound& rd = p.r[r];
    const fp special_x = vb_field(rd.root_off < 0 ? ext_root : proof + rd.root_off);
    for (uint32_t i = 0; i < rd.samples; ++i)
      ok = vb_fri_row(proof + rd.off + 32 + (uint64_t)i * 32 * (rd.l2 + 4ull * rd.l1), rd.l1, rd.l2, rd.w, rd.inv_i, rd.roudeg,
                      ys[rd.set_off + i], special_x) && ok;
  }
  // 4. spot checks
  if (p.stark)
    for (uint32_t i = 0; i < p.samples; ++i) {
      const uint8_t* b1 = proof + 64 + (2 * p.pb + p.lb) * i;
      ok = vb_spot(b1, b1 + p.pb, ys[i], p.sc, in, out, 1, coef, exps, row, tbegin) && ok;
    }
  // 5. final layer: the tree, then the degree bound
  const uint8_t* data = proof + p.final_off;
  const uint64_t len = p.final_len;
  std::vector<uint32_t> nodes(8 * len);
  for (uint64_t m = len / 2; m < len; ++m) {
    uint32_t l[8], r[8];
    vb_load8(data + 32 * vb_final_leaf(2 * m - len, len), l);
    vb_load8(data + 32 * vb_final_leaf(2 * m + 1 - len, len), r);
    const b2digest d = b2_hash_pair(l, r);
    memcpy(&nodes[8 * m], d.h, 32);
  }
  for (uint64_t m = len / 2 - 1; m >= 1; --m) {
    const b2digest d = b2_hash_pair(&nodes[16 * m], &nodes[16 * m + 8]);
    memcpy(&nodes[8 * m], d.h, 32);
  }
  const int64_t last_root = p.rounds ? (int64_t)p.r[p.rounds - 1].off : (p.stark ? 32 : -1);
  ok = memcmp(&nodes[8], last_root < 0 ? ext_root : proof + last_root, 32) == 0 && ok;
  fp wgt[VB_MAX_K];
  for (uint64_t a = 0; a < p.k; ++a) wgt[a] = vb_final_weight(a, p.exclude, data, p.inv_den);
  for (uint64_t t = p.k; t < vb_npts(len, p.exclude); ++t) ok = vb_final_point(t, p.k, p.w_final, p.exclude, data, p.xk, wgt) && ok;
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: see the header of this file\n");
    return 2;
  }
  const std::string kind = argv[1], dir = std::string(argv[2]) + "/";
  const std::vector<uint8_t> proofs = slurp(dir + "proofs");
  const uint32_t batch = (uint32_t)strtoul(argv[7], nullptr, 10);
  VbPlan p;
  int rc;
  std::vector<uint8_t> roots, coefs, exps, inputs, outputs;
  std::vector<uint32_t> counts;
  std::vector<fp> coef, in, out;
  std::vector<uint8_t> rows;
  uint32_t tbegin[SHK_STARK_MAX_WIDTH + 1] = {0};
  if (kind == "stark") {
    const uint64_t steps = strtoull(argv[3], nullptr, 10);
    const uint32_t ext = (uint32_t)strtoul(argv[4], nullptr, 10), width = (uint32_t)strtoul(argv[5], nullptr, 10);
    const uint32_t samples = (uint32_t)strtoul(argv[6], nullptr, 10);
    coefs = slurp(dir + "coefs");
    exps = slurp(dir + "exps");
    inputs = slurp(dir + "inputs");
    outputs = slurp(dir + "outputs");
    const std::vector<uint8_t> cb = slurp(dir + "counts");
    counts.resize(cb.size() / 4);
    memcpy(counts.data(), cb.data(), cb.size());
    rc = vb_plan_stark_proof(&p, steps, ext, width, exps.data(), counts.data(), samples);
    if (rc == SH_OK) {
      // the device layout of the terms (api_stark.hip:stark_terms): limb-form coefficients, exponent rows of width + 1 bytes
      const uint32_t total = (uint32_t)(coefs.size() / 32);
      for (uint32_t t = 0; t < total; ++t) coef.push_back(vb_wire(&coefs[32 * t]));
      rows.assign((size_t)total * (width + 1), 0);
      for (uint32_t t = 0; t < total; ++t) memcpy(&rows[t * (width + 1)], &exps[t * width], width);
      for (uint32_t d = 0; d < width; ++d) tbegin[d + 1] = tbegin[d] + counts[d];
      for (size_t i = 0; i < inputs.size() / 32; ++i) in.push_back(vb_wire(&inputs[32 * i]));
      for (size_t i = 0; i < outputs.size() / 32; ++i) out.push_back(vb_wire(&outputs[32 * i]));
    }
  } else {
    const uint64_t n = strtoull(argv[3], nullptr, 10), md = strtoull(argv[4], nullptr, 10);
    const uint32_t exclude = (uint32_t)strtoul(argv[5], nullptr, 10), samples = (uint32_t)strtoul(argv[6], nullptr, 10);
    roots = slurp(dir + "roots");
    const std::vector<uint8_t> root = slurp(dir + "root");
    rc = vb_plan_fri_proof(&p, n, root.data(), md, exclude, samples);
  }
  if (rc != SH_OK) {
    printf("shape %d\n", rc);
    return 0;
  }
  if (proofs.size() != (size_t)p.plen * batch) {
    printf("length %zu != %llu x %u\n", proofs.size(), (unsigned long long)p.plen, batch);
    return 1;
  }
  for (uint32_t b = 0; b < batch; ++b) {
    const uint8_t* proof = proofs.data() + (size_t)b * p.plen;
    const bool ok = p.stark ? verify_one(p, proof, nullptr, in.data() + (size_t)b * p.width, out.data() + (size_t)b * p.width, coef.data(),
                                         rows.data(), p.width + 1, tbegin)
                            : verify_one(p, proof, roots.data() + 32ull * b, nullptr, nullptr, nullptr, nullptr, 0, nullptr);
    printf("%d\n", ok ? SH_OK : SH_ERR_REJECTED);
  }
  return 0;
}
