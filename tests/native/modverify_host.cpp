// The FRI verifiers over any odd modulus on the host: shk::mod_fri_verify (starks_amd/csrc/modverify.hip, the code behind
// sh_mod_fri_verify, compiled into this program) beside the batch verifier's decomposition (starks_amd/csrc/modverify_items.cuh) run
// serially -- index sets, Merkle branches, FRI rows, the final layer, then the OR per proof: the items modverify_dev.hip launches, in
// the same order, over the same plan.  tests/test_modverify_host.py compares every line with the exact oracle.
//   modverify_host DIR n md exclude samples batch     DIR: mod root proofs roots (raw files; a missing file is passed as a null pointer)
// prints "plan <code>", then per proof "<host verifier's code> <item walk's code>": the walk's code is the plan's when the plan refuses
// the shape, SH_ERR_INVALID when the proofs' length is not the shape's (what sh_mod_fri_verify_batch answers), else 0 / -9.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "modverify.hip"
#include "modverify_items.cuh"

static std::vector<uint8_t> slurp(const std::string& path, bool* there) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  *there = f != nullptr;
  if (!f) return v;
  uint8_t buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

// get_pseudorandom_indices (utils.py:60-90) as sample_indices_quad chains it, one hash per 8 indices: a serial host rewrite (the quad-lane
// kernel code has no host form; the device's index sets are covered by tests/test_gpu_modverify.py)
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

static bool walk(const MvPlan& p, const uint8_t* proof, const uint8_t* ext_root) {
  const VbPlan& s = p.shape;
  const fpm_mod& M = p.M;
  std::vector<uint32_t> ys(s.ys_per_proof + 1);
  bool ok = true;
  for (uint32_t r = 0; r < s.rounds; ++r) {
    const VbRound& rd = s.r[r];
    uint32_t* set = ys.data() + rd.set_off;
    const uint64_t q = rd.roudeg / 4, per = 32ull * (rd.l2 + 4ull * rd.l1);
    const uint8_t* mroot = rd.root_off < 0 ? ext_root : proof + rd.root_off;
    // 1. the index set, 2. the column branch and the four row branches of every sample, 3. the rows
    indices(proof + rd.off, (uint32_t)q, rd.samples, s.exclude, set);
    const fpm sx = mv_field_mont(mroot, M);
    for (uint32_t i = 0; i < rd.samples; ++i) {
      const uint8_t* sample = proof + rd.off + 32 + i * per;
      ok = vb_branch(sample, proof + rd.off, set[i], rd.l2, 32) && ok;
      for (uint32_t j = 0; j < 4; ++j)
        ok = vb_branch(sample + 32ull * rd.l2 + 32ull * rd.l1 * j, mroot, (set[i] + j * q) % rd.roudeg, rd.l1, 32) && ok;
      ok = mv_fri_row(sample, rd.l1, rd.l2, p.w[r], p.inv_i[r], rd.roudeg, set[i], sx, M) && ok;
    }
  }
  // 4. the final layer: the tree, then the degree bound
  const uint8_t* data = proof + s.final_off;
  const uint64_t len = s.final_len;
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
  ok = memcmp(&nodes[8], s.rounds ? proof + s.r[s.rounds - 1].off : ext_root, 32) == 0 && ok;
  fpm wgt[VB_MAX_K];
  for (uint64_t a = 0; a < s.k; ++a) wgt[a] = mv_final_weight(a, s.exclude, data, p.cof, M);
  for (uint64_t t = s.k; t < vb_npts(len, s.exclude); ++t) ok = mv_final_point(t, s.k, p.w_final, s.exclude, data, p.xk, wgt, p.D, M) && ok;
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: see the header of this file\n");
    return 2;
  }
  const std::string dir = std::string(argv[1]) + "/";
  const uint64_t n = strtoull(argv[2], nullptr, 10), md = strtoull(argv[3], nullptr, 10);
  const uint32_t exclude = (uint32_t)strtoul(argv[4], nullptr, 10), samples = (uint32_t)strtoul(argv[5], nullptr, 10);
  const uint32_t batch = (uint32_t)strtoul(argv[6], nullptr, 10);
  bool has_mod, has_root, has_proofs, has_roots;
  const std::vector<uint8_t> mod = slurp(dir + "mod", &has_mod), root = slurp(dir + "root", &has_root);
  const std::vector<uint8_t> proofs = slurp(dir + "proofs", &has_proofs), roots = slurp(dir + "roots", &has_roots);
  if ((has_mod && mod.size() != 32) || (has_root && root.size() != 32) || batch == 0 || proofs.size() % batch ||
      (has_roots && roots.size() != 32ull * batch)) {
    fprintf(stderr, "malformed input files\n");
    return 2;
  }
  const uint64_t len = proofs.size() / batch;
  MvPlan p;
  const char* why = "";
  const int rc = mv_plan_fri_proof(&p, has_mod ? mod.data() : nullptr, n, has_root ? root.data() : nullptr, md, exclude, samples, &why);
  printf("plan %d\n", rc);
  for (uint32_t b = 0; b < batch; ++b) {
    // an exact-size copy of each proof: AddressSanitizer sees any read past its end
    const std::vector<uint8_t> one(proofs.begin() + b * len, proofs.begin() + (b + 1) * len);
    const uint8_t* mroot = has_roots ? roots.data() + 32ull * b : nullptr;
    const int host = shk::mod_fri_verify(has_mod ? mod.data() : nullptr, has_proofs ? one.data() : nullptr, len, mroot, n,
                                         has_root ? root.data() : nullptr, md, exclude, samples);
    int items = rc;
    if (rc == SH_OK) items = len != p.shape.plen || !has_proofs || !mroot ? SH_ERR_INVALID : (walk(p, one.data(), mroot) ? SH_OK : SH_ERR_REJECTED);
    printf("%d %d\n", host, items);
  }
  return 0;
}
