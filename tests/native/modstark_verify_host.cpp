// The STARK verifiers over a run-time modulus on the host: shk::mod_stark_verify (starks_amd/csrc/modverify.hip, the code behind
// sh_mod_stark_verify, compiled into this program) beside the batch verifier's decomposition (starks_amd/csrc/modverify_items.cuh) run
// serially -- index sets, Merkle branches, FRI rows, spot checks, the final layer, then the OR per proof: the items modverify_dev.hip
// launches, in the same order, over the same plan.  tests/test_modstark_verify_host.py compares every line with the exact oracle.
//   modstark_verify_host DIR steps ext width samples batch
//       DIR: mod proofs inputs outputs coefs exps counts (raw files; a missing file is passed as a null pointer); inputs / outputs
//       [batch][width] wire form
// prints "plan <code> <reason>", then per proof "<host verifier's code> <item walk's code>": the walk's code is the plan's when the plan
// refuses the shape, SH_ERR_INVALID when the proofs' length is not the shape's or a buffer is missing (what sh_mod_stark_verify_batch
// answers), else 0 / -9.
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
// kernel code has no host form; the device's index sets are covered by tests/test_gpu_modstark_verify.py)
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

static bool walk(const MvPlan& p, const uint8_t* proof, const fpm* in, const fpm* out, const fpm* coef, const uint8_t* exps,
                 const uint32_t* tbegin) {
  const VbPlan& s = p.shape;
  const fpm_mod& M = p.M;
  std::vector<uint32_t> ys(s.ys_per_proof + 1);
  bool ok = true;
  // 1. index sets: the spot positions from l_root, then one set per round from its root2
  indices(proof + 32, (uint32_t)s.n, s.samples, s.exclude, ys.data());
  for (uint32_t r = 0; r < s.rounds; ++r) indices(proof + s.r[r].off, (uint32_t)(s.r[r].roudeg / 4), s.r[r].samples, s.exclude, ys.data() + s.r[r].set_off);
  // 2. branches: the two packed ones of each position against m_root, the l branch against l_root, then each round's five
  const uint64_t per = 2 * s.pb + s.lb;
  for (uint32_t i = 0; i < s.samples; ++i) {
    const uint8_t* b1 = proof + 64 + per * i;
    ok = vb_branch(b1, proof, ys[i], s.lg + 1, 96 * s.width) && ok;
    ok = vb_branch(b1 + s.pb, proof, ((uint64_t)ys[i] + s.ext) % s.n, s.lg + 1, 96 * s.width) && ok;
    ok = vb_branch(b1 + 2 * s.pb, proof + 32, ys[i], s.lg + 1, 32) && ok;
  }
  for (uint32_t r = 0; r < s.rounds; ++r) {
    const VbRound& rd = s.r[r];
    const uint32_t* set = ys.data() + rd.set_off;
    const uint64_t q = rd.roudeg / 4, rper = 32ull * (rd.l2 + 4ull * rd.l1);
    const uint8_t* mroot = proof + rd.root_off;  // never the caller's: a STARK proof carries l_root
    const fpm sx = mv_field_mont(mroot, M);
    for (uint32_t i = 0; i < rd.samples; ++i) {
      const uint8_t* sample = proof + rd.off + 32 + i * rper;
      ok = vb_branch(sample, proof + rd.off, set[i], rd.l2, 32) && ok;
      for (uint32_t j = 0; j < 4; ++j)
        ok = vb_branch(sample + 32ull * rd.l2 + 32ull * rd.l1 * j, mroot, (set[i] + j * q) % rd.roudeg, rd.l1, 32) && ok;
      // 3. the row
      ok = mv_fri_row(sample, rd.l1, rd.l2, p.w[r], p.inv_i[r], rd.roudeg, set[i], sx, M) && ok;
    }
  }
  // 4. spot checks
  for (uint32_t i = 0; i < s.samples; ++i) {
    const uint8_t* b1 = proof + 64 + per * i;
    ok = mv_spot(b1, b1 + s.pb, ys[i], p.sc, in, out, 1, coef, exps, s.width, tbegin, M) && ok;
  }
  // 5. the final layer: the tree against the last root (l_root without a round), then the degree bound
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
  ok = memcmp(&nodes[8], proof + (s.rounds ? s.r[s.rounds - 1].off : 32), 32) == 0 && ok;
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
  const uint64_t steps = strtoull(argv[2], nullptr, 10);
  const uint32_t ext = (uint32_t)strtoul(argv[3], nullptr, 10), width = (uint32_t)strtoul(argv[4], nullptr, 10);
  const uint32_t samples = (uint32_t)strtoul(argv[5], nullptr, 10), batch = (uint32_t)strtoul(argv[6], nullptr, 10);
  bool has_mod, has_proofs, has_in, has_out, has_coefs, has_exps, has_counts;
  const std::vector<uint8_t> mod = slurp(dir + "mod", &has_mod), proofs = slurp(dir + "proofs", &has_proofs);
  const std::vector<uint8_t> inputs = slurp(dir + "inputs", &has_in), outputs = slurp(dir + "outputs", &has_out);
  const std::vector<uint8_t> coefs = slurp(dir + "coefs", &has_coefs), exps = slurp(dir + "exps", &has_exps);
  const std::vector<uint8_t> cb = slurp(dir + "counts", &has_counts);
  std::vector<uint32_t> counts(cb.size() / 4);
  if (!counts.empty()) memcpy(counts.data(), cb.data(), counts.size() * 4);
  uint64_t total = 0;
  for (uint32_t c : counts) total += c;
  // (the width of a refused shape may be anything: the files only have to fit where the verifiers read them, which they do after
  // their own checks of width and of the term counts)
  if ((has_mod && mod.size() != 32) || batch == 0 || proofs.size() % batch || (width >= 1 && width <= 9 && has_counts && counts.size() != width) ||
      (has_in && inputs.size() != 32ull * batch * (width ? width : 1)) || (has_out && outputs.size() != 32ull * batch * (width ? width : 1)) ||
      (has_coefs && has_counts && total <= 256 && coefs.size() != 32 * total) ||
      (has_exps && has_counts && total <= 256 && width >= 1 && width <= 9 && exps.size() != total * width)) {
    fprintf(stderr, "malformed input files\n");
    return 2;
  }
  const uint64_t len = proofs.size() / batch;
  // a file that is there but empty is a valid pointer to nothing, not a null pointer
  static const uint32_t nothing[1] = {0};
  auto bytes_of = [&](const std::vector<uint8_t>& v, bool has) {
    return has ? (v.empty() ? reinterpret_cast<const uint8_t*>(nothing) : v.data()) : nullptr;
  };
  const uint8_t* modp = bytes_of(mod, has_mod);
  const uint8_t* expp = bytes_of(exps, has_exps);
  const uint8_t* coefp = bytes_of(coefs, has_coefs);
  const uint32_t* cntp = has_counts ? (counts.empty() ? nothing : counts.data()) : nullptr;
  MvPlan p;
  const char* why = "";
  const int rc = mv_plan_stark_proof(&p, modp, steps, ext, width, expp, cntp, samples, &why);
  printf("plan %d %s\n", rc, why);
  // the terms as the device holds them (ModTermLayout): Montgomery-form coefficients, exponent rows of `width` bytes
  std::vector<fpm> coef;
  uint32_t tbegin[10] = {0};
  if (rc == SH_OK && has_coefs) {
    for (uint64_t t = 0; t < total; ++t) coef.push_back(fpm_to_mont(fpm_from_wire_bytes(&coefs[32 * t]), p.M));
    for (uint32_t d = 0; d < width; ++d) tbegin[d + 1] = tbegin[d] + counts[d];
  }
  const size_t wbytes = 32ull * (width ? width : 1);
  for (uint32_t b = 0; b < batch; ++b) {
    // exact-size copies of each proof and of its inputs and outputs: AddressSanitizer sees any read past an end
    const std::vector<uint8_t> one(proofs.begin() + b * len, proofs.begin() + (b + 1) * len);
    std::vector<uint8_t> in1, out1;
    if (has_in) in1.assign(inputs.begin() + b * wbytes, inputs.begin() + (b + 1) * wbytes);
    if (has_out) out1.assign(outputs.begin() + b * wbytes, outputs.begin() + (b + 1) * wbytes);
    const int host = shk::mod_stark_verify(modp, has_proofs ? one.data() : nullptr, len, has_in ? in1.data() : nullptr,
                                           has_out ? out1.data() : nullptr, steps, ext, width, coefp, expp, cntp,
                                           samples);
    int items = rc;
    if (rc == SH_OK) {
      if (len != p.shape.plen || !has_proofs || !has_in || !has_out || !has_coefs) {
        items = SH_ERR_INVALID;
      } else {
        std::vector<fpm> in, out;  // plain limbs: a byte reversal of the wire form, nothing reduced
        for (uint32_t d = 0; d < width; ++d) {
          in.push_back(fpm_from_wire_bytes(&in1[32 * d]));
          out.push_back(fpm_from_wire_bytes(&out1[32 * d]));
        }
        items = walk(p, one.data(), in.data(), out.data(), coef.data(), exps.data(), tbegin) ? SH_OK : SH_ERR_REJECTED;
      }
    }
    printf("%d %d\n", host, items);
  }
  return 0;
}
