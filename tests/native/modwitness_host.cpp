// The generic-modulus witness generator's decomposition (starks_amd/csrc/modwitness_items.cuh) run serially on the host: the term table
// as modwitness.hip stages it (Montgomery coefficients, the "coefficient is 1" flag derived from them), the plan, then per dispatch slice
// and step every lane of the group (mwi_lane), the exchange (mwi_gather) and the store in the chosen store form -- Montgomery rows and a
// closing pass (MWI_PASS), or a conversion on the store path (MWI_INLINE) -- with a dispatch resuming from the row the previous one
// stored.  tests/test_modwitness_host.py compares the witnesses with exact integers.
//   modwitness_host DIR width steps batch groups slices store
//   DIR: modulus (32 bytes wire) inputs (wire [batch][width]) coefs exps counts (raw files).  groups / slices: comma lists, 0 = the
//   library's default choice; store: 0 = pass, 1 = inline.  For every pair it prints "g s group slice cost" (what was asked, then the
//   plan) and writes DIR/witness.g.s (wire [batch][width][steps]).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "modwitness_items.cuh"

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
static std::vector<uint64_t> list_of(const char* s) {
  std::vector<uint64_t> v;
  for (const char* p = s; *p;) {
    char* end = nullptr;
    v.push_back(strtoull(p, &end, 10));
    if (end == p) break;
    p = *end == ',' ? end + 1 : end;
  }
  return v;
}

struct System {
  fpm_mod M;
  uint32_t T;
  WiRow rows[SHK_STARK_MAX_TERMS];
  fpm coefs[SHK_STARK_MAX_TERMS];
};

template <int W, int STORE>
static void trace(const System& S, const WiPlan& p, const uint8_t* in, uint64_t steps, uint32_t batch, uint8_t* out) {
  const fpm_mod& M = S.M;
  std::vector<fpm> wit((size_t)batch * W * steps);  // what d_witness holds
  for (uint32_t b = 0; b < batch; ++b) {
    fpm* col = wit.data() + (size_t)b * W * steps;
    fpm P[W];
    for (uint64_t k0 = 0, k1; k0 < steps; k0 = k1) {
      k1 = steps - k0 > p.slice ? k0 + p.slice : steps;
      uint64_t k = k0;
      if (k == 0) {
        for (int c = 0; c < W; ++c) {
          P[c] = fpm_to_mont(fpm_from_wire_bytes(in + 32ull * (b * W + c)), M);
          col[c * steps] = mwi_stored<STORE>(P[c], M);
        }
        k = 1;
      } else {  // a new dispatch: the state is the stored row
        for (int c = 0; c < W; ++c) P[c] = mwi_resumed<STORE>(col[c * steps + k - 1], M);
      }
      for (; k < k1; ++k) {
        fpm slots[WI_MAX_GROUP * W];
        for (uint32_t j = 0; j < p.group; ++j) {
          fpm Q[W];
          mwi_lane<W>(S.rows, S.coefs, p.t0[j], p.t1[j], P, Q, M);
          for (int c = 0; c < W; ++c) slots[j * W + c] = Q[c];
        }
        if (p.group == 1) {
          for (int c = 0; c < W; ++c) P[c] = slots[c];
        } else {
          mwi_gather<W>(slots, p, P, M);
        }
        for (int c = 0; c < W; ++c) col[c * steps + k] = mwi_stored<STORE>(P[c], M);
      }
    }
  }
  for (size_t i = 0; i < wit.size(); ++i) fpm_to_wire_bytes(STORE == MWI_PASS ? mwi_finish(wit[i], M) : wit[i], out + 32 * i);
}

template <int W>
static int run(const std::string& dir, uint64_t steps, uint32_t batch, const std::vector<uint64_t>& groups, const std::vector<uint64_t>& slices,
               int store) {
  const std::vector<uint8_t> md = slurp(dir + "/modulus"), in = slurp(dir + "/inputs"), cf = slurp(dir + "/coefs"), ex = slurp(dir + "/exps"),
                             cn = slurp(dir + "/counts");
  if (md.size() != 32 || cn.size() != 4 * W || in.size() != 32ull * batch * W) return 2;
  static System S;
  if (!fpm_mod_init(md.data(), &S.M)) return 2;
  uint32_t counts[W];
  memcpy(counts, cn.data(), sizeof counts);
  S.T = 0;
  for (int d = 0; d < W; ++d) S.T += counts[d];
  if (S.T == 0 || S.T > SHK_STARK_MAX_TERMS || cf.size() != 32ull * S.T || ex.size() != (size_t)W * S.T) return 2;
  for (uint32_t d = 0, t = 0; d < W; ++d)
    for (uint32_t i = 0; i < counts[d]; ++i, ++t) {
      S.coefs[t] = fpm_to_mont(fpm_from_wire_bytes(cf.data() + 32 * t), S.M);
      S.rows[t] = wi_pack_row(d, mwi_unit(S.coefs[t], S.M), ex.data() + (size_t)W * t, W);
    }
  std::vector<uint8_t> out(32ull * batch * W * steps);
  for (uint64_t g : groups)
    for (uint64_t sl : slices) {
      WiPlan p;
      mwi_plan(S.rows, S.T, W, (uint32_t)g, sl, &p);
      printf("%llu %llu %u %llu %u\n", (unsigned long long)g, (unsigned long long)sl, p.group, (unsigned long long)p.slice, p.cost);
      if (store) trace<W, MWI_INLINE>(S, p, in.data(), steps, batch, out.data());
      else trace<W, MWI_PASS>(S, p, in.data(), steps, batch, out.data());
      const std::string path = dir + "/witness." + std::to_string(g) + "." + std::to_string(sl);
      FILE* f = fopen(path.c_str(), "wb");
      if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 3;
      fclose(f);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: modwitness_host DIR width steps batch groups slices store\n");
    return 2;
  }
  const std::string dir = argv[1];
  const int width = atoi(argv[2]), store = atoi(argv[7]);
  const uint64_t steps = strtoull(argv[3], nullptr, 10);
  const uint32_t batch = (uint32_t)atoi(argv[4]);
  const std::vector<uint64_t> groups = list_of(argv[5]), slices = list_of(argv[6]);
  if (steps == 0 || batch == 0 || groups.empty() || slices.empty()) return 2;
  switch (width) {
    case 1: return run<1>(dir, steps, batch, groups, slices, store);
    case 2: return run<2>(dir, steps, batch, groups, slices, store);
    case 3: return run<3>(dir, steps, batch, groups, slices, store);
    case 4: return run<4>(dir, steps, batch, groups, slices, store);
    case 5: return run<5>(dir, steps, batch, groups, slices, store);
    case 6: return run<6>(dir, steps, batch, groups, slices, store);
    case 7: return run<7>(dir, steps, batch, groups, slices, store);
    case 8: return run<8>(dir, steps, batch, groups, slices, store);
    case 9: return run<9>(dir, steps, batch, groups, slices, store);
    default: return 2;
  }
}
