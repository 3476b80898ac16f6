// The packed-word witness generator's decomposition (starks_amd/csrc/mod64witness_items.cuh) run serially on the host: the packed
// prover's term image (m6s_terms_build: Montgomery coefficient words, exponent rows) staged as mod64witness.hip stages it (the dimension
// from the begin offsets, the "coefficient is 1" flag derived from the word), the plan, then per dispatch slice and step every lane of
// the group (m6w_lane), the exchange (m6w_gather) and the store in the chosen store form -- Montgomery rows and a closing pass (M6W_PASS),
// or a conversion on the store path (M6W_INLINE) -- with a dispatch resuming from the row the previous one stored.
// tests/test_mod64witness_host.py compares the witnesses with exact integers.
//   mod64witness_host DIR width steps batch groups slices store
//   DIR: modulus (one native word) inputs (native words [batch][width]) coefs (32-byte wire values) exps counts (raw files).  groups /
//   slices: comma lists, 0 = the library's default choice; store: 0 = pass, 1 = inline.  For every pair it prints "g s group slice cost"
//   (what was asked, then the plan) and writes DIR/witness.g.s (native words [batch][width][steps]).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mod64stark_items.cuh"
#include "mod64witness_items.cuh"

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
  f64_mod M;
  uint32_t T;
  WiRow rows[SHK_STARK_MAX_TERMS];
  uint64_t coefs[SHK_STARK_MAX_TERMS];
};

template <int W, int STORE>
static void trace(const System& S, const WiPlan& p, const uint64_t* in, uint64_t steps, uint32_t batch, uint64_t* out) {
  const f64_mod& M = S.M;
  std::vector<uint64_t> wit((size_t)batch * W * steps);  // what d_witness holds
  for (uint32_t b = 0; b < batch; ++b) {
    uint64_t* col = wit.data() + (size_t)b * W * steps;
    uint64_t P[W];
    for (uint64_t k0 = 0, k1; k0 < steps; k0 = k1) {
      k1 = steps - k0 > p.slice ? k0 + p.slice : steps;
      uint64_t k = k0;
      if (k == 0) {
        for (int c = 0; c < W; ++c) {
          P[c] = f64_to_mont(in[(size_t)b * W + c], M);
          col[c * steps] = m6w_stored<STORE>(P[c], M);
        }
        k = 1;
      } else {  // a new dispatch: the state is the stored row
        for (int c = 0; c < W; ++c) P[c] = m6w_resumed<STORE>(col[c * steps + k - 1], M);
      }
      for (; k < k1; ++k) {
        uint64_t slots[WI_MAX_GROUP * W];
        for (uint32_t j = 0; j < p.group; ++j) {
          uint64_t Q[W];
          m6w_lane<W>(S.rows, S.coefs, p.t0[j], p.t1[j], P, Q, M);
          for (int c = 0; c < W; ++c) slots[j * W + c] = Q[c];
        }
        if (p.group == 1) {
          for (int c = 0; c < W; ++c) P[c] = slots[c];
        } else {
          m6w_gather<W>(slots, p, P, M);
        }
        for (int c = 0; c < W; ++c) col[c * steps + k] = m6w_stored<STORE>(P[c], M);
      }
    }
  }
  for (size_t i = 0; i < wit.size(); ++i) out[i] = STORE == M6W_PASS ? m6w_finish(wit[i], M) : wit[i];
}

template <int W>
static int run(const std::string& dir, uint64_t steps, uint32_t batch, const std::vector<uint64_t>& groups, const std::vector<uint64_t>& slices,
               int store) {
  const std::vector<uint8_t> md = slurp(dir + "/modulus"), inb = slurp(dir + "/inputs"), cf = slurp(dir + "/coefs"), ex = slurp(dir + "/exps"),
                             cn = slurp(dir + "/counts");
  if (md.size() != 8 || cn.size() != 4 * W || inb.size() != 8ull * batch * W) return 2;
  static System S;
  uint64_t modulus;
  memcpy(&modulus, md.data(), 8);
  if (!f64_mod_init(modulus, &S.M)) return 2;
  uint32_t counts[W];
  memcpy(counts, cn.data(), sizeof counts);
  S.T = 0;
  for (int d = 0; d < W; ++d) S.T += counts[d];
  if (S.T == 0 || S.T > SHK_STARK_MAX_TERMS || cf.size() != 32ull * S.T || ex.size() != (size_t)W * S.T) return 2;
  {  // the packed prover's term image, then the kernel's staging of it
    std::vector<uint64_t> icf(S.T), dcf((size_t)S.T * W);
    std::vector<uint8_t> iex((size_t)S.T * W), dex((size_t)S.T * W * W);
    uint32_t dbeg[W * W + 1], begin[SHK_STARK_MAX_WIDTH + 1] = {0};
    m6s_terms_build(S.M, W, cf.data(), ex.data(), counts, S.T, icf.data(), dcf.data(), iex.data(), dex.data(), dbeg, begin);
    for (int c = W + 1; c <= (int)SHK_STARK_MAX_WIDTH; ++c) begin[c] = begin[W];
    for (uint32_t t = 0; t < S.T; ++t) {
      uint32_t dim = 0;
      for (int c = 0; c < W; ++c) dim += begin[c + 1] <= t ? 1u : 0u;
      S.coefs[t] = icf[t];
      S.rows[t] = wi_pack_row(dim, m6w_unit(icf[t], S.M), iex.data() + (size_t)t * W, W);
    }
  }
  std::vector<uint64_t> in((size_t)batch * W), out((size_t)batch * W * steps);
  memcpy(in.data(), inb.data(), inb.size());
  for (uint64_t g : groups)
    for (uint64_t sl : slices) {
      WiPlan p;
      m6w_plan(S.rows, S.T, W, (uint32_t)g, sl, &p);
      printf("%llu %llu %u %llu %u\n", (unsigned long long)g, (unsigned long long)sl, p.group, (unsigned long long)p.slice, p.cost);
      if (store) trace<W, M6W_INLINE>(S, p, in.data(), steps, batch, out.data());
      else trace<W, M6W_PASS>(S, p, in.data(), steps, batch, out.data());
      const std::string path = dir + "/witness." + std::to_string(g) + "." + std::to_string(sl);
      FILE* f = fopen(path.c_str(), "wb");
      if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) return 3;
      fclose(f);
    }
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: mod64witness_host DIR width steps batch groups slices store\n");
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
