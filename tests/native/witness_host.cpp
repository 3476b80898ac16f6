// The device witness generator's decomposition (starks_amd/csrc/witness_items.cuh) run serially on the host: the plan for the system,
// then per dispatch slice and step every lane of the group (wi_lane), the exchange (wi_gather) and the canonical store -- what witness.hip
// launches, with a dispatch resuming from the row the previous one stored.  tests/test_witness_host.py compares the witness with the
// reference's traces.
//   witness_host DIR width steps batch group slice     DIR: inputs (wire [batch][width]) coefs exps counts (raw files); writes DIR/witness
//   (wire [batch][width][steps]) and prints "group slice cost" of the plan.  group / slice 0 = the library's default choice.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "witness_items.cuh"

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
static fp from_wire(const uint8_t* b) {
  uint32_t w[8];
  memcpy(w, b, 32);
  return fp_from_wire_words(w);  // as read: possibly >= p
}
static void to_wire(const fp& a, uint8_t* b) {
  uint32_t w[8];
  fp_to_wire_words(fp_canon(a), w);
  memcpy(b, w, 32);
}

template <int W>
static int run(const std::string& dir, uint64_t steps, uint32_t batch, uint32_t group, uint64_t slice) {
  const std::vector<uint8_t> in = slurp(dir + "/inputs"), cf = slurp(dir + "/coefs"), ex = slurp(dir + "/exps"), cn = slurp(dir + "/counts");
  if (cn.size() != 4 * W || in.size() != 32ull * batch * W) return 2;
  uint32_t counts[W], T = 0;
  memcpy(counts, cn.data(), sizeof counts);
  for (int d = 0; d < W; ++d) T += counts[d];
  if (T == 0 || T > SHK_STARK_MAX_TERMS || cf.size() != 32ull * T || ex.size() != (size_t)W * T) return 2;
  WiRow rows[SHK_STARK_MAX_TERMS];
  fp coefs[SHK_STARK_MAX_TERMS];
  for (uint32_t d = 0, t = 0; d < W; ++d)
    for (uint32_t i = 0; i < counts[d]; ++i, ++t) {
      coefs[t] = fp_canon(from_wire(cf.data() + 32 * t));
      rows[t] = wi_pack_row(d, fp_eq_canon(coefs[t], fp_one()), ex.data() + (size_t)W * t, W);
    }
  WiPlan p;
  wi_plan(rows, T, W, group, slice, &p);
  printf("%u %llu %u\n", p.group, (unsigned long long)p.slice, p.cost);
  std::vector<uint8_t> out(32ull * batch * W * steps);
  for (uint32_t b = 0; b < batch; ++b) {
    uint8_t* col = out.data() + 32ull * b * W * steps;
    fp P[W];
    for (uint64_t k0 = 0, k1; k0 < steps; k0 = k1) {
      k1 = steps - k0 > p.slice ? k0 + p.slice : steps;
      uint64_t k = k0;
      if (k == 0) {
        for (int c = 0; c < W; ++c) {
          P[c] = from_wire(in.data() + 32ull * (b * W + c));
          to_wire(P[c], col + 32 * (c * steps));
        }
        k = 1;
      } else {  // a new dispatch: the state is the stored row
        for (int c = 0; c < W; ++c) P[c] = from_wire(col + 32 * (c * steps + k - 1));
      }
      for (; k < k1; ++k) {
        fp slots[WI_MAX_GROUP * W];
        for (uint32_t j = 0; j < p.group; ++j) {
          fp Q[W];
          wi_lane<W>(rows, coefs, p.t0[j], p.t1[j], P, Q);
          for (int c = 0; c < W; ++c) slots[j * W + c] = Q[c];
        }
        if (p.group == 1) {
          for (int c = 0; c < W; ++c) P[c] = slots[c];
        } else {
          wi_gather<W>(slots, p, P);
        }
        for (int c = 0; c < W; ++c) to_wire(P[c], col + 32 * (c * steps + k));
      }
    }
  }
  FILE* f = fopen((dir + "/witness").c_str(), "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 3;
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 7) {
    fprintf(stderr, "usage: witness_host DIR width steps batch group slice\n");
    return 2;
  }
  const std::string dir = argv[1];
  const int width = atoi(argv[2]);
  const uint64_t steps = strtoull(argv[3], nullptr, 10), slice = strtoull(argv[6], nullptr, 10);
  const uint32_t batch = (uint32_t)atoi(argv[4]), group = (uint32_t)atoi(argv[5]);
  if (steps == 0 || batch == 0) return 2;
  switch (width) {
    case 1: return run<1>(dir, steps, batch, group, slice);
    case 2: return run<2>(dir, steps, batch, group, slice);
    case 3: return run<3>(dir, steps, batch, group, slice);
    case 4: return run<4>(dir, steps, batch, group, slice);
    case 5: return run<5>(dir, steps, batch, group, slice);
    case 6: return run<6>(dir, steps, batch, group, slice);
    case 7: return run<7>(dir, steps, batch, group, slice);
    case 8: return run<8>(dir, steps, batch, group, slice);
    case 9: return run<9>(dir, steps, batch, group, slice);
    default: return 2;
  }
}
