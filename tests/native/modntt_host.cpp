// Host driver of tests/test_modntt_host.py: fpm.cuh's arithmetic on files of wire-form operands, and the pass bodies of
// modntt_items.cuh walked workgroup by workgroup, phase by phase, over the grid the library launches (api_modntt.hip: mod_run).
//   consts <dir>                      mod -> out = p | r2 | one | n0inv (32 bytes each); exit 2: modulus rejected
//   arith <dir> <op>                  mod, a, b -> out; op = mul add sub to_mont from_mont canon
//   ntt <dir>                         mod, in, cases (lines "log_n n_in batch inverse tile_log offset root": the case reads batch n_in
//                                     values of `in` from value `offset` on, root = 64 hex digits) -> out (concatenated wire results)
//                                     stdout: the passes of each case.  exit 2: modulus rejected, 3: root rejected
//   mul <dir> <log_n> <n_a> <n_b> <tile_log>   mod, root, a, b -> out = the cyclic product times n (fft.py:334-345)
//   check <dir> <n>                   mod, root -> exit 0 accepted, 2 modulus rejected, 3 root rejected
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "modntt_items.cuh"

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
static void put(std::vector<uint8_t>* o, const fpm& a) {
  uint8_t w[32];
  fpm_to_wire_bytes(a, w);
  o->insert(o->end(), w, w + 32);
}

// one transform exactly as api_modntt.hip's mod_run issues it; src / dst are wire form
static int walk(const fpm_mod& M, const fpm& root_mont, const fpm& scale, int log_n, int tile_log, const uint8_t* src, uint64_t n_in,
                uint8_t* dst, uint64_t batch) {
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
    if (d == 0) {
      a.n_in = n_in;
      a.wire_in = 1;
    }
    if (d + 1 == m) {
      a.scale = scale;
      a.wire_out = 1;
    }
    const uint64_t tiles = mn_tiles(a);
    for (uint64_t wg = 0; wg < tiles; ++wg) {
      for (uint32_t tid = 0; tid < MN_WG; ++tid) mn_load_item(a, M, wg, tid, lds.data());
      for (uint32_t s = 1; s <= a.log_R; ++s)
        for (uint32_t tid = 0; tid < MN_WG; ++tid) mn_stage_item(a, M, s, wg, tid, lds.data());
      for (uint32_t tid = 0; tid < MN_WG; ++tid) mn_store_item(a, M, wg, tid, lds.data());
    }
  }
  return m;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  const std::string mode = argv[1], dir = std::string(argv[2]) + "/";
  const std::vector<uint8_t> mod = slurp(dir + "mod");
  if (mod.size() != 32) return 1;
  fpm_mod M;
  if (!fpm_mod_init(mod.data(), &M)) return 2;
  std::vector<uint8_t> out;
  if (mode == "consts") {
    put(&out, fpm_from_words(M.p));
    put(&out, fpm_from_words(M.r2));
    put(&out, fpm_from_words(M.one));
    put(&out, fpm_from_u32(M.n0inv));
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "arith") {
    const std::string op = argv[3];
    const std::vector<uint8_t> a = slurp(dir + "a"), b = slurp(dir + "b");
    for (size_t i = 0; i + 32 <= a.size(); i += 32) {
      const fpm x = fpm_from_wire_bytes(&a[i]), y = i + 32 <= b.size() ? fpm_from_wire_bytes(&b[i]) : fpm_zero();
      put(&out, op == "mul" ? fpm_mul(x, y, M) : op == "add" ? fpm_add(x, y, M) : op == "sub" ? fpm_sub(x, y, M)
                : op == "to_mont" ? fpm_to_mont(x, M) : op == "from_mont" ? fpm_from_mont(x, M) : fpm_canon(x, M));
    }
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "ntt") {
    const std::vector<uint8_t> in = slurp(dir + "in");
    FILE* f = fopen((dir + "cases").c_str(), "r");
    if (!f) return 1;
    int log_n, inverse, tile_log;
    unsigned long long n_in, batch, offset;
    char hex[65];
    while (fscanf(f, "%d %llu %llu %d %d %llu %64s", &log_n, &n_in, &batch, &inverse, &tile_log, &offset, hex) == 7) {
      const uint64_t n = 1ull << log_n;
      if (in.size() < (offset + batch * n_in) * 32 || n_in > n || strlen(hex) != 64) return 1;
      uint8_t rb[32];
      for (int i = 0; i < 32; ++i) {
        unsigned v;
        sscanf(hex + 2 * i, "%2x", &v);
        rb[i] = (uint8_t)v;
      }
      const fpm root = fpm_from_wire_bytes(rb);
      if (!mn_check_root(root, n, M)) return 3;
      fpm r = fpm_to_mont(root, M);
      if (inverse) r = fpm_pow(r, n - 1, M);
      const fpm scale = inverse ? mn_inv_n(log_n, M) : fpm_from_u32(1u);
      std::vector<uint8_t> res(batch * n * 32);
      printf("%d\n", walk(M, r, scale, log_n, tile_log, in.data() + offset * 32, n_in, res.data(), batch));
      out.insert(out.end(), res.begin(), res.end());
    }
    fclose(f);
    spit(dir + "out", out);
    return 0;
  }
  const std::vector<uint8_t> rootb = slurp(dir + "root");
  if (rootb.size() != 32) return 1;
  const fpm root = fpm_from_wire_bytes(rootb.data());
  if (mode == "check") return mn_check_root(root, strtoull(argv[3], nullptr, 10), M) ? 0 : 3;
  if (mode == "mul" && argc == 7) {
    const int log_n = atoi(argv[3]), tile_log = atoi(argv[6]);
    const uint64_t n = 1ull << log_n, n_a = strtoull(argv[4], nullptr, 10), n_b = strtoull(argv[5], nullptr, 10);
    const std::vector<uint8_t> a = slurp(dir + "a"), b = slurp(dir + "b");
    if (a.size() < n_a * 32 || b.size() < n_b * 32 || n_a > n || n_b > n) return 1;
    if (!mn_check_root(root, n, M)) return 3;
    const fpm r = fpm_to_mont(root, M), one = fpm_from_u32(1u);
    std::vector<uint8_t> fa(n * 32), fb(n * 32), prod(n * 32);
    out.resize(n * 32);
    walk(M, r, one, log_n, tile_log, a.data(), n_a, fa.data(), 1);
    walk(M, r, one, log_n, tile_log, b.data(), n_b, fb.data(), 1);
    for (uint64_t i = 0; i < n; ++i) {
      uint8_t w[32];
      fpm_to_wire_bytes(mn_pointwise_item(fpm_from_wire_bytes(&fa[32 * i]), fpm_from_wire_bytes(&fb[32 * i]), M), w);
      memcpy(&prod[32 * i], w, 32);
    }
    walk(M, fpm_pow(r, n - 1, M), one, log_n, tile_log, prod.data(), n, out.data(), 1);
    spit(dir + "out", out);
    return 0;
  }
  return 1;
}
