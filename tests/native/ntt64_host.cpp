// Host driver of tests/test_ntt64_host.py: fp64m.cuh's arithmetic on files of native 64-bit words, the pass bodies of ntt64_items.cuh
// walked workgroup by workgroup, phase by phase, over the grid the library launches (api_ntt64.hip: m64_run), and the index maps of
// the same header enumerated lane by lane.  <p> and roots are decimal.
//   consts <dir> <p>                  -> out = p | n0inv | r2 | one; exit 2: modulus rejected
//   arith <dir> <p> <op>              a, b -> out; op = mul add sub to_mont from_mont canon
//   from_limbs <dir> <p>              a = 32-byte values (8 x u32 little-endian limbs) -> out = words
//   ntt <dir> <p>                     in, cases (lines "log_n n_in batch inverse tile_log offset root": the case reads batch n_in
//                                     words of `in` from word `offset` on) -> out (concatenated results); stdout: the passes of
//                                     each case.  exit 2: modulus rejected, 3: root rejected
//   mul <dir> <p> <log_n> <n_a> <n_b> <tile_log> <root>   a, b -> out = the cyclic product times n (fft.py:334-345)
//   check <dir> <p> <n> <root>        exit 0 accepted, 2 modulus rejected, 3 root rejected
//   runs <dir> <p> <log_n> <batch> <tile_log>    stdout, per pass: "pass load_run store_run" -- the shortest run of consecutive element
//                                     indices over the aligned groups of 16 lanes of every global load / store slot of the first
//                                     tile, the last tile and 64 tiles between
//   banks <dir> <p> <log_n> <batch> <tile_log>   stdout, per pass: "pass load_write group_read group_write store_read" -- the largest
//                                     conflict degree of any lane group of any LDS instruction of the same tiles (ds_read_b64: groups of
//                                     32 lanes over 64 banks; ds_write_b64: groups of 16 lanes over 32 banks)
// The LDS tile is a heap array of exactly the tile's elements, allocated per pass: an index outside the tile is caught by ASan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ntt64_items.cuh"

static std::vector<uint64_t> slurp(const std::string& path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (f) {
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
  }
  std::vector<uint64_t> w(v.size() / 8);
  if (!w.empty()) memcpy(w.data(), v.data(), w.size() * 8);
  return w;
}
static void spit(const std::string& path, const std::vector<uint64_t>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!v.empty()) fwrite(v.data(), 8, v.size(), f);
  fclose(f);
}

// one transform exactly as api_ntt64.hip's m64_run issues it
static int walk(const f64_mod& M, uint64_t root_mont, uint64_t scale, int log_n, int tile_log, const uint64_t* src, uint64_t n_in,
                uint64_t* dst, uint64_t batch) {
  const uint64_t n = 1ull << log_n;
  int radix[N64_MAX_PASSES];
  const int m = n64_plan(log_n, tile_log, radix);
  N64Tw t = {};
  std::vector<uint64_t> tab;
  if (log_n) {
    n64_tw_args(root_mont, log_n, radix[0], M, &t);
    tab.resize(n64_table_entries(t));
    t.tab = tab.data();
    for (uint64_t i = 0; i < tab.size(); ++i) n64_tw_item(t, M, i);
    if (n64_table_bytes(t) > n64_table_bound(log_n, tile_log)) return -1;
  }
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
  return m;
}

// the tiles the `runs` and `banks` modes look at
static std::vector<uint64_t> sample_tiles(uint64_t tiles) {
  std::vector<uint64_t> v;
  for (uint64_t i = 0; i < 66; ++i) v.push_back(tiles <= 66 ? i % tiles : (tiles - 1) * i / 65);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}
// the shortest maximal run of consecutive values in idx[0 .. cnt)
static uint32_t shortest_run(const uint64_t* idx, uint32_t cnt) {
  uint32_t best = ~0u, run = 1;
  for (uint32_t i = 1; i <= cnt; ++i) {
    if (i < cnt && idx[i] == idx[i - 1] + 1) {
      ++run;
    } else {
      best = std::min(best, run);
      run = 1;
    }
  }
  return best;
}
// the largest number of distinct word addresses of one lane group that share a bank: 8-byte accesses, `slots` = banks / 2
static uint32_t degree(const uint32_t* at, const bool* on, uint32_t lanes, uint32_t slots) {
  uint32_t worst = 0;
  for (uint32_t s = 0; s < slots; ++s) {
    std::vector<uint32_t> seen;
    for (uint32_t l = 0; l < lanes; ++l)
      if (on[l] && at[l] % slots == s && std::find(seen.begin(), seen.end(), at[l]) == seen.end()) seen.push_back(at[l]);
    worst = std::max(worst, (uint32_t)seen.size());
  }
  return worst;
}
static uint32_t worst_degree(const uint32_t at[N64_WG], const bool on[N64_WG], uint32_t lanes, uint32_t slots) {
  uint32_t worst = 0;
  for (uint32_t l = 0; l < N64_WG; l += lanes) worst = std::max(worst, degree(at + l, on + l, lanes, slots));
  return worst;
}

static int maps(bool banks, int log_n, uint64_t batch, int tile_log) {
  int radix[N64_MAX_PASSES];
  const int m = n64_plan(log_n, tile_log, radix);
  for (int d = 0; d < m; ++d) {
    const N64Pass a = n64_pass(log_n, tile_log, radix, m, d, batch);
    const uint32_t elems = n64_tile_elems(a);
    uint32_t load_run = ~0u, store_run = ~0u, load_w = 0, group_r = 0, group_w = 0, store_r = 0;
    for (uint64_t wg : sample_tiles(n64_tiles(a))) {
      uint64_t idx[N64_WG], e;
      uint32_t at[N64_WG];
      bool on[N64_WG], zero;
      for (uint32_t x0 = 0; x0 < elems; x0 += N64_WG) {  // one load / store instruction slot of the 256 threads
        for (uint32_t tid = 0; tid < N64_WG; ++tid)
          on[tid] = x0 + tid < elems && n64_load_map(a, wg, x0 + tid, &idx[tid], &zero, &at[tid]) && !zero;
        for (uint32_t l = 0; l < N64_WG; l += 16)
          if (std::all_of(on + l, on + l + 16, [](bool b) { return b; })) load_run = std::min(load_run, shortest_run(idx + l, 16));
        load_w = std::max(load_w, worst_degree(at, on, 16, 16));
        for (uint32_t tid = 0; tid < N64_WG; ++tid) on[tid] = x0 + tid < elems && n64_store_map(a, wg, x0 + tid, &idx[tid], &at[tid], &e);
        for (uint32_t l = 0; l < N64_WG; l += 16)
          if (std::all_of(on + l, on + l + 16, [](bool b) { return b; })) store_run = std::min(store_run, shortest_run(idx + l, 16));
        store_r = std::max(store_r, worst_degree(at, on, 32, 32));
      }
      for (uint32_t g = 0; g < n64_groups(a.log_R); ++g) {
        uint32_t q, b, low, el[N64_WG][8];
        n64_group_shape(a.log_R, g, &q, &b);
        for (uint32_t x0 = 0; x0 < (elems >> q); x0 += N64_WG) {
          for (uint32_t tid = 0; tid < N64_WG; ++tid) on[tid] = x0 + tid < (elems >> q) && n64_group_map(a, b, q, wg, x0 + tid, el[tid], &low);
          for (uint32_t j = 0; j < (1u << q); ++j) {  // element j: one ds_read_b64 and one ds_write_b64 of every wave
            for (uint32_t tid = 0; tid < N64_WG; ++tid) at[tid] = on[tid] ? el[tid][j] : 0;
            group_r = std::max(group_r, worst_degree(at, on, 32, 32));
            group_w = std::max(group_w, worst_degree(at, on, 16, 16));
          }
        }
      }
    }
    if (banks) printf("%d %u %u %u %u\n", d, load_w, group_r, group_w, store_r);
    else printf("%d %u %u\n", d, load_run, store_run);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) return 1;
  const std::string mode = argv[1], dir = std::string(argv[2]) + "/";
  f64_mod M;
  if (!f64_mod_init(strtoull(argv[3], nullptr, 10), &M)) return 2;
  std::vector<uint64_t> out;
  if (mode == "consts") {
    out = {M.p, M.n0inv, M.r2, M.one};
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "arith" && argc == 5) {
    const std::string op = argv[4];
    const std::vector<uint64_t> a = slurp(dir + "a"), b = slurp(dir + "b");
    for (size_t i = 0; i < a.size(); ++i) {
      const uint64_t x = a[i], y = i < b.size() ? b[i] : 0;
      out.push_back(op == "mul" ? f64_mul(x, y, M) : op == "add" ? f64_add(x, y, M) : op == "sub" ? f64_sub(x, y, M)
                    : op == "to_mont" ? f64_to_mont(x, M) : op == "from_mont" ? f64_from_mont(x, M) : f64_canon(x, M));
    }
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "from_limbs") {
    const std::vector<uint64_t> a = slurp(dir + "a");
    for (size_t i = 0; i + 4 <= a.size(); i += 4) {
      uint32_t w[8];
      memcpy(w, &a[i], 32);
      out.push_back(f64_from_limbs(w, M));
    }
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "ntt") {
    const std::vector<uint64_t> in = slurp(dir + "in");
    FILE* f = fopen((dir + "cases").c_str(), "r");
    if (!f) return 1;
    int log_n, inverse, tile_log;
    unsigned long long n_in, batch, offset, root;
    while (fscanf(f, "%d %llu %llu %d %d %llu %llu", &log_n, &n_in, &batch, &inverse, &tile_log, &offset, &root) == 7) {
      const uint64_t n = 1ull << log_n;
      if (in.size() < offset + batch * n_in || n_in > n) return 1;
      if (!n64_check_root(root, n, M)) return 3;
      uint64_t r = f64_to_mont(root, M);
      if (inverse) r = f64_pow(r, n - 1, M);
      const uint64_t scale = inverse ? n64_inv_n(log_n, M) : 1;
      // the source is a heap copy of exactly the words the case may read
      const std::vector<uint64_t> src(in.begin() + offset, in.begin() + offset + batch * n_in);
      std::vector<uint64_t> res(batch * n);
      const int m = walk(M, r, scale, log_n, tile_log, src.data(), n_in, res.data(), batch);
      if (m < 0) return 4;
      printf("%d\n", m);
      out.insert(out.end(), res.begin(), res.end());
    }
    fclose(f);
    spit(dir + "out", out);
    return 0;
  }
  if (mode == "check" && argc == 6) return n64_check_root(strtoull(argv[5], nullptr, 10), strtoull(argv[4], nullptr, 10), M) ? 0 : 3;
  if (mode == "mul" && argc == 9) {
    const int log_n = atoi(argv[4]), tile_log = atoi(argv[7]);
    const uint64_t n = 1ull << log_n, n_a = strtoull(argv[5], nullptr, 10), n_b = strtoull(argv[6], nullptr, 10);
    const uint64_t root = strtoull(argv[8], nullptr, 10);
    std::vector<uint64_t> a = slurp(dir + "a"), b = slurp(dir + "b");
    if (a.size() < n_a || b.size() < n_b || n_a > n || n_b > n) return 1;
    a.resize(n_a);
    b.resize(n_b);
    if (!n64_check_root(root, n, M)) return 3;
    const uint64_t r = f64_to_mont(root, M);
    std::vector<uint64_t> fa(n), fb(n);
    out.resize(n);
    walk(M, r, 1, log_n, tile_log, a.data(), n_a, fa.data(), 1);
    walk(M, r, 1, log_n, tile_log, b.data(), n_b, fb.data(), 1);
    for (uint64_t i = 0; i < n; ++i) fa[i] = n64_pointwise_item(fa[i], fb[i], M);
    walk(M, f64_pow(r, n - 1, M), 1, log_n, tile_log, fa.data(), n, out.data(), 1);
    spit(dir + "out", out);
    return 0;
  }
  if ((mode == "runs" || mode == "banks") && argc == 7)
    return maps(mode == "banks", atoi(argv[4]), strtoull(argv[5], nullptr, 10), atoi(argv[6]));
  return 1;
}
