// The device batch inversion's decomposition (starks_amd/csrc/inv_items.cuh) run serially on the host: the levels of iv_levels, per
// level and tile every lane's chunk (iv_chunk_forward), the tile's product tree (iv_tree_up), the single top inversion, the tree walked
// down (iv_tree_down) and every lane's chunk backwards (iv_chunk_backward) -- what multi_inv.hip launches, tile by tile, with the tile
// shape as a parameter.  tests/test_poly_utils_host.py compares the outputs with exact integers.
//   multi_inv_host inv    L C DIR     DIR/in: n wire-form values -> DIR/out: n wire-form inverses (0 for 0), in place like d_in == d_out
//   multi_inv_host interp L C DIR     DIR/xs, DIR/ys: [rows][4] wire form -> DIR/out: [rows][4] coefficients
// Prints "depth inversions launches" of the call.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "inv_items.cuh"

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
static std::vector<fp> from_wire(const std::vector<uint8_t>& b) {
  std::vector<fp> v(b.size() / 32);
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t w[8];
    memcpy(w, b.data() + 32 * i, 32);
    v[i] = fp_from_wire_words(w);  // as read: possibly >= p
  }
  return v;
}
static void write_wire(const std::string& path, const std::vector<fp>& v) {
  std::vector<uint8_t> b(32 * v.size());
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t w[8];
    fp_to_wire_words(v[i], w);  // as stored: the items' finish stores canonical values
    memcpy(b.data() + 32 * i, w, 32);
  }
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) exit(3);
  fwrite(b.data(), 1, b.size(), f);
  fclose(f);
}

static uint32_t inversions = 0, launches = 0;

template <uint32_t L, uint32_t C, class Src>
static void up(const Src& s, uint64_t count, fp* next) {
  ++launches;
  const uint64_t tiles = (count + L * C - 1) / (L * C);
  std::vector<fp> t(2 * L);
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    IvChunk<C> ch;
    for (uint32_t l = 0; l < L; ++l) t[L + l] = iv_chunk_forward<L, C>(s, count, tile, l, ch);
    for (uint32_t h = L / 2; h >= 1; h /= 2)
      for (uint32_t l = 0; l < h; ++l) iv_tree_up(t.data(), h + l);
    next[tile] = fp_canon(t[1]);
  }
}

template <uint32_t L, uint32_t C, class Src>
static void down(const Src& s, uint64_t count, const fp* tile_inv) {
  ++launches;
  const uint64_t tiles = (count + L * C - 1) / (L * C);
  std::vector<fp> t(2 * L);
  std::vector<IvChunk<C>> ch(L);
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    for (uint32_t l = 0; l < L; ++l) t[L + l] = iv_chunk_forward<L, C>(s, count, tile, l, ch[l]);
    for (uint32_t h = L / 2; h >= 1; h /= 2)
      for (uint32_t l = 0; l < h; ++l) iv_tree_up(t.data(), h + l);
    if (tile_inv) {
      t[1] = tile_inv[tile];
    } else {
      t[1] = fp_inv(t[1]);
      ++inversions;
    }
    for (uint32_t h = 1; h < L; h *= 2)
      for (uint32_t l = 0; l < h; ++l) iv_tree_down(t.data(), h + l);
    for (uint32_t l = 0; l < L; ++l) iv_chunk_backward<L, C>(s, count, tile, l, ch[l], t[L + l]);
  }
}

// multi_inv.hip's run(): the same order of passes
template <uint32_t L, uint32_t C, class Src>
static void run(const Src& items, uint64_t n) {
  const IvLevels v = iv_levels(n, (uint64_t)L * C);
  std::vector<fp> scratch(v.scratch + 1);
  fp* sc = scratch.data();
  for (uint32_t j = 0; j + 1 < v.depth; ++j) {
    if (j == 0) up<L, C>(items, v.count[0], sc + v.off[1]);
    else up<L, C>(IvElems{sc + v.off[j], sc + v.off[j]}, v.count[j], sc + v.off[j + 1]);
  }
  for (int j = (int)v.depth - 1; j >= 0; --j) {
    const fp* above = j + 1 < (int)v.depth ? sc + v.off[j + 1] : nullptr;
    if (j == 0) down<L, C>(items, v.count[0], above);
    else down<L, C>(IvElems{sc + v.off[j], sc + v.off[j]}, v.count[j], above);
  }
  printf("%u %u %u\n", v.depth, inversions, launches);
}

template <uint32_t L, uint32_t C>
static int go(const std::string& mode, const std::string& dir) {
  if (mode == "inv") {
    std::vector<fp> x = from_wire(slurp(dir + "/in"));
    if (x.empty()) return 2;
    run<L, C>(IvElems{x.data(), x.data()}, x.size());
    write_wire(dir + "/out", x);
    return 0;
  }
  if (mode == "interp") {
    std::vector<fp> xs = from_wire(slurp(dir + "/xs")), ys = from_wire(slurp(dir + "/ys"));
    if (xs.empty() || xs.size() % 4 || ys.size() != xs.size()) return 2;
    std::vector<fp> out(xs.size());
    run<L, C>(IvRows{xs.data(), ys.data(), out.data()}, xs.size() / 4);
    write_wire(dir + "/out", out);
    return 0;
  }
  return 2;
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const std::string mode = argv[1], dir = argv[4];
  const uint32_t L = atoi(argv[2]), C = atoi(argv[3]);
  // the production tiles and a few tiny ones (several levels at n ~ 10^3)
  if (L == IV_LANES && C == IV_CHUNK) return go<IV_LANES, IV_CHUNK>(mode, dir);
  if (L == IV_LANES && C == IV_ROW_CHUNK) return go<IV_LANES, IV_ROW_CHUNK>(mode, dir);
  if (L == 4 && C == 2) return go<4, 2>(mode, dir);
  if (L == 2 && C == 2) return go<2, 2>(mode, dir);
  if (L == 4 && C == 1) return go<4, 1>(mode, dir);
  if (L == 8 && C == 3) return go<8, 3>(mode, dir);
  return 2;
}
