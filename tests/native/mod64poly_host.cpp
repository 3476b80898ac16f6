// The packed-word polynomial arithmetic and batch inversion (starks_amd/csrc/mod64poly_items.cuh with the drivers of poly_items.cuh --
// the code api_mod64poly.hip runs) on a host back end: a textbook radix-2 NTT over f64_* in place of the device plans, one loop per
// kernel launch over the same element steps, and the batch inversion's tiles walked serially with the tile shape as a parameter.
// tests/test_mod64poly_host.py compares the results with exact integers.
//   mod64poly_host mul DIR P ROOT ROOT_LOG        DIR/a, DIR/b        -> DIR/out        (n_a + n_b - 1 coefficients)
//   mod64poly_host divmod DIR P ROOT ROOT_LOG     DIR/a, DIR/b        -> DIR/q, DIR/r
//   mod64poly_host zpoly DIR P ROOT ROOT_LOG      DIR/xs              -> DIR/out        (n + 1 coefficients)
//   mod64poly_host lagrange DIR P ROOT ROOT_LOG   DIR/xs, DIR/ys      -> DIR/out        (n coefficients)
//   mod64poly_host inv DIR P L C                  DIR/in              -> DIR/out        (in place, like d_in == d_out)
//   mod64poly_host interp DIR P L C               DIR/xs, DIR/ys      -> DIR/out        ([rows][4] coefficients)
// P and ROOT are decimal; every file holds native 8-byte words.  The first four print "largest-transform-seen
// sh_mod_poly_max_transform's-value transforms", the last two "depth powers launches".  Exit codes: 2 usage or a bad file, 4 a refused
// modulus, 5 a refused root, 7 a transform above the root's order.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mod64poly_items.cuh"
#include "modpoly_items.cuh"  // mp_max_transform
#include "ntt64_items.cuh"    // n64_check_root, n64_inv_n, n64_pointwise_item

typedef std::vector<uint64_t> V;
static uint64_t g_transforms = 0, g_largest = 0;

static V load(const std::string& path) {
  V v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return v;
  uint64_t buf[1 << 13];
  size_t k;
  while ((k = fread(buf, 8, sizeof buf / 8, f)) > 0) v.insert(v.end(), buf, buf + k);  // as read: possibly >= p
  fclose(f);
  return v;
}
static void store(const std::string& path, const V& v, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) exit(3);
  if (n) fwrite(v.data(), 8, n, f);  // as stored: the steps store canonical words
  fclose(f);
}

// poly_items.cuh's Ops on the host over the modulus M: one loop per launch
struct HostOps {
  f64_mod M;
  uint64_t root_mont;
  int root_log;
  V bufs[PA_BUF_COUNT];

  // dst[b][0, n) = the size-n transform of src[b][0, n_in) (zero beyond) over root^(2^(root_log - lg n)); plain words in and out
  int ntt(const uint64_t* src, uint64_t* dst, uint64_t batch, uint64_t n, uint64_t n_in, bool inverse) {
    if (n_in == 0 || n_in > n) n_in = n;
    const int lg = (int)pa_log2(n);
    if (lg > root_log) return 7;
    if (n > g_largest) g_largest = n;
    uint64_t w = root_mont;
    for (int i = lg; i < root_log; ++i) w = f64_mul(w, w, M);
    if (inverse) w = f64_pow(w, n - 1, M);
    const uint64_t scale = inverse ? n64_inv_n(lg, M) : 1;
    V a(n);
    for (uint64_t b = 0; b < batch; ++b) {
      ++g_transforms;
      for (uint64_t i = 0; i < n; ++i) {
        uint64_t r = 0;
        for (int k = 0; k < lg; ++k) r |= ((i >> k) & 1) << (lg - 1 - k);
        a[r] = i < n_in ? f64_to_mont(src[b * n_in + i], M) : 0;
      }
      for (uint64_t len = 2; len <= n; len <<= 1) {
        const uint64_t wl = f64_pow(w, n / len, M);
        for (uint64_t s = 0; s < n; s += len) {
          uint64_t t = M.one;
          for (uint64_t k = 0; k < len / 2; ++k) {
            const uint64_t u = a[s + k], v = f64_mul(a[s + k + len / 2], t, M);
            a[s + k] = f64_add(u, v, M);
            a[s + k + len / 2] = f64_sub(u, v, M);
            t = f64_mul(t, wl, M);
          }
        }
      }
      for (uint64_t i = 0; i < n; ++i) dst[b * n + i] = f64_mul(a[i], scale, M);  // the plain scale leaves Montgomery form
    }
    return 0;
  }
  int copy(const PaCopy& c, const uint64_t* src, uint64_t* dst) {
    for (uint64_t r = 0; r < c.rows; ++r)
      for (uint64_t k = 0; k < c.len; ++k) dst[r * c.ds + k] = m6p_copy_item(c, src, r, k, M);
    return 0;
  }
  int pointwise(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = n64_pointwise_item(a[i], b[i], M);
    return 0;
  }
  // the pair loops of mod64poly.hip's m6p_tree_kernel and m6p_mid_kernel
  int tree(const uint64_t* hz, uint64_t* oz, const uint64_t* hn, uint64_t* on, uint32_t log2d, uint64_t nodes) {
    for (uint64_t g = 0; g < (nodes / 2) << log2d; ++g) {
      const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1), a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
      if (oz) oz[g] = m6p_tree_node(hz[a], hz[b], i, M);
      if (on) on[g] = m6p_num_node(hn[a], hn[b], hz[a], hz[b], i, M);
    }
    return 0;
  }
  int mid(const uint64_t* hd, uint64_t* hr, uint32_t log2d, uint64_t children) {
    for (uint64_t g = 0; g < (children / 2) << log2d; ++g) {
      const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1), a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
      uint64_t oa, ob;
      m6p_mid(hd[g], hr[a], hr[b], &oa, &ob, M);
      hr[a] = oa;
      hr[b] = ob;
    }
    return 0;
  }
  int newton(const uint64_t* F, uint64_t* G, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) G[i] = m6p_newton(F[i], G[i], M);
    return 0;
  }
  int inv1(const uint64_t* src, uint64_t* dst) {
    *dst = m6p_inv1(*src, M);
    return 0;
  }
  int deriv_rev(const uint64_t* top, uint64_t* out, uint64_t N, uint64_t n) {
    for (uint64_t k = 0; k < N; ++k) out[k] = m6p_deriv_rev(top, N, n, k, M);
    return 0;
  }
  int multi_inv(const uint64_t* in, uint64_t* out, uint64_t n);  // below: the tiled decomposition with the production tile
  int weights(const uint64_t* ys, const uint64_t* inv, uint64_t* out, uint64_t n, uint64_t N) {
    for (uint64_t i = 0; i < N; ++i) out[i] = i < n ? m6p_weight(ys[i], inv[i], M) : 0;
    return 0;
  }
  int sub(const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = m6p_sub(a[i], b[i], M);
    return 0;
  }
  int buf(int slot, uint64_t elems, uint64_t** out) {
    bufs[slot].assign(elems ? elems : 1, 0);
    *out = bufs[slot].data();
    return 0;
  }
};

// ---- the batch inversion, tile by tile (mod64poly.hip's kernels and run()) -------------------------------------------------------------
static uint32_t g_powers = 0, g_launches = 0;

template <uint32_t L, uint32_t C, class Src>
static void up(const Src& s, const f64_mod& M, uint64_t count, uint64_t* next) {
  ++g_launches;
  const uint64_t tiles = (count + L * C - 1) / (L * C);
  V t(2 * L);
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    M6pChunk<C> ch;
    for (uint32_t l = 0; l < L; ++l) t[L + l] = m6p_chunk_forward<L, C>(s, M, count, tile, l, ch);
    for (uint32_t h = L / 2; h >= 1; h /= 2)
      for (uint32_t l = 0; l < h; ++l) m6p_tree_up(t.data(), h + l, M);
    next[tile] = t[1];
  }
}
template <uint32_t L, uint32_t C, class Src>
static void down(const Src& s, const f64_mod& M, uint64_t count, const uint64_t* tile_inv) {
  ++g_launches;
  const uint64_t tiles = (count + L * C - 1) / (L * C);
  V t(2 * L);
  std::vector<M6pChunk<C>> ch(L);
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    for (uint32_t l = 0; l < L; ++l) t[L + l] = m6p_chunk_forward<L, C>(s, M, count, tile, l, ch[l]);
    for (uint32_t h = L / 2; h >= 1; h /= 2)
      for (uint32_t l = 0; l < h; ++l) m6p_tree_up(t.data(), h + l, M);
    if (tile_inv) {
      t[1] = tile_inv[tile];
    } else {
      t[1] = m6p_top_inv(t[1], M);
      ++g_powers;
    }
    for (uint32_t h = 1; h < L; h *= 2)
      for (uint32_t l = 0; l < h; ++l) m6p_tree_down(t.data(), h + l, M);
    for (uint32_t l = 0; l < L; ++l) m6p_chunk_backward<L, C>(s, M, count, tile, l, ch[l], t[L + l]);
  }
}
template <uint32_t L, uint32_t C, class Src>
static uint32_t run(const Src& items, const f64_mod& M, uint64_t n) {
  const IvLevels v = m6p_iv_levels<L, C>(n);
  V scratch(v.scratch + 1);
  uint64_t* sc = scratch.data();
  for (uint32_t j = 0; j + 1 < v.depth; ++j) {
    if (j == 0) up<L, C>(items, M, v.count[0], sc + v.off[1]);
    else up<L, C>(M6pMont{sc + v.off[j]}, M, v.count[j], sc + v.off[j + 1]);
  }
  for (int j = (int)v.depth - 1; j >= 0; --j) {
    const uint64_t* above = j + 1 < (int)v.depth ? sc + v.off[j + 1] : nullptr;
    if (j == 0) down<L, C>(items, M, v.count[0], above);
    else down<L, C>(M6pMont{sc + v.off[j]}, M, v.count[j], above);
  }
  return v.depth;
}
int HostOps::multi_inv(const uint64_t* in, uint64_t* out, uint64_t n) {
  run<M6P_IV_LANES, M6P_IV_CHUNK>(M6pElems{in, out}, M, n);
  return 0;
}

template <uint32_t L, uint32_t C>
static int go(const std::string& mode, const std::string& dir, const f64_mod& M) {
  uint32_t depth = 0;
  if (mode == "inv") {
    V x = load(dir + "in");
    if (x.empty()) return 2;
    depth = run<L, C>(M6pElems{x.data(), x.data()}, M, x.size());
    store(dir + "out", x, x.size());
  } else {
    V xs = load(dir + "xs"), ys = load(dir + "ys");
    if (xs.empty() || xs.size() % 4 || ys.size() != xs.size()) return 2;
    V out(xs.size());
    depth = run<L, C>(M6pRows{xs.data(), ys.data(), out.data()}, M, xs.size() / 4);
    store(dir + "out", out, out.size());
  }
  printf("%u %u %u\n", depth, g_powers, g_launches);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    fprintf(stderr, "usage: %s mul|divmod|zpoly|lagrange DIR P ROOT ROOT_LOG | inv|interp DIR P L C\n", argv[0]);
    return 2;
  }
  const std::string op = argv[1], dir = std::string(argv[2]) + "/";
  HostOps o;
  if (!f64_mod_init(strtoull(argv[3], nullptr, 10), &o.M)) return 4;
  if (op == "inv" || op == "interp") {
    const uint32_t L = atoi(argv[4]), C = atoi(argv[5]);
    // the production tiles and a few tiny ones (several levels at n ~ 10^3)
    if (L == M6P_IV_LANES && C == M6P_IV_CHUNK) return go<M6P_IV_LANES, M6P_IV_CHUNK>(op, dir, o.M);
    if (L == M6P_IV_LANES && C == M6P_IV_ROW_CHUNK) return go<M6P_IV_LANES, M6P_IV_ROW_CHUNK>(op, dir, o.M);
    if (L == 4 && C == 2) return go<4, 2>(op, dir, o.M);
    if (L == 2 && C == 2) return go<2, 2>(op, dir, o.M);
    if (L == 4 && C == 1) return go<4, 1>(op, dir, o.M);
    if (L == 8 && C == 3) return go<8, 3>(op, dir, o.M);
    return 2;
  }
  const uint64_t root = strtoull(argv[4], nullptr, 10);
  o.root_log = atoi(argv[5]);
  if (o.root_log < 0 || o.root_log > N64_MAX_LOG_N) return 4;
  if (!n64_check_root(root, 1ull << o.root_log, o.M)) return 5;
  o.root_mont = f64_to_mont(root, o.M);
  int rc = 2;
  uint64_t formula = 0;
  if (op == "mul") {
    const V a = load(dir + "a"), b = load(dir + "b");
    if (a.empty() || b.empty()) return 2;
    const uint64_t nc = a.size() + b.size() - 1;
    V out(nc), t1(pa_pow2_at_least(nc)), t2(t1.size());
    formula = mp_max_transform(MP_OP_MUL, a.size(), b.size());
    rc = pa_mul(o, a.data(), a.size(), b.data(), b.size(), out.data(), t1.data(), t2.data());
    store(dir + "out", out, nc);
  } else if (op == "divmod") {
    const V a = load(dir + "a"), b = load(dir + "b");
    if (a.empty() || b.empty()) return 2;
    const uint64_t nq = a.size() >= b.size() ? a.size() - b.size() + 1 : 0, nr = a.size() < b.size() - 1 ? a.size() : b.size() - 1;
    V q(nq + 1), r(nr + 1);
    formula = mp_max_transform(MP_OP_DIVMOD, a.size(), b.size());
    rc = pa_divmod(o, a.data(), a.size(), b.data(), b.size(), q.data(), r.data());
    store(dir + "q", q, nq);
    store(dir + "r", r, nr);
  } else if (op == "zpoly") {
    const V xs = load(dir + "xs");
    V out(xs.size() + 1);
    formula = mp_max_transform(MP_OP_ZPOLY, xs.size(), 0);
    rc = pa_zpoly(o, xs.data(), xs.size(), out.data());
    store(dir + "out", out, out.size());
  } else if (op == "lagrange") {
    const V xs = load(dir + "xs"), ys = load(dir + "ys");
    V out(xs.size());
    formula = mp_max_transform(MP_OP_LAGRANGE, xs.size(), 0);
    rc = xs.empty() ? 0 : pa_lagrange(o, xs.data(), ys.data(), xs.size(), out.data());
    store(dir + "out", out, out.size());
  }
  printf("%llu %llu %llu\n", (unsigned long long)g_largest, (unsigned long long)formula, (unsigned long long)g_transforms);
  return rc;
}
