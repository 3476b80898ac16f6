// The generic-modulus polynomial arithmetic and batch inversion (starks_amd/csrc/modpoly_items.cuh with the drivers of poly_items.cuh --
// the code api_modpoly.hip runs) on a host back end: a textbook radix-2 NTT over fpm in place of the device plans, one loop per kernel
// launch over the same element steps, and the batch inversion's tiles walked serially with the tile shape as a parameter.
// tests/test_modpoly_host.py compares the results with exact integers.
//   modpoly_host mul DIR ROOT_LOG        DIR/a, DIR/b        -> DIR/out        (n_a + n_b - 1 coefficients)
//   modpoly_host divmod DIR ROOT_LOG     DIR/a, DIR/b        -> DIR/q, DIR/r
//   modpoly_host zpoly DIR ROOT_LOG      DIR/xs              -> DIR/out        (n + 1 coefficients)
//   modpoly_host lagrange DIR ROOT_LOG   DIR/xs, DIR/ys      -> DIR/out        (n coefficients)
//   modpoly_host inv DIR L C             DIR/in              -> DIR/out        (in place, like d_in == d_out)
//   modpoly_host interp DIR L C          DIR/xs, DIR/ys      -> DIR/out        ([rows][4] coefficients)
// DIR/mod holds the modulus and DIR/root the root of order 2^ROOT_LOG; all files are 32-byte big-endian wire form.  The first four print
// "largest-transform-seen sh_mod_poly_max_transform's-value transforms", the last two "depth powers launches".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

// many instantiations of the tile walk: without forced inlining the host compile takes seconds, not minutes (fpm.cuh)
#define FPM_HD __host__ __device__ inline
#include "modpoly_items.cuh"

typedef std::vector<fpm> V;
static uint64_t g_transforms = 0, g_largest = 0;

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
static V load(const std::string& path) {
  const std::vector<uint8_t> b = slurp(path);
  V v(b.size() / 32);
  for (size_t i = 0; i < v.size(); ++i) v[i] = fpm_from_wire_bytes(&b[32 * i]);  // as read: possibly >= p
  return v;
}
static void store(const std::string& path, const V& v, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) exit(3);
  for (size_t i = 0; i < n; ++i) {
    uint8_t w[32];
    fpm_to_wire_bytes(v[i], w);  // as stored: the steps store canonical values
    fwrite(w, 1, 32, f);
  }
  fclose(f);
}

// poly_items.cuh's Ops on the host over the modulus M: one loop per launch
struct HostOps {
  fpm_mod M;
  fpm root_mont;
  int root_log;
  V bufs[PA_BUF_COUNT];

  // dst[b][0, n) = the size-n transform of src[b][0, n_in) (zero beyond) over root^(2^(root_log - lg n)); plain values in and out
  int ntt(const fpm* src, fpm* dst, uint64_t batch, uint64_t n, uint64_t n_in, bool inverse) {
    if (n_in == 0 || n_in > n) n_in = n;
    const int lg = (int)pa_log2(n);
    if (lg > root_log) return 7;
    if (n > g_largest) g_largest = n;
    fpm w = root_mont;
    for (int i = lg; i < root_log; ++i) w = fpm_mul(w, w, M);
    if (inverse) w = fpm_pow(w, n - 1, M);
    const fpm scale = inverse ? mn_inv_n(lg, M) : fpm_from_u32(1u);
    V a(n);
    for (uint64_t b = 0; b < batch; ++b) {
      ++g_transforms;
      for (uint64_t i = 0; i < n; ++i) {
        uint64_t r = 0;
        for (int k = 0; k < lg; ++k) r |= ((i >> k) & 1) << (lg - 1 - k);
        a[r] = i < n_in ? fpm_to_mont(src[b * n_in + i], M) : fpm_zero();
      }
      for (uint64_t len = 2; len <= n; len <<= 1) {
        const fpm wl = fpm_pow(w, n / len, M);
        for (uint64_t s = 0; s < n; s += len) {
          fpm t = fpm_from_words(M.one);
          for (uint64_t k = 0; k < len / 2; ++k) {
            const fpm u = a[s + k], v = fpm_mul(a[s + k + len / 2], t, M);
            a[s + k] = fpm_add(u, v, M);
            a[s + k + len / 2] = fpm_sub(u, v, M);
            t = fpm_mul(t, wl, M);
          }
        }
      }
      for (uint64_t i = 0; i < n; ++i) dst[b * n + i] = fpm_mul(a[i], scale, M);  // the plain scale leaves Montgomery form
    }
    return 0;
  }
  int copy(const PaCopy& c, const fpm* src, fpm* dst) {
    for (uint64_t r = 0; r < c.rows; ++r)
      for (uint64_t k = 0; k < c.len; ++k) dst[r * c.ds + k] = mp_copy_item(c, src, r, k, M);
    return 0;
  }
  int pointwise(const fpm* a, const fpm* b, fpm* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = mn_pointwise_item(a[i], b[i], M);
    return 0;
  }
  // the pair loops of modpoly.hip's mp_tree_kernel and mp_mid_kernel
  int tree(const fpm* hz, fpm* oz, const fpm* hn, fpm* on, uint32_t log2d, uint64_t nodes) {
    for (uint64_t g = 0; g < (nodes / 2) << log2d; ++g) {
      const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1), a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
      if (oz) oz[g] = mp_tree_node(hz[a], hz[b], i, M);
      if (on) on[g] = mp_num_node(hn[a], hn[b], hz[a], hz[b], i, M);
    }
    return 0;
  }
  int mid(const fpm* hd, fpm* hr, uint32_t log2d, uint64_t children) {
    for (uint64_t g = 0; g < (children / 2) << log2d; ++g) {
      const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1), a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
      fpm oa, ob;
      mp_mid(hd[g], hr[a], hr[b], &oa, &ob, M);
      hr[a] = oa;
      hr[b] = ob;
    }
    return 0;
  }
  int newton(const fpm* F, fpm* G, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) G[i] = mp_newton(F[i], G[i], M);
    return 0;
  }
  int inv1(const fpm* src, fpm* dst) {
    *dst = mp_inv1(*src, ms_pm2(M), M);
    return 0;
  }
  int deriv_rev(const fpm* top, fpm* out, uint64_t N, uint64_t n) {
    for (uint64_t k = 0; k < N; ++k) out[k] = mp_deriv_rev(top, N, n, k, M);
    return 0;
  }
  int multi_inv(const fpm* in, fpm* out, uint64_t n);  // below: the tiled decomposition with the production tile
  int weights(const fpm* ys, const fpm* inv, fpm* out, uint64_t n, uint64_t N) {
    for (uint64_t i = 0; i < N; ++i) out[i] = i < n ? mp_weight(ys[i], inv[i], M) : fpm_zero();
    return 0;
  }
  int sub(const fpm* a, const fpm* b, fpm* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = mp_sub(a[i], b[i], M);
    return 0;
  }
  int buf(int slot, uint64_t elems, fpm** out) {
    bufs[slot].assign(elems ? elems : 1, fpm_zero());
    *out = bufs[slot].data();
    return 0;
  }
};

// ---- the batch inversion, tile by tile (modpoly.hip's kernels and run()) --------------------------------------------------------------
static uint32_t g_powers = 0, g_launches = 0;

template <uint32_t L, uint32_t C, class Src>
static void up(const Src& s, const fpm_mod& M, uint64_t count, fpm* next) {
  ++g_launches;
  const uint64_t tiles = (count + L * C - 1) / (L * C);
  V t(2 * L);
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    MpChunk<C> ch;
    for (uint32_t l = 0; l < L; ++l) t[L + l] = mp_chunk_forward<L, C>(s, M, count, tile, l, ch);
    for (uint32_t h = L / 2; h >= 1; h /= 2)
      for (uint32_t l = 0; l < h; ++l) mp_tree_up(t.data(), h + l, M);
    next[tile] = t[1];
  }
}
template <uint32_t L, uint32_t C, class Src>
static void down(const Src& s, const fpm_mod& M, uint64_t count, const fpm* tile_inv) {
  ++g_launches;
  const uint64_t tiles = (count + L * C - 1) / (L * C);
  V t(2 * L);
  std::vector<MpChunk<C>> ch(L);
  for (uint64_t tile = 0; tile < tiles; ++tile) {
    for (uint32_t l = 0; l < L; ++l) t[L + l] = mp_chunk_forward<L, C>(s, M, count, tile, l, ch[l]);
    for (uint32_t h = L / 2; h >= 1; h /= 2)
      for (uint32_t l = 0; l < h; ++l) mp_tree_up(t.data(), h + l, M);
    if (tile_inv) {
      t[1] = tile_inv[tile];
    } else {
      t[1] = mp_top_inv(t[1], ms_pm2(M), M);
      ++g_powers;
    }
    for (uint32_t h = 1; h < L; h *= 2)
      for (uint32_t l = 0; l < h; ++l) mp_tree_down(t.data(), h + l, M);
    for (uint32_t l = 0; l < L; ++l) mp_chunk_backward<L, C>(s, M, count, tile, l, ch[l], t[L + l]);
  }
}
template <uint32_t L, uint32_t C, class Src>
static uint32_t run(const Src& items, const fpm_mod& M, uint64_t n) {
  const IvLevels v = mp_iv_levels<L, C>(n);
  V scratch(v.scratch + 1);
  fpm* sc = scratch.data();
  for (uint32_t j = 0; j + 1 < v.depth; ++j) {
    if (j == 0) up<L, C>(items, M, v.count[0], sc + v.off[1]);
    else up<L, C>(MpMont{sc + v.off[j]}, M, v.count[j], sc + v.off[j + 1]);
  }
  for (int j = (int)v.depth - 1; j >= 0; --j) {
    const fpm* above = j + 1 < (int)v.depth ? sc + v.off[j + 1] : nullptr;
    if (j == 0) down<L, C>(items, M, v.count[0], above);
    else down<L, C>(MpMont{sc + v.off[j]}, M, v.count[j], above);
  }
  return v.depth;
}
int HostOps::multi_inv(const fpm* in, fpm* out, uint64_t n) {
  run<MP_IV_LANES, MP_IV_CHUNK>(MpElems{in, out}, M, n);
  return 0;
}

template <uint32_t L, uint32_t C>
static int go(const std::string& mode, const std::string& dir, const fpm_mod& M) {
  uint32_t depth = 0;
  if (mode == "inv") {
    V x = load(dir + "in");
    if (x.empty()) return 2;
    depth = run<L, C>(MpElems{x.data(), x.data()}, M, x.size());
    store(dir + "out", x, x.size());
  } else {
    V xs = load(dir + "xs"), ys = load(dir + "ys");
    if (xs.empty() || xs.size() % 4 || ys.size() != xs.size()) return 2;
    V out(xs.size());
    depth = run<L, C>(MpRows{xs.data(), ys.data(), out.data()}, M, xs.size() / 4);
    store(dir + "out", out, out.size());
  }
  printf("%u %u %u\n", depth, g_powers, g_launches);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s mul|divmod|zpoly|lagrange DIR ROOT_LOG | inv|interp DIR L C\n", argv[0]);
    return 2;
  }
  const std::string op = argv[1], dir = std::string(argv[2]) + "/";
  const std::vector<uint8_t> mod = slurp(dir + "mod");
  HostOps o;
  if (mod.size() != 32 || !fpm_mod_init(mod.data(), &o.M)) return 4;
  if (op == "inv" || op == "interp") {
    if (argc != 5) return 2;
    const uint32_t L = atoi(argv[3]), C = atoi(argv[4]);
    // the production tiles and a few tiny ones (several levels at n ~ 10^3)
    if (L == MP_IV_LANES && C == MP_IV_CHUNK) return go<MP_IV_LANES, MP_IV_CHUNK>(op, dir, o.M);
    if (L == MP_IV_LANES && C == MP_IV_ROW_CHUNK) return go<MP_IV_LANES, MP_IV_ROW_CHUNK>(op, dir, o.M);
    if (L == 4 && C == 2) return go<4, 2>(op, dir, o.M);
    if (L == 2 && C == 2) return go<2, 2>(op, dir, o.M);
    if (L == 4 && C == 1) return go<4, 1>(op, dir, o.M);
    if (L == 8 && C == 3) return go<8, 3>(op, dir, o.M);
    return 2;
  }
  const std::vector<uint8_t> root = slurp(dir + "root");
  o.root_log = atoi(argv[3]);
  if (root.size() != 32 || o.root_log < 0 || o.root_log > 26) return 4;
  const fpm w = fpm_from_wire_bytes(root.data());
  if (!mn_check_root(w, 1ull << o.root_log, o.M)) return 5;
  o.root_mont = fpm_to_mont(w, o.M);
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
