// Both drivers of polynomial evaluation on packed 64-bit words (starks_amd/csrc/poly_items.cuh: pa_eval with pa_eval_direct and
// pa_eval_tree, instantiated over uint64_t with the element steps of mod64eval_items.cuh -- the code api_mod64poly.hip runs) on a host
// back end: a textbook radix-2 NTT over f64_* in place of the device plans, and one loop per kernel launch over the same element steps,
// the direct path walked workgroup by workgroup, (b, group, w, lane), as mod64eval.hip's m6e_direct_kernel decomposes it.
// tests/test_mod64eval_host.py compares the results with exact integers.
//   mod64eval_host direct|tree|default DIR P ROOT ROOT_LOG BATCH   DIR/coefs ([BATCH][n]), DIR/xs ([m]) -> DIR/out ([BATCH][m])
//        prints "largest-transform-seen mp_max_transform(4, n, m) transforms path A B C": path 1 = direct, then "W T G"; 0 = tree,
//        then "N C 0".  default takes m6e_direct_preferred's choice.
//   mod64eval_host shape FILE             FILE holds lines "n m batch"; prints per line "W T G" of the packed direct shape
//   mod64eval_host prefer FILE ROOT_LOG   prints per line "rule chosen": pe_direct_preferred(M6E_COST, ...), m6e_direct_preferred(...)
//   mod64eval_host consts                 prints M6E_GROUP, then the five constants of M6E_COST
// P and ROOT are decimal; the files hold native 8-byte words.  The host checks of api_mod64poly.hip's eval_check restated, with exit
// codes: 2 usage or a bad file, 3 batch = 0 or coefficients that are no whole polynomials, 4 a refused modulus, 5 a refused root
// (at or above p, or of another order), 6 root_log above 28, 7 a transform above the root's order (a forced tree that does not fit),
// 9 a size above the limits.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "mod64eval_items.cuh"
#include "modpoly_items.cuh"  // mp_max_transform
#include "ntt64_items.cuh"    // n64_check_root, n64_inv_n

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
  if (!f) exit(2);
  if (n) fwrite(v.data(), 8, n, f);  // as stored: the steps store canonical words
  fclose(f);
}

// poly_items.cuh's Ops on the host over the modulus M: one loop per launch (the tree steps are mod64poly_host.cpp's)
struct HostOps {
  f64_mod M;
  uint64_t root_mont;
  int root_log;
  V bufs[PA_BUF_COUNT];

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
  // the direct path: mod64eval.hip's m6e_pow_table_kernel, m6e_direct_kernel (a workgroup = PE_WG lanes summed) and m6e_sum_kernel
  int eval_pow_table(const uint64_t* xs, uint64_t m, uint32_t lgS, uint64_t* tbl) {
    for (uint64_t i = 0; i < m; ++i) m6e_pow_table_item(xs, m, lgS, tbl, i, M);
    return 0;
  }
  template <int G>
  void direct_group(const PeDirect& s, const uint64_t* coefs, const uint64_t* tbl, uint64_t* dst, uint64_t b, uint64_t grp, uint64_t w) {
    uint64_t sum[G], acc[G];
    for (int q = 0; q < G; ++q) sum[q] = 0;
    for (uint64_t lane = 0; lane < PE_WG; ++lane) {
      m6e_lane<G>(s, coefs + b * s.n, tbl, grp * G, w * PE_WG + lane, acc, M);
      for (int q = 0; q < G; ++q) sum[q] = f64_add(sum[q], acc[q], M);
    }
    for (int q = 0; q < G; ++q)
      if (grp * G + q < s.m) dst[(b * s.W + w) * s.m + grp * G + q] = sum[q];
  }
  int eval_direct(const PeDirect& s, const uint64_t* coefs, const uint64_t* tbl, uint64_t* dst) {
    if (s.G != M6E_GROUP && s.G != 1) return 8;
    for (uint64_t b = 0; b < s.batch; ++b)
      for (uint64_t grp = 0; grp < s.groups; ++grp)
        for (uint64_t w = 0; w < s.W; ++w) {
          if (s.G == M6E_GROUP) direct_group<M6E_GROUP>(s, coefs, tbl, dst, b, grp, w);
          else direct_group<1>(s, coefs, tbl, dst, b, grp, w);
        }
    return 0;
  }
  // m6e_sum_kernel: SL = min(W, 64) lanes share an output, lane `sub` adds w = sub, sub + SL, ..., then the lanes' sums are added
  int eval_sum(const PeDirect& s, const uint64_t* part, uint64_t* out) {
    const uint64_t SL = s.W < 64 ? s.W : 64;
    for (uint64_t b = 0; b < s.batch; ++b)
      for (uint64_t i = 0; i < s.m; ++i) {
        uint64_t acc = 0;
        for (uint64_t sub = 0; sub < SL; ++sub) acc = f64_add(acc, m6e_sum_item(s, part, b, i, sub, SL, M), M);
        out[b * s.m + i] = acc;
      }
    return 0;
  }
  // the tree path's kernels
  int eval_chunks(const uint64_t* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, uint64_t* dst) {
    for (uint64_t r = 0; r < batch * C; ++r)
      for (uint64_t k = 0; k < N; ++k) dst[r * N + k] = m6e_chunk_rev_item(coefs, n, N, C, r, k);
    return 0;
  }
  int bcast_mul(uint64_t* a, const uint64_t* b, uint64_t rows, uint64_t len) {
    for (uint64_t g = 0; g < rows * len; ++g) a[g] = m6e_bcast_mul_item(a[g], b[g % len], M);
    return 0;
  }
  int eval_combine(const uint64_t* leaves, const uint64_t* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, uint64_t* out) {
    for (uint64_t b = 0; b < batch; ++b)
      for (uint64_t i = 0; i < m; ++i) out[b * m + i] = m6e_combine_item(leaves, xs, N, C, b, i, M);
    return 0;
  }
  int buf(int slot, uint64_t elems, uint64_t** out) {
    bufs[slot].assign(elems ? elems : 1, 0);
    *out = bufs[slot].data();
    return 0;
  }
};

typedef unsigned long long ull;

int main(int argc, char** argv) {
  const std::string op = argc > 1 ? argv[1] : "";
  if (op == "consts" && argc == 2) {
    printf("%u\n%.17g %.17g %.17g %.17g %.17g\n", M6E_GROUP, M6E_COST.direct_products_per_us, M6E_COST.direct_floor_us,
           M6E_COST.tree_us_per_level, M6E_COST.tree_elements_per_us, M6E_COST.tree_us_per_row);
    return 0;
  }
  if ((op == "shape" && argc == 3) || (op == "prefer" && argc == 4)) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    const uint32_t root_log = op == "prefer" ? (uint32_t)atoi(argv[3]) : 0;
    ull n, m, b;
    while (fscanf(f, "%llu %llu %llu", &n, &m, &b) == 3) {
      if (op == "shape") {
        const PeDirect s = pe_direct_shape_of<pe_group<uint64_t>::value>(n, m, b);
        printf("%llu %llu %u\n", (ull)s.W, (ull)s.T, s.G);
      } else {
        printf("%d %d\n", pe_direct_preferred(M6E_COST, n, m, b) ? 1 : 0, m6e_direct_preferred(n, m, b, root_log) ? 1 : 0);
      }
    }
    fclose(f);
    return 0;
  }
  if ((op != "direct" && op != "tree" && op != "default") || argc != 7) {
    fprintf(stderr, "usage: %s direct|tree|default DIR P ROOT ROOT_LOG BATCH | shape FILE | prefer FILE ROOT_LOG | consts\n", argv[0]);
    return 2;
  }
  const std::string dir = std::string(argv[2]) + "/";
  const uint64_t p = strtoull(argv[3], nullptr, 10), root = strtoull(argv[4], nullptr, 10), batch = strtoull(argv[6], nullptr, 10);
  const long rl = strtol(argv[5], nullptr, 10);
  const V coefs = load(dir + "coefs"), xs = load(dir + "xs");
  // api_mod64poly.hip's eval_check, in its order: limits, then the modulus and the root, then the path
  if (batch == 0 || coefs.size() % batch) return 3;
  const uint64_t n = coefs.size() / batch, m = xs.size();
  if (n > (1ull << 25) || batch * n > (1ull << 26) || m > (1ull << 20)) return 9;
  HostOps o;
  if (!f64_mod_init(p, &o.M)) return 4;
  if (rl < 0 || rl > N64_MAX_LOG_N) return 6;
  o.root_log = (int)rl;
  if (root >= p || !n64_check_root(root, 1ull << o.root_log, o.M)) return 5;
  o.root_mont = f64_to_mont(root, o.M);
  const bool direct = op == "direct" || (op == "default" && m6e_direct_preferred(n, m, batch, (uint32_t)o.root_log));
  if (!direct && mp_max_transform(MP_OP_EVAL, n, m) > (1ull << o.root_log)) return 7;
  V out(batch * m + 1);
  const int rc = pa_eval(o, coefs.data(), n, batch, xs.data(), m, out.data(), direct);
  store(dir + "out", out, batch * m);
  printf("%llu %llu %llu %d ", (ull)g_largest, (ull)mp_max_transform(MP_OP_EVAL, n, m), (ull)g_transforms, direct ? 1 : 0);
  if (direct) {
    const PeDirect s = pe_direct_shape_of<pe_group<uint64_t>::value>(n, m, batch);
    printf("%llu %llu %u\n", (ull)s.W, (ull)s.T, s.G);
  } else {
    const uint64_t N = pa_pow2_at_least(m);
    printf("%llu %llu 0\n", (ull)N, (ull)((n + N - 1) / N));
  }
  return rc;
}
