// Both drivers of polynomial evaluation over a run-time modulus (starks_amd/csrc/poly_items.cuh: pa_eval with pa_eval_direct and
// pa_eval_tree, instantiated over fpm with the element steps of modeval_items.cuh -- the code api_modpoly.hip runs) on a host back end:
// a textbook radix-2 NTT over fpm in place of the device plans, and one loop per kernel launch over the same element steps, the direct
// path's workgroups summed lane by lane as modeval.hip's me_direct_kernel does.  tests/test_modeval_host.py compares the results with
// exact integers.
//   modeval_host direct|tree DIR BATCH ROOT_LOG   DIR/coefs ([BATCH][n]), DIR/xs ([m])  ->  DIR/out ([BATCH][m])
//        prints "largest-transform-seen mp_max_transform(4, n, m) transforms W T G" (tree: W T G are "N C 0")
//   modeval_host rules FILE ROOT_LOG              FILE holds lines "n m batch"; prints per line "mimc generic chosen": pe_direct_preferred
//        over the MiMC constants, over ME_COST, and me_direct_preferred(n, m, batch, ROOT_LOG)
//   modeval_host consts                           prints the five constants of PE_COST_MIMC, then of ME_COST
// DIR/mod holds the modulus and DIR/root the root of order 2^ROOT_LOG; all files are 32-byte big-endian wire form.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define FPM_HD __host__ __device__ inline
#include "modeval_items.cuh"

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

// poly_items.cuh's Ops on the host over the modulus M: one loop per launch (the tree steps are modpoly_host.cpp's)
struct HostOps {
  fpm_mod M;
  fpm root_mont;
  int root_log;
  V bufs[PA_BUF_COUNT];

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
  // the direct path: modeval.hip's me_pow_table_kernel, me_direct_kernel (a workgroup = PE_WG lanes summed) and me_sum_kernel
  int eval_pow_table(const fpm* xs, uint64_t m, uint32_t lgS, fpm* tbl) {
    for (uint64_t i = 0; i < m; ++i) me_pow_table_item(xs, m, lgS, tbl, i, M);
    return 0;
  }
  template <int G>
  void direct_group(const PeDirect& s, const fpm* coefs, const fpm* tbl, fpm* dst, uint64_t b, uint64_t grp, uint64_t w) {
    fpm sum[G], acc[G];
    for (int q = 0; q < G; ++q) sum[q] = fpm_zero();
    for (uint64_t lane = 0; lane < PE_WG; ++lane) {
      me_lane<G>(s, coefs + b * s.n, tbl, grp * G, w * PE_WG + lane, acc, M);
      for (int q = 0; q < G; ++q) sum[q] = fpm_add(sum[q], acc[q], M);
    }
    for (int q = 0; q < G; ++q)
      if (grp * G + q < s.m) dst[(b * s.W + w) * s.m + grp * G + q] = sum[q];
  }
  int eval_direct(const PeDirect& s, const fpm* coefs, const fpm* tbl, fpm* dst) {
    if (s.G != ME_GROUP && s.G != 1) return 8;
    for (uint64_t b = 0; b < s.batch; ++b)
      for (uint64_t grp = 0; grp < s.groups; ++grp)
        for (uint64_t w = 0; w < s.W; ++w) {
          if (s.G == ME_GROUP) direct_group<ME_GROUP>(s, coefs, tbl, dst, b, grp, w);
          else direct_group<1>(s, coefs, tbl, dst, b, grp, w);
        }
    return 0;
  }
  int eval_sum(const PeDirect& s, const fpm* part, fpm* out) {
    for (uint64_t b = 0; b < s.batch; ++b)
      for (uint64_t i = 0; i < s.m; ++i) out[b * s.m + i] = me_sum_item(s, part, b, i, M);
    return 0;
  }
  // the tree path's kernels
  int eval_chunks(const fpm* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, fpm* dst) {
    for (uint64_t r = 0; r < batch * C; ++r)
      for (uint64_t k = 0; k < N; ++k) dst[r * N + k] = me_chunk_rev_item(coefs, n, N, C, r, k);
    return 0;
  }
  int bcast_mul(fpm* a, const fpm* b, uint64_t rows, uint64_t len) {
    for (uint64_t g = 0; g < rows * len; ++g) a[g] = me_bcast_mul_item(a[g], b[g % len], M);
    return 0;
  }
  int eval_combine(const fpm* leaves, const fpm* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, fpm* out) {
    for (uint64_t b = 0; b < batch; ++b)
      for (uint64_t i = 0; i < m; ++i) out[b * m + i] = me_combine_item(leaves, xs, N, C, b, i, M);
    return 0;
  }
  int buf(int slot, uint64_t elems, fpm** out) {
    bufs[slot].assign(elems ? elems : 1, fpm_zero());
    *out = bufs[slot].data();
    return 0;
  }
};

static void print_cost(const PeCost& k) {
  printf("%.17g %.17g %.17g %.17g %.17g\n", k.direct_products_per_us, k.direct_floor_us, k.tree_us_per_level, k.tree_elements_per_us,
         k.tree_us_per_row);
}

int main(int argc, char** argv) {
  const std::string op = argc > 1 ? argv[1] : "";
  if (op == "consts" && argc == 2) {
    print_cost(PE_COST_MIMC);
    print_cost(ME_COST);
    return 0;
  }
  if (op == "rules" && argc == 4) {
    FILE* f = fopen(argv[2], "r");
    if (!f) return 2;
    const uint32_t root_log = (uint32_t)atoi(argv[3]);
    unsigned long long n, m, b;
    while (fscanf(f, "%llu %llu %llu", &n, &m, &b) == 3)
      printf("%d %d %d\n", pe_direct_preferred(n, m, b) ? 1 : 0, pe_direct_preferred(ME_COST, n, m, b) ? 1 : 0,
             me_direct_preferred(n, m, b, root_log) ? 1 : 0);
    fclose(f);
    return 0;
  }
  if ((op != "direct" && op != "tree") || argc != 5) {
    fprintf(stderr, "usage: %s direct|tree DIR BATCH ROOT_LOG | rules FILE ROOT_LOG | consts\n", argv[0]);
    return 2;
  }
  const std::string dir = std::string(argv[2]) + "/";
  const uint64_t batch = strtoull(argv[3], nullptr, 10);
  const std::vector<uint8_t> mod = slurp(dir + "mod"), root = slurp(dir + "root");
  HostOps o;
  if (mod.size() != 32 || !fpm_mod_init(mod.data(), &o.M)) return 4;
  o.root_log = atoi(argv[4]);
  if (root.size() != 32 || o.root_log < 0 || o.root_log > 26) return 4;
  const fpm w = fpm_from_wire_bytes(root.data());
  if (!mn_check_root(w, 1ull << o.root_log, o.M)) return 5;
  o.root_mont = fpm_to_mont(w, o.M);
  const V coefs = load(dir + "coefs"), xs = load(dir + "xs");
  if (batch == 0 || coefs.size() % batch) return 2;
  const uint64_t n = coefs.size() / batch, m = xs.size();
  V out(batch * m + 1);
  const int rc = pa_eval(o, coefs.data(), n, batch, xs.data(), m, out.data(), op == "direct");
  store(dir + "out", out, batch * m);
  printf("%llu %llu %llu ", (unsigned long long)g_largest, (unsigned long long)mp_max_transform(MP_OP_EVAL, n, m),
         (unsigned long long)g_transforms);
  if (op == "direct") {
    const PeDirect s = pe_direct_shape_of<pe_group<fpm>::value>(n, m, batch);
    printf("%llu %llu %u\n", (unsigned long long)s.W, (unsigned long long)s.T, s.G);
  } else {
    const uint64_t N = pa_pow2_at_least(m);
    printf("%llu %llu 0\n", (unsigned long long)N, (unsigned long long)((n + N - 1) / N));
  }
  return rc;
}
