// Both drivers of polynomial evaluation (starks_amd/csrc/poly_items.cuh: pa_eval with pa_eval_direct and pa_eval_tree -- the code
// api_poly.hip runs) on a host back end: a textbook radix-2 NTT over 7^((p - 1) / m) in place of the device plans, and one loop per
// kernel launch over the same element steps, the direct path's workgroups summed lane by lane as poly_eval.hip's direct_kernel does.
// tests/test_poly_eval_host.py compares the results with exact integers.
//   poly_eval_host direct|tree DIR BATCH     DIR/coefs ([BATCH][n]), DIR/xs ([m])  ->  DIR/out ([BATCH][m])
//   poly_eval_host rule N M BATCH            prints 1 when the default rule (pe_direct_preferred) takes the direct path, else 0
// All files are 32-byte big-endian wire form.  Prints "W T G" of the direct path's shape (the tree path prints "N C").
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "poly_items.cuh"

typedef std::vector<fp> V;

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
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t w[8];
    memcpy(w, &b[32 * i], 32);
    v[i] = fp_from_wire_words(w);
  }
  return v;
}
static void store(const std::string& path, const V& v, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  for (size_t i = 0; i < n; ++i) {
    uint32_t w[8];
    fp_to_wire_words(fp_canon(v[i]), w);
    fwrite(w, 1, 32, f);
  }
  fclose(f);
}

static fp pow_limbs(const fp& a, const uint32_t e[8]) {
  fp r = fp_one(), b = a;
  for (int i = 0; i < 256; ++i) {
    if ((e[i / 32] >> (i % 32)) & 1) r = fp_mul(r, b);
    b = fp_sqr(b);
  }
  return r;
}
// 7^((p - 1) / 2^lg)
static fp root_pow2(int lg) {
  const uint32_t pm1[8] = {0u, 0xfffffea1u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  uint32_t e[8];
  for (int i = 0; i < 8; ++i) {
    const int lo = i + lg / 32, sh = lg % 32;
    uint64_t v = lo < 8 ? pm1[lo] : 0;
    if (sh) v = (v >> sh) | ((uint64_t)(lo + 1 < 8 ? pm1[lo + 1] : 0) << (32 - sh));
    e[i] = (uint32_t)v;
  }
  return pow_limbs(fp_from_u32(7u), e);
}

// run_ntt: dst[b][0, n) = the size-n transform of src[b][0, n_in) (zero beyond); inverse = over w^-1 and scaled by n^-1
static void host_ntt(const fp* src, fp* dst, uint64_t batch, uint64_t n, uint64_t n_in, bool inverse) {
  if (n_in == 0 || n_in > n) n_in = n;
  const int lg = (int)pa_log2(n);
  fp w = root_pow2(lg);
  if (inverse) w = fp_pow_u64(w, n - 1);
  fp ninv = fp_one();
  if (inverse) ninv = fp_inv(fp_from_u32((uint32_t)n));
  V a(n);
  for (uint64_t b = 0; b < batch; ++b) {
    for (uint64_t i = 0; i < n; ++i) {
      uint64_t r = 0;
      for (int k = 0; k < lg; ++k) r |= ((i >> k) & 1) << (lg - 1 - k);
      a[r] = i < n_in ? src[b * n_in + i] : fp_zero();
    }
    for (uint64_t len = 2; len <= n; len <<= 1) {
      const fp wl = fp_pow_u64(w, n / len);
      for (uint64_t s = 0; s < n; s += len) {
        fp t = fp_one();
        for (uint64_t k = 0; k < len / 2; ++k) {
          const fp u = a[s + k], v = fp_mul(a[s + k + len / 2], t);
          a[s + k] = fp_add(u, v);
          a[s + k + len / 2] = fp_sub(u, v);
          t = fp_mul(t, wl);
        }
      }
    }
    for (uint64_t i = 0; i < n; ++i) dst[b * n + i] = inverse ? fp_mul(a[i], ninv) : a[i];
  }
}

// poly_items.cuh's Ops on the host: one loop per launch
struct HostOps {
  V bufs[PA_BUF_COUNT];
  int ntt(const fp* src, fp* dst, uint64_t batch, uint64_t n, uint64_t n_in, bool inverse) {
    host_ntt(src, dst, batch, n, n_in, inverse);
    return 0;
  }
  int copy(const PaCopy& c, const fp* src, fp* dst) {
    for (uint64_t r = 0; r < c.rows; ++r)
      for (uint64_t k = 0; k < c.len; ++k) dst[r * c.ds + k] = pa_copy_item(c, src, r, k);
    return 0;
  }
  int tree(const fp* hz, fp* oz, const fp* hn, fp* on, uint32_t log2d, uint64_t nodes) {
    for (uint64_t g = 0; g < (nodes / 2) << log2d; ++g) {
      const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1), a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
      if (oz) oz[g] = pa_tree_node(hz[a], hz[b], i);
      if (on) on[g] = pa_num_node(hn[a], hn[b], hz[a], hz[b], i);
    }
    return 0;
  }
  int mid(const fp* hd, fp* hr, uint32_t log2d, uint64_t children) {
    for (uint64_t g = 0; g < (children / 2) << log2d; ++g) {
      const uint64_t j = g >> log2d, i = g & ((1ull << log2d) - 1), a = ((2 * j) << log2d) + i, b = a + (1ull << log2d);
      const fp ra = hr[a];
      hr[a] = fp_mul(hd[g], hr[b]);
      hr[b] = fp_mul(hd[g], ra);
    }
    return 0;
  }
  int newton(const fp* F, fp* G, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) G[i] = pa_newton(F[i], G[i]);
    return 0;
  }
  int inv1(const fp* src, fp* dst) {
    *dst = fp_inv(fp_canon(*src));
    return 0;
  }
  // the direct path: poly_eval.hip's pow_table_kernel, direct_kernel (a workgroup = PE_WG lanes summed) and sum_kernel
  int eval_pow_table(const fp* xs, uint64_t m, uint32_t lgS, fp* tbl) {
    for (uint64_t i = 0; i < m; ++i) pe_pow_table_item(xs, m, lgS, tbl, i);
    return 0;
  }
  template <int G>
  void direct_group(const PeDirect& s, const fp* coefs, const fp* tbl, fp* dst, uint64_t b, uint64_t grp, uint64_t w) {
    fp sum[G], acc[G];
    for (int q = 0; q < G; ++q) sum[q] = fp_zero();
    for (uint64_t lane = 0; lane < PE_WG; ++lane) {
      pe_lane<G>(s, coefs + b * s.n, tbl, grp * G, w * PE_WG + lane, acc);
      for (int q = 0; q < G; ++q) sum[q] = fp_add(sum[q], acc[q]);
    }
    for (int q = 0; q < G; ++q)
      if (grp * G + q < s.m) dst[(b * s.W + w) * s.m + grp * G + q] = s.W == 1 ? fp_canon(sum[q]) : sum[q];
  }
  int eval_direct(const PeDirect& s, const fp* coefs, const fp* tbl, fp* dst) {
    for (uint64_t b = 0; b < s.batch; ++b)
      for (uint64_t grp = 0; grp < s.groups; ++grp)
        for (uint64_t w = 0; w < s.W; ++w) {
          if (s.G == PE_GROUP) direct_group<PE_GROUP>(s, coefs, tbl, dst, b, grp, w);
          else direct_group<1>(s, coefs, tbl, dst, b, grp, w);
        }
    return 0;
  }
  int eval_sum(const PeDirect& s, const fp* part, fp* out) {
    for (uint64_t b = 0; b < s.batch; ++b)
      for (uint64_t i = 0; i < s.m; ++i) out[b * s.m + i] = pe_sum_item(s, part, b, i);
    return 0;
  }
  // the tree path's kernels
  int eval_chunks(const fp* coefs, uint64_t n, uint64_t batch, uint64_t N, uint64_t C, fp* dst) {
    for (uint64_t r = 0; r < batch * C; ++r)
      for (uint64_t k = 0; k < N; ++k) dst[r * N + k] = pe_chunk_rev_item(coefs, n, N, C, r, k);
    return 0;
  }
  int bcast_mul(fp* a, const fp* b, uint64_t rows, uint64_t len) {
    for (uint64_t g = 0; g < rows * len; ++g) a[g] = fp_mul(a[g], b[g % len]);
    return 0;
  }
  int eval_combine(const fp* leaves, const fp* xs, uint64_t m, uint64_t N, uint64_t C, uint64_t batch, fp* out) {
    for (uint64_t b = 0; b < batch; ++b)
      for (uint64_t i = 0; i < m; ++i) out[b * m + i] = pe_combine_item(leaves, xs, N, C, b, i);
    return 0;
  }
  int buf(int slot, uint64_t elems, fp** out) {
    bufs[slot].assign(elems ? elems : 1, fp_zero());
    *out = bufs[slot].data();
    return 0;
  }
};

int main(int argc, char** argv) {
  if (argc != 4 && !(argc == 5 && std::string(argv[1]) == "rule")) {
    fprintf(stderr, "usage: %s direct|tree DIR BATCH | rule N M BATCH\n", argv[0]);
    return 2;
  }
  const std::string op = argv[1], dir = std::string(argv[2]) + "/";
  const uint64_t batch = strtoull(argv[3], nullptr, 10);
  if (argc == 5 && op == "rule") {
    printf("%d\n", pe_direct_preferred(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10)) ? 1 : 0);
    return 0;
  }
  if (op != "direct" && op != "tree") return 2;
  const V coefs = load(dir + "coefs"), xs = load(dir + "xs");
  if (batch == 0 || coefs.size() % batch) return 2;
  const uint64_t n = coefs.size() / batch, m = xs.size();
  HostOps o;
  V out(batch * m + 1);
  const int rc = pa_eval(o, coefs.data(), n, batch, xs.data(), m, out.data(), op == "direct");
  store(dir + "out", out, batch * m);
  if (op == "direct") {
    const PeDirect s = pe_direct_shape(n, m, batch);
    printf("%llu %llu %u\n", (unsigned long long)s.W, (unsigned long long)s.T, s.G);
  } else {
    const uint64_t N = pa_pow2_at_least(m);
    printf("%llu %llu\n", (unsigned long long)N, (unsigned long long)((n + N - 1) / N));
  }
  return rc;
}
