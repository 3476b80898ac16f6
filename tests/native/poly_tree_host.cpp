// The device polynomial arithmetic's drivers (starks_amd/csrc/poly_items.cuh: pa_mul, pa_divmod, pa_zpoly, pa_lagrange -- the code
// api_poly.hip runs) on a host back end: a textbook radix-2 NTT over 7^((p - 1) / m) in place of the device plans, and one loop per kernel
// launch over the same element steps.  tests/test_poly_arith_host.py compares the results with exact integers.
//   poly_tree_host mul DIR        DIR/a, DIR/b        -> DIR/out        (n_a + n_b - 1 coefficients)
//   poly_tree_host divmod DIR     DIR/a, DIR/b        -> DIR/q, DIR/r
//   poly_tree_host zpoly DIR      DIR/xs              -> DIR/out        (n + 1 coefficients)
//   poly_tree_host lagrange DIR   DIR/xs, DIR/ys      -> DIR/out        (n coefficients)
// All files are 32-byte big-endian wire form.  Prints the number of transforms run.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "poly_items.cuh"

typedef std::vector<fp> V;
static uint64_t g_transforms = 0;

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
    ++g_transforms;
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
  int pointwise(const fp* a, const fp* b, fp* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = fp_mul(a[i], b[i]);
    return 0;
  }
  // the pair loops of poly_arith.hip's tree_kernel and mid_kernel
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
  int deriv_rev(const fp* top, fp* out, uint64_t N, uint64_t n) {
    for (uint64_t k = 0; k < N; ++k) out[k] = pa_deriv_rev(top, N, n, k);
    return 0;
  }
  int multi_inv(const fp* in, fp* out, uint64_t n) {  // 0 for a zero, as sh_dev_multi_inv
    for (uint64_t i = 0; i < n; ++i) {
      const fp v = fp_canon(in[i]);
      out[i] = fp_eq_canon(v, fp_zero()) ? fp_zero() : fp_inv(v);
    }
    return 0;
  }
  int weights(const fp* ys, const fp* inv, fp* out, uint64_t n, uint64_t N) {
    for (uint64_t i = 0; i < N; ++i) out[i] = i < n ? pa_weight(ys[i], inv[i]) : fp_zero();
    return 0;
  }
  int sub(const fp* a, const fp* b, fp* out, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) out[i] = fp_canon(fp_sub(a[i], b[i]));
    return 0;
  }
  int buf(int slot, uint64_t elems, fp** out) {
    bufs[slot].assign(elems ? elems : 1, fp_zero());
    *out = bufs[slot].data();
    return 0;
  }
};

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s mul|divmod|zpoly|lagrange DIR\n", argv[0]);
    return 2;
  }
  const std::string op = argv[1], dir = std::string(argv[2]) + "/";
  HostOps o;
  int rc = 2;
  if (op == "mul") {
    const V a = load(dir + "a"), b = load(dir + "b");
    const uint64_t nc = a.size() + b.size() - 1;
    V out(nc), t1(pa_pow2_at_least(nc)), t2(t1.size());
    rc = pa_mul(o, a.data(), a.size(), b.data(), b.size(), out.data(), t1.data(), t2.data());
    store(dir + "out", out, nc);
  } else if (op == "divmod") {
    const V a = load(dir + "a"), b = load(dir + "b");
    const uint64_t nq = a.size() >= b.size() ? a.size() - b.size() + 1 : 0, nr = a.size() < b.size() - 1 ? a.size() : b.size() - 1;
    V q(nq + 1), r(nr + 1);
    rc = pa_divmod(o, a.data(), a.size(), b.data(), b.size(), q.data(), r.data());
    store(dir + "q", q, nq);
    store(dir + "r", r, nr);
  } else if (op == "zpoly") {
    const V xs = load(dir + "xs");
    V out(xs.size() + 1);
    rc = pa_zpoly(o, xs.data(), xs.size(), out.data());
    store(dir + "out", out, out.size());
  } else if (op == "lagrange") {
    const V xs = load(dir + "xs"), ys = load(dir + "ys");
    V out(xs.size());
    rc = xs.empty() ? 0 : pa_lagrange(o, xs.data(), ys.data(), xs.size(), out.data());
    store(dir + "out", out, out.size());
  }
  printf("%llu\n", (unsigned long long)g_transforms);
  return rc;
}
