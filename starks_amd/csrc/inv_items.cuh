// inv_items.cuh -- the decomposition of the device batch inversion (multi_inv.hip) and the host plan it runs by.
//
// multi_inv (starks/poly_utils.py:301-320) is Montgomery's trick: one inversion of the product of all values, then two products per
// value.  Here the product is a tree.  A TILE of T = L * C items belongs to one workgroup of L lanes; lane l owns the items
// l + L k, k < C, of its tile (coalesced loads), multiplies its item LEAVES into one chunk product, and the L chunk products of a
// tile form a binary product tree (heap layout t[1 .. 2L), t[L + l] = lane l's chunk product, t[1] = the tile's product).  The tile
// products of a level are the items of the next level, until a level fits in one tile; that tile's product is inverted once
// (fp_inv), and on the way down each tile turns the inverse of its product into the inverses of its chunk products
// (inv(ab) b = inv(a)) and each lane walks its chunk backwards: inverse of leaf k = inv(chunk) * prefix_k, then inv *= leaf_k.
//
// An item is a value (IvElems: multi_inv, leaf = the value, 0 replaced by 1 as the reference does, poly_utils.py:305-309) or a row
// of multi_interp_4 (IvRows: leaf = the product of the row's four e_k, poly_utils.py:426-430).  The inverse of a leaf is handed to
// the item's `finish`, which writes the outputs.
//
// Inversion is elementwise: no output depends on how the items are tiled, so the inverses of a batch of arrays are the inverses of
// their concatenation.  Every function here is __host__ __device__ with L and C as template parameters, so
// tests/native/multi_inv_host.cpp runs the same decomposition serially with tiny tiles (several levels at n ~ 10^3) and with the
// production tile.
#pragma once
#include <stdint.h>

#include "fp256.cuh"

constexpr uint32_t IV_LANES = 256;      // lanes per tile (one workgroup)
constexpr uint32_t IV_CHUNK = 4;        // values per lane of multi_inv: T = 1024
constexpr uint32_t IV_ROW_CHUNK = 1;    // rows per lane of multi_interp_4: T = 256 (a row is ~60 products already)
constexpr uint32_t IV_MAX_LEVELS = 40;  // 2^64 items at T = 4 (the smallest tile the host tests use) need 33 levels

FP_HD fp iv_ld(const fp* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return fp_load(p);
#else
  return *p;
#endif
}
FP_HD void iv_st(fp* p, const fp& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  fp_store(p, v);
#else
  *p = v;
#endif
}
FP_HD bool iv_is_zero(const fp& canonical) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= canonical.v[i];
  return d == 0;
}

// ---- items ----------------------------------------------------------------------------------------------------------------------
// Values: out[i] = in[i]^-1 (canonical), 0 for a value == 0 mod p (lazily reduced limbs equal to p included).  in may equal out:
// item i is read and written by one lane only, the read first.
struct IvElems {
  const fp* in;
  fp* out;
  FP_HD fp leaf(uint64_t i, bool& zero) const {
    const fp x = fp_canon(iv_ld(in + i));
    zero = iv_is_zero(x);
    return zero ? fp_one() : x;
  }
  FP_HD void finish(uint64_t i, bool zero, const fp& inv) const { iv_st(out + i, zero ? fp_zero() : fp_canon(inv)); }
};

// Rows of four points: xs[r][0..3], ys[r][0..3] -> coeffs[r][0..3] = sum_k eq_k * y_k * e_k^-1, eq_k = prod_{j != k} (X - x_j) and
// e_k = eq_k(x_k) = prod_{j != k} (x_k - x_j) (poly_utils.py:418-439).  A zero e_k (a repeated x) enters the product as 1 and so comes
// back with the "inverse" 1 -- what the reference's multi_inv returns for a zero field element (it tests the truthiness of an element,
// which is always true, poly_utils.py:317), so a degenerate row gets the reference's coefficients.  coeffs may equal xs or ys.
struct IvRows {
  const fp* xs;
  const fp* ys;
  fp* coeffs;
  // d[] = x_0 - x_1, x_0 - x_2, x_0 - x_3, x_1 - x_2, x_1 - x_3, x_2 - x_3;  e_k with a zero replaced by 1
  FP_HD static void es(const fp x[4], fp e[4]) {
    const fp d01 = fp_sub(x[0], x[1]), d02 = fp_sub(x[0], x[2]), d03 = fp_sub(x[0], x[3]);
    const fp d12 = fp_sub(x[1], x[2]), d13 = fp_sub(x[1], x[3]), d23 = fp_sub(x[2], x[3]);
    e[0] = fp_mul(fp_mul(d01, d02), d03);
    e[1] = fp_neg(fp_mul(fp_mul(d01, d12), d13));
    e[2] = fp_mul(fp_mul(d02, d12), d23);
    e[3] = fp_neg(fp_mul(fp_mul(d03, d13), d23));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      e[k] = fp_canon(e[k]);
      if (iv_is_zero(e[k])) e[k] = fp_one();
    }
  }
  FP_HD void load(uint64_t i, fp x[4]) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = iv_ld(xs + 4 * i + k);
  }
  FP_HD fp leaf(uint64_t i, bool& zero) const {
    fp x[4], e[4];
    load(i, x);
    es(x, e);
    zero = false;
    return fp_mul(fp_mul(e[0], e[1]), fp_mul(e[2], e[3]));
  }
  FP_HD void finish(uint64_t i, bool, const fp& inv) const {
    fp x[4], y[4], e[4];
    load(i, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = iv_ld(ys + 4 * i + k);
    es(x, e);
    // the row's own Montgomery walk: e_k^-1 = inv(e_0 .. e_k) * (e_0 .. e_{k-1})
    const fp p1 = e[0], p2 = fp_mul(p1, e[1]), p3 = fp_mul(p2, e[2]);
    fp I = inv, w[4];
    w[3] = fp_mul(y[3], fp_mul(I, p3));
    I = fp_mul(I, e[3]);
    w[2] = fp_mul(y[2], fp_mul(I, p2));
    I = fp_mul(I, e[2]);
    w[1] = fp_mul(y[1], fp_mul(I, p1));
    I = fp_mul(I, e[1]);
    w[0] = fp_mul(y[0], I);
    // eq_k = X^3 - s1_k X^2 + s2_k X - s3_k over the three other points
    const fp x01 = fp_mul(x[0], x[1]), x02 = fp_mul(x[0], x[2]), x03 = fp_mul(x[0], x[3]);
    const fp x12 = fp_mul(x[1], x[2]), x13 = fp_mul(x[1], x[3]), x23 = fp_mul(x[2], x[3]);
    const fp s1[4] = {fp_add(fp_add(x[1], x[2]), x[3]), fp_add(fp_add(x[0], x[2]), x[3]), fp_add(fp_add(x[0], x[1]), x[3]),
                      fp_add(fp_add(x[0], x[1]), x[2])};
    const fp s2[4] = {fp_add(fp_add(x12, x13), x23), fp_add(fp_add(x02, x03), x23), fp_add(fp_add(x01, x03), x13),
                      fp_add(fp_add(x01, x02), x12)};
    const fp s3[4] = {fp_mul(x12, x[3]), fp_mul(x02, x[3]), fp_mul(x01, x[3]), fp_mul(x01, x[2])};
    fp c0 = fp_mul(s3[0], w[0]), c1 = fp_mul(s2[0], w[0]), c2 = fp_mul(s1[0], w[0]), c3 = w[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      c0 = fp_add(c0, fp_mul(s3[k], w[k]));
      c1 = fp_add(c1, fp_mul(s2[k], w[k]));
      c2 = fp_add(c2, fp_mul(s1[k], w[k]));
      c3 = fp_add(c3, w[k]);
    }
    iv_st(coeffs + 4 * i + 0, fp_canon(fp_neg(c0)));
    iv_st(coeffs + 4 * i + 1, fp_canon(c1));
    iv_st(coeffs + 4 * i + 2, fp_canon(fp_neg(c2)));
    iv_st(coeffs + 4 * i + 3, fp_canon(c3));
  }
};

// ---- one lane's chunk -----------------------------------------------------------------------------------------------------------
template <uint32_t C>
struct IvChunk {
  fp leaf[C], pre[C];  // pre[k] = leaf[0] ... leaf[k - 1]
  bool zero[C];
};
// Item k of lane l in tile `tile`: tile * L * C + k * L + l (below count).  Returns the chunk product (1 for a lane past the end).
template <uint32_t L, uint32_t C, class Src>
FP_HD fp iv_chunk_forward(const Src& s, uint64_t count, uint64_t tile, uint32_t l, IvChunk<C>& ch) {
  const uint64_t base = tile * L * C + l;
#pragma unroll
  for (uint32_t k = 0; k < C; ++k) {
    ch.zero[k] = false;
    ch.leaf[k] = fp_one();
    if (base + (uint64_t)k * L < count) ch.leaf[k] = s.leaf(base + (uint64_t)k * L, ch.zero[k]);
    ch.pre[k] = k == 0 ? fp_one() : k == 1 ? ch.leaf[0] : fp_mul(ch.pre[k - 1], ch.leaf[k - 1]);
  }
  return C == 1 ? ch.leaf[0] : fp_mul(ch.pre[C - 1], ch.leaf[C - 1]);
}
// inv = the inverse of the chunk product: leaf k's inverse is inv(leaf[0 .. k]) * pre[k]
template <uint32_t L, uint32_t C, class Src>
FP_HD void iv_chunk_backward(const Src& s, uint64_t count, uint64_t tile, uint32_t l, const IvChunk<C>& ch, fp inv) {
  const uint64_t base = tile * L * C + l;
#pragma unroll
  for (uint32_t j = 0; j < C; ++j) {  // k = C - 1 .. 0 (a counting-up loop: the unrolled k must stay static, or ch goes to scratch)
    const uint32_t k = C - 1 - j;
    if (base + (uint64_t)k * L < count) s.finish(base + (uint64_t)k * L, ch.zero[k], k == 0 ? inv : fp_mul(inv, ch.pre[k]));
    if (k) inv = fp_mul(inv, ch.leaf[k]);
  }
}

// ---- the tile's product tree (t[1 .. 2L), heap order) -----------------------------------------------------------------------------
// up: every node of one level (nodes h .. 2h - 1, h = L/2, L/4, .., 1), each after the level below it
FP_HD void iv_tree_up(fp* t, uint32_t node) { t[node] = fp_mul(t[2 * node], t[2 * node + 1]); }
// down: t[node] holds the inverse of its product; its children get theirs (levels h = 1, 2, .., L/2, each after the one above)
FP_HD void iv_tree_down(fp* t, uint32_t node) {
  const fp a = t[2 * node], b = t[2 * node + 1], v = t[node];
  t[2 * node] = fp_mul(v, b);
  t[2 * node + 1] = fp_mul(v, a);
}

// ---- host: the levels -----------------------------------------------------------------------------------------------------------
// Level 0 = the n items; level j + 1 = the ceil(count_j / T) tile products of level j, stored at scratch + off[j + 1] (elements);
// the last level (`depth - 1`) holds at most T items and is the single tile whose product is inverted.  A call launches depth - 1
// up passes, the top tile and depth - 1 down passes: 2 depth - 1 launches.
struct IvLevels {
  uint32_t depth;
  uint64_t count[IV_MAX_LEVELS];
  uint64_t off[IV_MAX_LEVELS];  // off[0] is unused (level 0 is the caller's array)
  uint64_t scratch;             // elements of scratch for levels 1 ..
};
inline IvLevels iv_levels(uint64_t n, uint64_t T) {
  IvLevels v{};
  v.depth = 1;
  v.count[0] = n;
  while (v.count[v.depth - 1] > T && v.depth < IV_MAX_LEVELS) {
    const uint64_t c = v.count[v.depth - 1];
    v.off[v.depth] = v.scratch;
    v.count[v.depth] = c / T + (c % T ? 1 : 0);
    v.scratch += v.count[v.depth];
    ++v.depth;
  }
  return v;
}
