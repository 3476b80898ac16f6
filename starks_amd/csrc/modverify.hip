// modverify.hip -- the host verifier of FRI proofs over any odd modulus below 2^256 (host code only; no kernel, no context, no GPU):
//   shk::mod_fri_verify = SmoothSubgroupFRI.verify_proximity_proof (starks/fri.py:268-366) over IntegersModP(p)
//   shk::mod_stark_verify = STARK.verify_proof (starks/stark.py:281-388) over IntegersModP(p), on sh_mod_stark_prove's flat proofs, at the
//                           end of this file: the FRI proof of the linear combination by the code below, then the spot checks
// on the FLAT proofs sh_mod_fri_prove writes (the layout of sh_fri_prove, include/starkhip.h).  It walks one proof serially, as verify.hip
// walks a MiMC proof, on the run-time-modulus arithmetic of fpm.cuh, and shares no code with the batch path (modverify_items.cuh): it
// is the yardstick the batch verifier's statuses are compared with.
//
// Every value read from a proof -- leaves, column values, the final layer, the challenge field(merkle_root) -- is any 256-bit number,
// taken modulo p; nothing is reduced modulo the MiMC prime.  All arithmetic below is in Montgomery form (to_m reduces and converts in
// one product), so two residues compare limb for limb.
//
// p may be composite: root^(n/2) = -1 is all that is asked.  That makes w of order n modulo every prime factor of p, so every w^d - 1,
// 0 < d < n, is a unit, and with them every denominator below -- but x^(p-2) is not its inverse.  The row check needs none (the closed
// form of the fold: I^-1 = w^(3 n/4), two halvings).  The final layer inverts its barycentric denominators by the binary extended
// Euclid algorithm (mod_inverse), which is exact for any unit of any odd modulus.  (The batch path cross-multiplies instead and
// inverts nothing.)
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/starkhip.h"
#include "blake2s.cuh"
#include "fpm.cuh"

namespace {

// ---- BLAKE2s-256 of a byte string (hashlib.blake2s(x).digest(), merkle_tree.py:5) ------------------------------------------------
void m_blake(const uint8_t* msg, size_t len, uint8_t out[32]) {
  uint32_t h[8];
  b2_init(h);
  size_t off = 0;
  uint32_t m[16];
  while (len - off > 64) {
    memcpy(m, msg + off, 64);
    off += 64;
    b2_compress_cpp(h, m, (uint32_t)off, false);
  }
  uint8_t last[64] = {0};
  memcpy(last, msg + off, len - off);
  memcpy(m, last, 64);
  b2_compress_cpp(h, m, (uint32_t)len, true);
  memcpy(out, h, 32);
}
void m_blake_pair(const uint8_t a[32], const uint8_t b[32], uint8_t out[32]) {
  uint8_t buf[64];
  memcpy(buf, a, 32);
  memcpy(buf + 32, b, 32);
  m_blake(buf, 64, out);
}

// ---- get_pseudorandom_indices (utils.py:60-90); the caller has checked that `count` samples fit the proof --------------------------
bool m_sample_indices(const uint8_t entropy[32], uint64_t modulus, uint32_t count, uint32_t exclude, std::vector<uint32_t>* out) {
  if (modulus >= (1ull << 24) || exclude == 1) return false;  // assert modulus < 2**24; division by zero in the reference
  const uint64_t real = exclude ? modulus * (exclude - 1) / exclude : modulus;
  if (real == 0) return false;
  std::vector<uint8_t> data(entropy, entropy + 32);
  while (data.size() < 4ull * count) {
    uint8_t d[32];
    m_blake(data.data() + data.size() - 32, 32, d);
    data.insert(data.end(), d, d + 32);
  }
  out->clear();
  for (uint32_t i = 0; i < count; ++i) {
    const uint32_t w = ((uint32_t)data[4 * i] << 24) | ((uint32_t)data[4 * i + 1] << 16) | ((uint32_t)data[4 * i + 2] << 8) | data[4 * i + 3];
    const uint32_t x = (uint32_t)(w % real);
    out->push_back(exclude ? x + 1 + x / (exclude - 1) : x);
  }
  return true;
}

// ---- verify_branch (merkle_tree.py:71-86) on `entries` 32-byte entries, the leaf first ---------------------------------------------
bool m_verify_branch(const uint8_t root[32], uint64_t index, const uint8_t* proof, uint32_t entries) {
  if (entries < 2) return false;
  const uint64_t half = 1ull << (entries - 1);  // 2**len(proof) // 2
  const uint64_t q = half / 4;
  if (q == 0 || index >= half) return false;
  uint64_t idx = index / q + 4 * (index % q) + half;  // get_index_in_permuted + half
  uint8_t v[32];
  memcpy(v, proof, 32);
  for (uint32_t e = 1; e < entries; ++e, idx >>= 1) {
    uint8_t d[32];
    if (idx & 1)
      m_blake_pair(proof + 32 * e, v, d);
    else
      m_blake_pair(v, proof + 32 * e, d);
    memcpy(v, d, 32);
  }
  return memcmp(v, root, 32) == 0;
}

// the same on a branch of a packed tree (merkle_tree.py:94-119): leaf (leaf_bytes) | sibling leaf (leaf_bytes) | entries - 2 nodes
bool m_verify_packed_branch(const uint8_t root[32], uint64_t index, const uint8_t* proof, uint32_t entries, size_t leaf_bytes) {
  if (entries < 2) return false;
  const uint64_t half = 1ull << (entries - 1);
  const uint64_t q = half / 4;
  if (q == 0 || index >= half) return false;
  uint64_t idx = index / q + 4 * (index % q) + half;
  std::vector<uint8_t> buf(2 * leaf_bytes);
  memcpy(buf.data(), idx & 1 ? proof + leaf_bytes : proof, leaf_bytes);
  memcpy(buf.data() + leaf_bytes, idx & 1 ? proof : proof + leaf_bytes, leaf_bytes);
  uint8_t v[32];
  m_blake(buf.data(), buf.size(), v);
  idx >>= 1;
  const uint8_t* node = proof + 2 * leaf_bytes;
  for (uint32_t e = 2; e < entries; ++e, node += 32, idx >>= 1) {
    uint8_t d[32];
    if (idx & 1)
      m_blake_pair(node, v, d);
    else
      m_blake_pair(v, node, d);
    memcpy(v, d, 32);
  }
  return memcmp(v, root, 32) == 0;
}

// ---- the ring Z/p ---------------------------------------------------------------------------------------------------------------------
struct Ring {
  fpm_mod M;
  fpm to_m(const uint8_t b[32]) const { return fpm_to_mont(fpm_from_wire_bytes(b), M); }  // int.from_bytes(b, 'big') % p
  fpm one() const { return fpm_from_words(M.one); }
  fpm mul(const fpm& a, const fpm& b) const { return fpm_mul(a, b, M); }
  fpm add(const fpm& a, const fpm& b) const { return fpm_add(a, b, M); }
  fpm sub(const fpm& a, const fpm& b) const { return fpm_sub(a, b, M); }
  fpm pow(const fpm& a, uint64_t e) const { return fpm_pow(a, e, M); }
  // x / 2 of a canonical residue: (x + p) / 2 when x is odd (p is odd); the same map in either form
  fpm half(const fpm& x) const {
    uint64_t carry = 0;
    uint32_t t[9];
    const bool odd = x.v[0] & 1;
    for (int i = 0; i < 8; ++i) {
      const uint64_t s = (uint64_t)x.v[i] + (odd ? M.p[i] : 0u) + carry;
      t[i] = (uint32_t)s;
      carry = s >> 32;
    }
    t[8] = (uint32_t)carry;
    fpm r;
    for (int i = 0; i < 8; ++i) r.v[i] = (t[i] >> 1) | (t[i + 1] << 31);
    return r;
  }
};

// 256-bit helpers of the inversion: little-endian limbs
bool is_one(const fpm& a) {
  uint32_t d = a.v[0] ^ 1u;
  for (int i = 1; i < 8; ++i) d |= a.v[i];
  return d == 0;
}
bool is_zero(const fpm& a) {
  uint32_t d = 0;
  for (int i = 0; i < 8; ++i) d |= a.v[i];
  return d == 0;
}
bool geq(const fpm& a, const fpm& b) {
  for (int i = 7; i >= 0; --i)
    if (a.v[i] != b.v[i]) return a.v[i] > b.v[i];
  return true;
}
fpm shr1(const fpm& a) {
  fpm r;
  for (int i = 0; i < 8; ++i) r.v[i] = (a.v[i] >> 1) | (i < 7 ? a.v[i + 1] << 31 : 0u);
  return r;
}
fpm sub_int(const fpm& a, const fpm& b) {  // a - b, a >= b
  fpm r;
  uint64_t borrow = 0;
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)a.v[i] - b.v[i] - borrow;
    r.v[i] = (uint32_t)x;
    borrow = (x >> 32) & 1;
  }
  return r;
}
// a^-1 modulo the odd p for a canonical plain a, by the binary extended Euclid algorithm: x1 a = u and x2 a = v hold modulo p
// throughout, while u and v shrink and keep gcd(u, v) = gcd(a, p); at u = 1 (or v = 1) x1 (x2) is the inverse.  false: a is no unit.
bool mod_inverse(const Ring& R, const fpm& a, fpm* out) {
  fpm u = a, v = fpm_from_words(R.M.p), x1 = fpm_from_u32(1u), x2 = fpm_zero();
  if (is_zero(u)) return false;
  while (!is_one(u) && !is_one(v)) {
    while (!(u.v[0] & 1)) {
      u = shr1(u);
      x1 = R.half(x1);
    }
    while (!(v.v[0] & 1)) {
      v = shr1(v);
      x2 = R.half(x2);
    }
    if (geq(u, v)) {
      u = sub_int(u, v);
      x1 = R.sub(x1, x2);
      if (is_zero(u)) return false;  // u == v > 1: a common factor
    } else {
      v = sub_int(v, u);
      x2 = R.sub(x2, x1);
    }
  }
  *out = is_one(u) ? x1 : x2;
  return true;
}

struct Cursor {
  const uint8_t* p;
  uint64_t left;
  const uint8_t* take(uint64_t n) {
    if (n > left) return nullptr;
    const uint8_t* r = p;
    p += n;
    left -= n;
    return r;
  }
};

int ilog2u(uint64_t n) {
  int k = 0;
  while ((1ull << k) < n) ++k;
  return k;
}

// fri.py:268-366 on the flat layout; w = the root in Montgomery form
int fri_verify(const Ring& R, Cursor cur, const uint8_t merkle_root_in[32], uint64_t n, fpm w, uint64_t md, uint32_t exclude,
               uint32_t samples) {
  uint8_t merkle_root[32];
  memcpy(merkle_root, merkle_root_in, 32);
  uint64_t roudeg = n;
  bool first = true;
  std::vector<uint32_t> ys;
  while (md > 16) {
    if (roudeg < 16) return SH_ERR_INVALID;
    const uint32_t s = first ? samples : 40;  // the prover's recursion falls back to 40 (fri.py:262-266)
    const uint64_t q = roudeg / 4;
    const uint32_t lg = (uint32_t)ilog2u(roudeg), l2 = lg - 1, l1 = lg + 1;
    const uint8_t* root2 = cur.take(32);
    if (!root2) return SH_ERR_INVALID;
    // the round's branches must all be there before anything is derived from `s`: a hostile count costs nothing
    if (cur.left / (32ull * (l2 + 4ull * l1)) < s) return SH_ERR_INVALID;
    if (!m_sample_indices(root2, q, s, exclude, &ys)) return SH_ERR_INVALID;
    const fpm special_x = R.to_m(merkle_root);  // field(m[1]) (fri.py:229), used modulo p
    const fpm inv_i = R.pow(w, 3 * q);          // I^-1 = I^3, I = w^(n_r / 4)
    for (uint32_t i = 0; i < s; ++i) {
      const uint64_t y = ys[i];
      const uint8_t* b0 = cur.take(32ull * l2);
      fpm row[4];
      for (int j = 0; j < 4; ++j) {
        const uint8_t* bj = cur.take(32ull * l1);
        if (!m_verify_branch(merkle_root, y + q * j, bj, l1)) return SH_ERR_REJECTED;
        row[j] = R.to_m(bj);
      }
      if (!m_verify_branch(root2, y, b0, l2)) return SH_ERR_REJECTED;
      // the value at x* of the cubic through (w^(y + j q), row[j]): the fold's closed form in t = x* / w^y
      const fpm t = R.mul(special_x, R.pow(w, (roudeg - y) % roudeg));
      const fpm u0 = R.add(row[0], row[2]), u1 = R.sub(row[0], row[2]), u2 = R.add(row[1], row[3]);
      const fpm u3 = R.mul(R.sub(row[1], row[3]), inv_i);
      const fpm G0 = R.add(u0, u2), G2 = R.sub(u0, u2), G1 = R.add(u1, u3), G3 = R.sub(u1, u3);
      fpm acc = R.add(R.mul(G3, t), G2);
      acc = R.add(R.mul(acc, t), G1);
      acc = R.add(R.mul(acc, t), G0);
      if (!fpm_eq(R.half(R.half(acc)), R.to_m(b0))) return SH_ERR_REJECTED;
    }
    memcpy(merkle_root, root2, 32);
    w = R.pow(w, 4);
    md /= 4;
    roudeg /= 4;
    first = false;
  }
  // the final layer (fri.py:340-366): its Merkle root is the last committed root, and the values off the first maxdeg_plus_1 retained
  // points lie on the interpolant through those
  const uint64_t len = roudeg;
  if (len < 4 || len > cur.left / 32) return SH_ERR_INVALID;  // (before 32 * len: no wrap-around)
  const uint8_t* data = cur.take(32 * len);
  if (!data || cur.left != 0) return SH_ERR_INVALID;
  {
    std::vector<uint8_t> nodes(64 * len, 0);
    const uint64_t q = len / 4;
    for (uint64_t i = 0; i < q; ++i)
      for (uint64_t j = 0; j < 4; ++j) memcpy(&nodes[32 * (len + 4 * i + j)], data + 32 * (i + j * q), 32);  // permute4
    for (uint64_t i = len - 1; i >= 1; --i) m_blake(&nodes[64 * i], 64, &nodes[32 * i]);
    if (memcmp(&nodes[32], merkle_root, 32) != 0) return SH_ERR_REJECTED;
  }
  std::vector<uint64_t> pts;
  for (uint64_t x = 0; x < len; ++x)
    if (!exclude || x % exclude) pts.push_back(x);
  const uint64_t k = md < pts.size() ? md : pts.size();
  std::vector<fpm> xs(len), vals(len);
  xs[0] = R.one();
  for (uint64_t i = 1; i < len; ++i) xs[i] = R.mul(xs[i - 1], w);
  for (uint64_t i = 0; i < len; ++i) vals[i] = R.to_m(data + 32 * i);
  // barycentric form of the interpolant through the first k retained points
  std::vector<fpm> wgt(k);
  const fpm r2 = fpm_from_words(R.M.r2);
  for (uint64_t a = 0; a < k; ++a) {
    fpm den = R.one();
    for (uint64_t b = 0; b < k; ++b)
      if (b != a) den = R.mul(den, R.sub(xs[pts[a]], xs[pts[b]]));
    fpm inv;
    if (!mod_inverse(R, fpm_from_mont(den, R.M), &inv)) return SH_ERR_ROOT_ORDER;  // (unreachable: root^(n/2) = -1 makes den a unit)
    wgt[a] = R.mul(vals[pts[a]], R.mul(inv, r2));
  }
  for (uint64_t t = k; t < pts.size(); ++t) {
    const fpm x = xs[pts[t]];
    fpm total = fpm_zero();
    for (uint64_t a = 0; a < k; ++a) {
      fpm num = wgt[a];
      for (uint64_t b = 0; b < k; ++b)
        if (b != a) num = R.mul(num, R.sub(x, xs[pts[b]]));
      total = R.add(total, num);
    }
    if (!fpm_eq(total, vals[pts[t]])) return SH_ERR_REJECTED;
  }
  return SH_OK;
}

}  // namespace

namespace shk {
int mod_fri_verify(const uint8_t modulus[32], const uint8_t* proof, uint64_t proof_len, const uint8_t merkle_root[32], uint64_t n,
                   const uint8_t root[32], uint64_t maxdeg_plus_1, uint32_t exclude_multiples_of, uint32_t samples) {
  if (!modulus || !proof || !merkle_root || !root) return SH_ERR_INVALID;
  Ring R;
  if (!fpm_mod_init(modulus, &R.M)) return SH_ERR_INVALID;  // even, 0 or 1
  if (n < 4 || (n & (n - 1)) || samples == 0) return SH_ERR_INVALID;
  if (n > (1ull << 26)) return SH_ERR_UNSUPPORTED;  // as sh_mod_fri_prove
  const fpm wp = fpm_from_wire_bytes(root);
  if (!fpm_below_p(wp, R.M)) return SH_ERR_ROOT_ORDER;
  const fpm w = fpm_to_mont(wp, R.M);
  if (!fpm_eq(R.pow(w, n / 2), fpm_neg(R.one(), R.M))) return SH_ERR_ROOT_ORDER;
  return fri_verify(R, Cursor{proof, proof_len}, merkle_root, n, w, maxdeg_plus_1, exclude_multiples_of, samples);
}

// STARK.verify_proof + verify_proof_at_position (stark.py:281-388) over IntegersModP(p) on the flat proof of sh_mod_stark_prove
// (the layout of sh_stark_prove): the FRI proof of the linear combination against l_root, then per sampled position the three Merkle
// branches, the transition constraint and the boundary constraint.  (The linear-combination check is commented out in the reference,
// stark.py:376-384, and is not made.)  Every value -- proof, inputs, outputs, coefficients -- is any 256-bit number taken modulo p.
// The two denominators x - x_last and x_last - 1 are inverted by mod_inverse; both are units wherever G2^(n/2) = -1 (G2 has order n
// modulo every prime factor of p; a sampled position is no multiple of ext, and 0 < (steps - 1) ext < n).
int mod_stark_verify(const uint8_t modulus[32], const uint8_t* proof, uint64_t proof_len, const uint8_t* inputs, const uint8_t* outputs,
                     uint64_t steps, uint32_t ext, uint32_t width, const uint8_t* term_coefs, const uint8_t* term_exps,
                     const uint32_t* term_counts, uint32_t samples) {
  if (!modulus || !proof || !inputs || !outputs || !term_coefs || !term_exps || !term_counts) return SH_ERR_INVALID;
  Ring R;
  if (!fpm_mod_init(modulus, &R.M)) return SH_ERR_INVALID;  // even, 0 or 1
  if (width == 0 || samples == 0) return SH_ERR_INVALID;
  if (steps < 2 || (steps & (steps - 1)) || ext < 2 || (ext & (ext - 1))) return SH_ERR_INVALID;
  if (steps >= (1ull << 24) || ext >= (1u << 24) || steps * ext >= (1ull << 24)) return SH_ERR_INVALID;  // utils.py:69 (no wrap-around)
  if (width > 9) return SH_ERR_UNSUPPORTED;  // get_pseudorandom_ks returns None from 10 on (stark.py:106-126)
  const uint64_t n = steps * ext;
  const uint32_t lg = (uint32_t)ilog2u(n), k = 3 * width;
  uint32_t degree = 0;
  uint64_t total = 0;
  std::vector<uint32_t> tbegin(width + 1, 0);
  for (uint32_t d = 0; d < width; ++d) {
    if (term_counts[d] > 256) return SH_ERR_UNSUPPORTED;
    tbegin[d] = (uint32_t)total;
    total += term_counts[d];
  }
  tbegin[width] = (uint32_t)total;
  if (total > 256) return SH_ERR_UNSUPPORTED;
  if (total == 0) return SH_ERR_INVALID;
  std::vector<fpm> coef(total);
  for (uint32_t t = 0; t < total; ++t) {
    coef[t] = R.to_m(term_coefs + 32 * t);
    uint32_t sum = 0;
    for (uint32_t v = 0; v < width; ++v) sum += term_exps[(size_t)t * width + v];
    if (sum > degree) degree = sum;  // as sh_mod_stark_prove takes it: every listed term counts
  }
  // G2 = 7^((p - 1) // n) (stark.py:205): p - 1 is p without its low bit, the division a shift
  fpm g2 = R.one();
  {
    fpm b = fpm_to_mont(fpm_from_u32(7u), R.M);
    for (uint32_t i = lg; i < 256; ++i) {  // bit i of p - 1 is bit i - lg of the exponent
      const uint32_t bit = i == 0 ? 0u : (R.M.p[i / 32] >> (i % 32)) & 1u;
      if (bit) g2 = R.mul(g2, b);
      b = R.mul(b, b);
    }
  }
  if (!fpm_eq(R.pow(g2, n / 2), fpm_neg(R.one(), R.M))) return SH_ERR_ROOT_ORDER;
  Cursor cur{proof, proof_len};
  const uint8_t* m_root = cur.take(32);
  const uint8_t* l_root = cur.take(32);
  if (!m_root || !l_root) return SH_ERR_INVALID;
  const uint64_t pb = 32ull * (2 * k + (lg - 1)), lb = 32ull * (lg + 1);
  if (cur.left / (2 * pb + lb) < samples) return SH_ERR_INVALID;  // before anything is derived from `samples`: a hostile count costs nothing
  const uint8_t* branches = cur.take((2 * pb + lb) * samples);
  if (!branches) return SH_ERR_INVALID;
  // the low-degree proof of the linear combination (stark.py:287-289)
  const int rc = fri_verify(R, cur, l_root, n, g2, steps * (uint64_t)degree, ext, 40);
  if (rc != SH_OK) return rc;
  std::vector<uint32_t> pos;
  if (!m_sample_indices(l_root, n, samples, ext, &pos)) return SH_ERR_INVALID;
  const fpm r2 = fpm_from_words(R.M.r2);
  const fpm last = R.pow(g2, (steps - 1) * ext);
  fpm inv;
  if (!mod_inverse(R, fpm_from_mont(R.sub(last, R.one()), R.M), &inv)) return SH_ERR_ROOT_ORDER;  // (unreachable: a unit, see above)
  const fpm inv_last_m1 = R.mul(inv, r2);
  std::vector<fpm> px(width), dx(width), bx(width), pg(width);
  for (uint32_t i = 0; i < samples; ++i) {
    const uint8_t* b1 = branches + (2 * pb + lb) * i;
    const uint8_t* b2 = b1 + pb;
    const uint8_t* b3 = b2 + pb;
    const uint64_t x_i = pos[i];
    if (!m_verify_packed_branch(m_root, x_i, b1, lg + 1, 32 * k)) return SH_ERR_REJECTED;
    if (!m_verify_packed_branch(m_root, (x_i + ext) % n, b2, lg + 1, 32 * k)) return SH_ERR_REJECTED;
    if (!m_verify_branch(l_root, x_i, b3, lg + 1)) return SH_ERR_REJECTED;
    for (uint32_t d = 0; d < width; ++d) {
      px[d] = R.to_m(b1 + 32 * d);
      dx[d] = R.to_m(b1 + 32 * (width + d));
      bx[d] = R.to_m(b1 + 32 * (2 * width + d));
      pg[d] = R.to_m(b2 + 32 * d);
    }
    const fpm x = R.pow(g2, x_i);
    const fpm xm = R.sub(x, last);
    if (!mod_inverse(R, fpm_from_mont(xm, R.M), &inv)) return SH_ERR_REJECTED;  // the sampling excludes the trace points
    const fpm zvalue = R.mul(R.sub(R.pow(x, steps), R.one()), R.mul(inv, r2));  // Z(x) = (x^steps - 1) / (x - x_last)
    const fpm z2 = R.mul(R.sub(x, R.one()), xm);
    for (uint32_t d = 0; d < width; ++d) {
      // transition constraint: P_d(g1 x) - step_d(P(x)) = Z(x) D_d(x) (stark.py:355-365)
      fpm acc = fpm_zero();
      for (uint32_t t = tbegin[d]; t < tbegin[d + 1]; ++t) {
        fpm prod = coef[t];
        for (uint32_t v = 0; v < width; ++v)
          for (uint32_t e = 0; e < term_exps[(size_t)t * width + v]; ++e) prod = R.mul(prod, px[v]);
        acc = R.add(acc, prod);
      }
      if (!fpm_eq(R.sub(pg[d], acc), R.mul(zvalue, dx[d]))) return SH_ERR_REJECTED;
      // boundary constraint: B_d(x) Z2(x) + I_d(x) = P_d(x), I_d through (1, input), (x_last, output) (stark.py:367-374)
      const fpm in = R.to_m(inputs + 32 * d), out = R.to_m(outputs + 32 * d);
      const fpm slope = R.mul(R.sub(out, in), inv_last_m1);
      const fpm interp = R.add(R.sub(in, slope), R.mul(slope, x));
      if (!fpm_eq(R.sub(px[d], R.mul(bx[d], z2)), interp)) return SH_ERR_REJECTED;
    }
  }
  return SH_OK;
}
}  // namespace shk
