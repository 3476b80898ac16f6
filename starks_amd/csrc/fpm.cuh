// fpm.cuh -- arithmetic in Z/p for ANY odd modulus 3 <= p < 2^256 given at run time: Montgomery form on 8 x u32 little-endian
// limbs, R = 2^256.  The generic transform (modntt_items.cuh, sh_mod_ntt) is built on it; the MiMC prime keeps its own
// special-form code (fp256.cuh), which nothing here touches.
//
// The modulus travels as an fpm_mod block -- p, R^2 mod p, R mod p and -p^-1 mod 2^32 -- that every kernel takes BY VALUE as a
// kernel argument: there is no __constant__ and no global, so contexts with different moduli run side by side on one device.
// Primality is the caller's business: every function below is exact in the ring Z/p for any odd p.
//
// Contracts (x R^-1 etc. are residues mod p; "canonical" = in [0, p)):
//   fpm_mul(a, b)    = a b R^-1, canonical, for ANY 256-bit a and canonical b.  The running sum of the CIOS loop stays below
//                      p + a < 2^257, i.e. it needs a ninth word for p > 2^255 (the MiMC prime is such a modulus), and ends below
//                      2 p: one conditional subtraction.
//   fpm_add, fpm_sub   canonical operands -> canonical result.
//   fpm_to_mont(a)   = a R for any 256-bit a (wire values may be >= p), fpm_from_mont(a) = a R^-1 for canonical a,
//   fpm_canon(a)     = a mod p for any 256-bit a (two products: no bound on a / p is assumed, p may be 3).
// All of it is plain C++: the 32 x 32 + 64-bit steps are written as uint64_t expressions that compile to v_mad_u64_u32.
// Everything is __host__ __device__; the host builds the constants (fpm_mod_init) and checks roots (fpm_pow) with the same code.
// tests/test_modntt_host.py pins every function against Python ints for ten moduli; tests/test_modarith_host.py (host compile) and
// tests/test_gpu_modarith.py (device compile) pin each one elementwise for thirteen, on every operand class named above.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef FPM_HD  // a host program that walks many instantiations may define it without the inlining
#define FPM_HD __host__ __device__ __forceinline__
#endif

struct fpm {
  uint32_t v[8];
};

struct fpm_mod {
  uint32_t p[8], r2[8], one[8];  // the modulus, R^2 mod p, R mod p (1 in Montgomery form)
  uint32_t n0inv;                // -p^-1 mod 2^32
};

FPM_HD fpm fpm_zero() {
  fpm r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = 0;
  return r;
}
FPM_HD fpm fpm_from_u32(uint32_t x) {
  fpm r = fpm_zero();
  r.v[0] = x;
  return r;
}
FPM_HD fpm fpm_from_words(const uint32_t w[8]) {
  fpm r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = w[i];
  return r;
}
FPM_HD bool fpm_eq(const fpm& a, const fpm& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) d |= a.v[i] ^ b.v[i];
  return d == 0;
}

// t (8 words + the bit `top` above them) >= p ?  then t - p, else t; the result fits 8 words whenever t < 2 p
FPM_HD fpm fpm_cond_sub(const uint32_t t[8], uint32_t top, const fpm_mod& M) {
  uint32_t d[8];
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)t[i] - M.p[i] - borrow;
    d[i] = (uint32_t)x;
    borrow = (x >> 32) & 1;
  }
  const bool take = top != 0 || borrow == 0;  // t >= 2^256 > p, or no borrow: t >= p
  fpm r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = take ? d[i] : t[i];
  return r;
}

FPM_HD fpm fpm_add(const fpm& a, const fpm& b, const fpm_mod& M) {
  uint32_t t[8];
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)a.v[i] + b.v[i] + carry;
    t[i] = (uint32_t)x;
    carry = x >> 32;
  }
  return fpm_cond_sub(t, (uint32_t)carry, M);
}

FPM_HD fpm fpm_sub(const fpm& a, const fpm& b, const fpm_mod& M) {
  uint32_t t[8];
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)a.v[i] - b.v[i] - borrow;
    t[i] = (uint32_t)x;
    borrow = (x >> 32) & 1;
  }
  const uint32_t mask = borrow ? 0xffffffffu : 0u;  // a < b: add p back
  fpm r;
  uint64_t carry = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t x = (uint64_t)t[i] + (M.p[i] & mask) + carry;
    r.v[i] = (uint32_t)x;
    carry = x >> 32;
  }
  return r;
}
FPM_HD fpm fpm_neg(const fpm& a, const fpm_mod& M) { return fpm_sub(fpm_zero(), a, M); }

// a b R^-1 mod p (CIOS: one limb of b per round, the reduction of the lowest word interleaved).  Any a, canonical b.
FPM_HD fpm fpm_mul(const fpm& a, const fpm& b, const fpm_mod& M) {
  uint32_t t[8];
  uint32_t t8 = 0;  // the ninth word: 0 or 1 between rounds
#pragma unroll
  for (int i = 0; i < 8; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint64_t carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t x = (uint64_t)a.v[j] * b.v[i] + t[j] + carry;
      t[j] = (uint32_t)x;
      carry = x >> 32;
    }
    const uint64_t hi = (uint64_t)t8 + carry;  // words 8 and 9 of the sum: below 2^33
    const uint32_t m = t[0] * M.n0inv;
    uint64_t x = (uint64_t)m * M.p[0] + t[0];
    carry = x >> 32;
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      x = (uint64_t)m * M.p[j] + t[j] + carry;
      t[j - 1] = (uint32_t)x;
      carry = x >> 32;
    }
    x = hi + carry;
    t[7] = (uint32_t)x;
    t8 = (uint32_t)(x >> 32);
  }
  return fpm_cond_sub(t, t8, M);
}

FPM_HD fpm fpm_to_mont(const fpm& a, const fpm_mod& M) { return fpm_mul(a, fpm_from_words(M.r2), M); }
FPM_HD fpm fpm_from_mont(const fpm& a, const fpm_mod& M) { return fpm_mul(a, fpm_from_u32(1u), M); }
FPM_HD fpm fpm_canon(const fpm& a, const fpm_mod& M) { return fpm_from_mont(fpm_to_mont(a, M), M); }

// a^e in Montgomery form (a canonical, Montgomery form)
FPM_HD fpm fpm_pow(fpm a, uint64_t e, const fpm_mod& M) {
  fpm r = fpm_from_words(M.one);
  while (e) {
    if (e & 1) r = fpm_mul(r, a, M);
    a = fpm_mul(a, a, M);
    e >>= 1;
  }
  return r;
}

// ---- wire form (32 bytes big-endian) <-> limbs: a byte swap, nothing is reduced ----------------------------------------------
FPM_HD fpm fpm_from_wire_words(const uint32_t w[8]) {
  fpm r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = __builtin_bswap32(w[7 - i]);
  return r;
}
FPM_HD void fpm_to_wire_words(const fpm& a, uint32_t w[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) w[i] = __builtin_bswap32(a.v[7 - i]);
}

// ---- the constants of a modulus (host side of every call; cheap: 512 doublings) ------------------------------------------------
// false: p is even or below 3 (0 and 1 included)
inline bool fpm_mod_init(const uint8_t wire[32], fpm_mod* M) {
  for (int i = 0; i < 8; ++i) {
    const uint8_t* b = wire + 4 * (7 - i);
    M->p[i] = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
  }
  bool high = false;
  for (int i = 1; i < 8; ++i) high = high || M->p[i] != 0;
  if (!(M->p[0] & 1) || (!high && M->p[0] < 3)) return false;
  uint32_t inv = 1;  // p^-1 mod 2^32 by Newton's iteration (p odd): the correct bits double each round
  for (int i = 0; i < 5; ++i) inv *= 2u - M->p[0] * inv;
  M->n0inv = 0u - inv;
  fpm x = fpm_from_u32(1u);  // 2^k mod p by doubling, 1 < p
  for (int k = 1; k <= 512; ++k) {
    x = fpm_add(x, x, *M);
    if (k == 256)
      for (int i = 0; i < 8; ++i) M->one[i] = x.v[i];
  }
  for (int i = 0; i < 8; ++i) M->r2[i] = x.v[i];
  return true;
}
inline fpm fpm_from_wire_bytes(const uint8_t wire[32]) {
  uint32_t w[8];
  for (int i = 0; i < 8; ++i) {
    const uint8_t* b = wire + 4 * i;
    w[i] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  }
  return fpm_from_wire_words(w);
}
inline void fpm_to_wire_bytes(const fpm& a, uint8_t wire[32]) {
  for (int i = 0; i < 8; ++i) {
    const uint32_t x = a.v[7 - i];
    wire[4 * i] = (uint8_t)(x >> 24);
    wire[4 * i + 1] = (uint8_t)(x >> 16);
    wire[4 * i + 2] = (uint8_t)(x >> 8);
    wire[4 * i + 3] = (uint8_t)x;
  }
}
// a < p as integers
inline bool fpm_below_p(const fpm& a, const fpm_mod& M) {
  for (int i = 7; i >= 0; --i)
    if (a.v[i] != M.p[i]) return a.v[i] < M.p[i];
  return false;
}
