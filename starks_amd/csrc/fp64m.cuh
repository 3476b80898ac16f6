// fp64m.cuh -- arithmetic in Z/p for ANY odd modulus 3 <= p < 2^64 given at run time: Montgomery form on one native 64-bit word,
// R = 2^64.  The packed-word transform (ntt64_items.cuh, sh_mod64_ntt) is built on it; fpm.cuh keeps the moduli up to 256 bits.
//
// The modulus travels as an f64_mod block -- p, -p^-1 mod 2^64, R^2 mod p and R mod p -- that every kernel takes BY VALUE as a
// kernel argument: there is no __constant__ and no global, so contexts with different moduli run side by side on one device.
// Primality is the caller's business: every function below is exact in the ring Z/p for any odd p.
//
// Contracts (x R^-1 etc. are residues mod p; "canonical" = in [0, p)):
//   f64_mul(a, b)    = a b R^-1, canonical, for ANY 64-bit a and canonical b.  With t = a b and m = t n0inv mod 2^64 the sum
//                      t + m p is a multiple of 2^64 below 2^64 * 2 p: its upper part needs a 65th bit (the 129th of the sum) for
//                      p > 2^63 and is below 2 p: one conditional subtraction.  The low words of t and m p cancel, so the carry
//                      out of them is (low word of t != 0) and m p's low word is never formed.
//   f64_add, f64_sub   canonical operands -> canonical result; for p > 2^63 the sum carries out of 64 bits.
//   f64_to_mont(a)   = a R for any 64-bit a, f64_from_mont(a) = a R^-1 for canonical a,
//   f64_canon(a)     = a mod p for any 64-bit a (two products: no bound on a / p is assumed, p may be 3).
// On the host the products are unsigned __int128; on the device __umul64hi and 64-bit products, which compile to v_mad_u64_u32
// chains.  Everything is __host__ __device__; the host builds the constants (f64_mod_init) and checks roots (f64_pow) with the same
// code.  tests/test_ntt64_host.py pins every function against Python ints; tests/test_modarith_host.py (host compile) and
// tests/test_gpu_modarith.py (device compile, __umul64hi) pin each one elementwise on every operand class named above.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define F64_HD __host__ __device__ __forceinline__

struct f64_mod {
  uint64_t p, n0inv, r2, one;  // the modulus, -p^-1 mod 2^64, R^2 mod p, R mod p (1 in Montgomery form)
};

F64_HD uint64_t f64_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// t (64 bits + the bit `top` above them) >= p ?  then t - p, else t; the result fits the word whenever t < 2 p
F64_HD uint64_t f64_cond_sub(uint64_t t, bool top, const f64_mod& M) { return (top || t >= M.p) ? t - M.p : t; }

F64_HD uint64_t f64_add(uint64_t a, uint64_t b, const f64_mod& M) {
  const uint64_t s = a + b;
  return f64_cond_sub(s, s < a, M);
}
F64_HD uint64_t f64_sub(uint64_t a, uint64_t b, const f64_mod& M) {
  const uint64_t d = a - b;
  return a < b ? d + M.p : d;
}
F64_HD uint64_t f64_neg(uint64_t a, const f64_mod& M) { return a ? M.p - a : 0; }

// a b R^-1 mod p.  Any a, canonical b.
F64_HD uint64_t f64_mul(uint64_t a, uint64_t b, const f64_mod& M) {
  const uint64_t lo = a * b, hi = f64_mulhi(a, b);  // hi <= b - 1 < p
  const uint64_t m = lo * M.n0inv;
  const uint64_t mp = f64_mulhi(m, M.p);            // < p
  const uint64_t s = hi + mp;
  const bool c1 = s < hi;
  const uint64_t s2 = s + (lo != 0 ? 1u : 0u);
  return f64_cond_sub(s2, c1 || s2 < s, M);
}

F64_HD uint64_t f64_to_mont(uint64_t a, const f64_mod& M) { return f64_mul(a, M.r2, M); }
F64_HD uint64_t f64_from_mont(uint64_t a, const f64_mod& M) { return f64_mul(a, 1u, M); }
F64_HD uint64_t f64_canon(uint64_t a, const f64_mod& M) { return f64_from_mont(f64_to_mont(a, M), M); }

// a^e in Montgomery form (a canonical, Montgomery form)
F64_HD uint64_t f64_pow(uint64_t a, uint64_t e, const f64_mod& M) {
  uint64_t r = M.one;
  while (e) {
    if (e & 1) r = f64_mul(r, a, M);
    a = f64_mul(a, a, M);
    e >>= 1;
  }
  return r;
}

// (the 256-bit value of 8 x u32 little-endian limbs) mod p, canonical: Horner over the limbs, two per step, in Montgomery form --
// acc R -> (acc R) R^2 R^-1 + w R = (acc 2^64 + w) R -- and one product with 1 at the end
F64_HD uint64_t f64_from_limbs(const uint32_t w[8], const f64_mod& M) {
  uint64_t acc = 0;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    const uint64_t word = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    acc = f64_add(f64_mul(acc, M.r2, M), f64_to_mont(word, M), M);
  }
  return f64_from_mont(acc, M);
}

// ---- the constants of a modulus (host side of every call; cheap: 128 doublings) -------------------------------------------------------
// false: p is even or below 3 (0 and 1 included)
inline bool f64_mod_init(uint64_t p, f64_mod* M) {
  if (!(p & 1) || p < 3) return false;
  M->p = p;
  uint64_t inv = 1;  // p^-1 mod 2^64 by Newton's iteration (p odd): the correct bits double each round
  for (int i = 0; i < 6; ++i) inv *= 2u - p * inv;
  M->n0inv = 0u - inv;
  uint64_t x = 1;  // 2^k mod p by doubling, 1 < p
  for (int k = 1; k <= 128; ++k) {
    x = f64_add(x, x, *M);
    if (k == 64) M->one = x;
  }
  M->r2 = x;
  return true;
}
