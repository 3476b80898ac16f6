"""Moduli, roots and the exact oracle of the generic transform's tests (test_modntt_host.py, test_gpu_modntt.py).

Every modulus but the last is prime; `adicity` is the power of two in p - 1 and `base` the smallest x for which
x^((p - 1) / 2^adicity) has full order 2^adicity.  4369 = 17 * 257 is composite: its roots are given per size (129^8 = -1 at n = 16,
253^4 = -1 at n = 8), which is all a transform needs in a ring where 2 is invertible.  The oracle is a recursive radix-2 transform
on Python ints; for n <= 64 `dft_pow` is the definition itself."""
import hashlib
import random

MIMC_P = 2**256 - 351 * 2**32 + 1
BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BLS12_381 = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
SECP256K1_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
GOLDILOCKS = 2**64 - 2**32 + 1
BABYBEAR = 2**31 - 2**27 + 1
COMPOSITE = 4369

# name -> (modulus, 2-adicity, base)
PRIMES = {
    "mimc": (MIMC_P, 32, 3),
    "bn254": (BN254, 28, 5),
    "bls12_381": (BLS12_381, 32, 5),
    "secp256k1_n": (SECP256K1_N, 6, 5),
    "goldilocks": (GOLDILOCKS, 32, 7),
    "babybear": (BABYBEAR, 27, 11),
    "f65537": (65537, 16, 3),
    "f257": (257, 8, 3),
    "f17": (17, 4, 3),
}
COMPOSITE_ROOTS = {16: 129, 8: 253}
MODULI = dict({k: v[0] for k, v in PRIMES.items()}, composite=COMPOSITE)


def max_log(name):
    """largest log2 n the modulus has a root for"""
    return 4 if name == "composite" else PRIMES[name][1]


def root_of(name, n):
    """a root of order exactly n (a power of two) in Z/MODULI[name]"""
    if name == "composite":
        if n in COMPOSITE_ROOTS:
            return COMPOSITE_ROOTS[n]
        return pow(COMPOSITE_ROOTS[16], 16 // n, COMPOSITE)  # n = 1, 2, 4: powers of the 16th root
    p, v, base = PRIMES[name]
    assert n <= 1 << v
    return pow(pow(base, (p - 1) >> v, p), (1 << v) // n, p)


def _rec(vals, p, roots):
    if len(vals) == 1:
        return vals
    even, odd = _rec(vals[0::2], p, roots[0::2]), _rec(vals[1::2], p, roots[0::2])
    h = len(even)
    out = [0] * len(vals)
    for i in range(h):
        t = odd[i] * roots[i] % p
        out[i] = (even[i] + t) % p
        out[i + h] = (even[i] - t) % p
    return out


def transform(vals, n, p, w, inv=False):
    """out[k] = sum_j vals[j] w^(jk) mod p over the zero-padded input; inv: w^-1 and the factor n^-1 (fft_1d, fft.py:316-331)"""
    x = [int(v) % p for v in vals] + [0] * (n - len(vals))
    assert len(x) == n
    g = pow(w, n - 1, p) if inv else w % p
    roots = [1] * n
    for i in range(1, n):
        roots[i] = roots[i - 1] * g % p
    out = _rec(x, p, roots)
    if inv:
        ninv = pow(n, -1, p)
        out = [v * ninv % p for v in out]
    return out


def dft_pow(vals, n, p, w, inv=False):
    """the definition, with pow: n <= 64"""
    x = [int(v) % p for v in vals] + [0] * (n - len(vals))
    g = pow(w, n - 1, p) if inv else w
    s = pow(n, -1, p) if inv else 1
    return [sum(x[j] * pow(g, j * k, p) for j in range(n)) * s % p for k in range(n)]


def mul_polys(a, b, n, p, w):
    """fft.py:334-345: forward, forward, pointwise, the reversed roots and NO 1/n = n * (a b mod x^n - 1)"""
    fa, fb = transform(a, n, p, w), transform(b, n, p, w)
    return [v * n % p for v in transform([x * y % p for x, y in zip(fa, fb)], n, p, w, inv=True)]


def cyclic_times_n(a, b, n, p):
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[(i + j) % n] = (out[(i + j) % n] + x * y) % p
    return [v * n % p for v in out]


def wire(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def ints(buf):
    return [int.from_bytes(buf[i:i + 32], "big") for i in range(0, len(buf), 32)]


def inputs(seed, count, p):
    """`count` seeded values below 2^256; every fifth one is at or above p when 2^256 - p leaves room (wire values may be >= p)"""
    rnd = random.Random(seed)
    out = []
    for i in range(count):
        v = rnd.randrange(p)
        if i % 5 == 2:
            v = p + rnd.randrange(min(2**256 - p, 2**200))
        out.append(v)
    return out


def recorded(vals):
    """What tests/golden/mod_ntt.json keeps of an output list: every value up to 8 of them; beyond that the SHA-256 of the values'
    wire form (32 bytes big-endian each, the bytes sh_mod_ntt returns) with the first four values and the last one, as the other
    fixtures of this directory keep their large outputs.  Equal records = equal bytes."""
    vals = [int(v) for v in vals]
    if len(vals) <= 8:
        return {"n": len(vals), "values": ["%x" % v for v in vals]}
    return {"n": len(vals), "sha256": hashlib.sha256(wire(vals)).hexdigest(), "head": ["%x" % v for v in vals[:4]], "tail": "%x" % vals[-1]}
