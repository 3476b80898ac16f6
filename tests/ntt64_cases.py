"""Moduli, roots and inputs of the packed-word transform's tests (test_ntt64_host.py, test_gpu_ntt64.py), on top of modntt_cases: the
oracle is modntt_cases.transform / dft_pow / cyclic_times_n, unchanged.

Every modulus is below 2^64 and odd.  0xffffffffffe40001 = 2^64 - 1835007 is a prime of 2-adicity 18 (base 7): its sums carry out
of 64 bits, with roots up to 2^18.  KoalaBear is 2^31 - 2^24 + 1 (adicity 24, base 3).  2^64 - 59 is the largest prime below 2^64
(adicity 2: n <= 4); 2^64 - 1 is the largest odd modulus and composite: -1 has order 2 there, which is all n <= 2 needs."""
import random
import struct

import modntt_cases as mc

GOLDILOCKS = mc.GOLDILOCKS
BIG18 = 0xffffffffffe40001
BABYBEAR = mc.BABYBEAR
KOALABEAR = 2**31 - 2**24 + 1
P64_59 = 2**64 - 59
ALL_ONES = 2**64 - 1
COMPOSITE = mc.COMPOSITE

# name -> (modulus, 2-adicity, base)
PRIMES = {
    "goldilocks": (GOLDILOCKS, 32, 7),
    "big18": (BIG18, 18, 7),
    "babybear": (BABYBEAR, 27, 11),
    "koalabear": (KOALABEAR, 24, 3),
    "f65537": (65537, 16, 3),
    "f257": (257, 8, 3),
    "f17": (17, 4, 3),
    "f3": (3, 1, 2),
    "p64_59": (P64_59, 2, 2),
}
MODULI = dict({k: v[0] for k, v in PRIMES.items()}, composite=COMPOSITE, all_ones=ALL_ONES)


def max_log(name):
    """largest log2 n the modulus has a root for"""
    return 4 if name == "composite" else 1 if name == "all_ones" else PRIMES[name][1]


def root_of(name, n):
    """a root of order exactly n (a power of two) in Z/MODULI[name]"""
    if name == "composite":
        return mc.root_of("composite", n)
    if name == "all_ones":
        assert n <= 2
        return 1 if n == 1 else ALL_ONES - 1
    p, v, base = PRIMES[name]
    assert n <= 1 << v
    return pow(pow(base, (p - 1) >> v, p), (1 << v) // n, p)


def inputs(seed, count, p):
    """`count` seeded values below 2^64; every fifth one is at or above p where 2^64 - p leaves room"""
    rnd = random.Random(seed)
    out = []
    for i in range(count):
        v = rnd.randrange(p)
        if i % 5 == 2 and p < 2**64:
            v = p + rnd.randrange(2**64 - p)
        out.append(v)
    return out


def words(vals):
    """native 8-byte words (the machines this runs on are little-endian)"""
    vals = [int(v) for v in vals]
    return struct.pack("<%dQ" % len(vals), *vals)


def ints(buf):
    buf = bytes(buf)
    return list(struct.unpack("<%dQ" % (len(buf) // 8), buf))


def limbs(vals):
    """8 x u32 little-endian limbs = 32 little-endian bytes per value"""
    return b"".join(int(v).to_bytes(32, "little") for v in vals)
