"""What the host and GPU tests of the packed-word polynomial entries (sh_mod64_poly_mul .. sh_mod64_multi_interp_4) share: the exact
Python-int statements of tests/modpoly_cases.py as they are, word packing, the modulus table and the size grids.  A word input is any
64-bit value and stands for its residue; an output word is canonical, so it equals the 256-bit value the sh_mod_* twin gives and the
recorded outputs of tests/golden/mod_poly.json (the reference reduces its inputs too)."""
import struct

from modpoly_cases import (BABYBEAR, GOLDILOCKS, KOALABEAR, OP_DIVMOD, OP_LAGRANGE, OP_MUL, OP_ZPOLY,  # noqa: F401
                           divmod_, lagrange, matches, max_transform, mul, multi_interp_4, multi_inv, operand, resolved, strip,
                           two_adic_root, zpoly)

P63 = 0x8000000002F00001  # 9223372036904058881: a prime just above 2^63, 2-adicity 20
BIG = 2**64 - 59          # the largest prime below 2^64, 2-adicity 2
# modulus -> 2-adicity of p - 1
FIELDS = {GOLDILOCKS: 32, P63: 20, BABYBEAR: 27, KOALABEAR: 24, 65537: 16, 12289: 12, 193: 6, 97: 5, 3: 1, BIG: 2}
IDS = {GOLDILOCKS: "goldilocks", P63: "p63", BABYBEAR: "babybear", KOALABEAR: "koalabear", 65537: "f65537", 12289: "f12289", 193: "f193",
       97: "f97", 3: "f3", BIG: "big"}
FIXTURE_MODULI = [GOLDILOCKS, 65537, 97]  # the moduli of tests/golden/mod_poly.json below 2^64
MAX_ROOT_LOG = 28                         # the packed transform's limit; two_adic_root stops at 26

# the size grids of tests/test_modpoly_host.py, with a few tiny pairs that fields of 2-adicity 1 and 2 admit
ZPOLY_SIZES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 127, 128, 129, 255, 300, 511, 512, 513, 1000, 1023, 1024, 1025]
LAGRANGE_SIZES = [1, 2, 3, 5, 8, 9, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 383, 700]
MUL_SIZES = [(1, 1), (1, 2), (2, 3), (1, 9), (2, 2), (31, 33), (64, 64), (65, 64), (200, 57), (511, 514), (1000, 1025)]
DIVMOD_SIZES = [(1, 1), (2, 1), (3, 2), (4, 3), (9, 1), (9, 2), (33, 33), (5, 9), (64, 33), (129, 64), (1000, 3), (1025, 512), (1024, 1023)]
# how many sizes of each grid must have run per field: a condition on the grids, from each field's 2-adicity (97 admits transforms of
# 32: eight zpoly sizes; 3 admits 2 and BIG 4, and Lagrange interpolation of one point already needs 4)
FLOORS = {"zpoly": 8, "lagrange": 8, "mul": 5, "divmod": 7}
SMALL_FLOORS = {3: {"zpoly": 2, "lagrange": 0, "mul": 2, "divmod": 2}, BIG: {"zpoly": 3, "lagrange": 2, "mul": 4, "divmod": 5}}


def floor(p, what):
    return SMALL_FLOORS.get(p, FLOORS)[what]


def is_prime(n):
    """deterministic Miller-Rabin below 3.3 * 10^24 (the first thirteen primes as bases)"""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41)
    if n < 2:
        return False
    for b in bases:
        if n % b == 0:
            return n == b
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def admits(p, op, *sizes):
    return max_transform(op, *sizes) <= 1 << min(FIELDS[p], 26)


def words(p, vals):
    """native 8-byte words; a negative or oversized int is stored as its residue"""
    return struct.pack("=%dQ" % len(vals), *[(int(v) if 0 <= int(v) < 2**64 else int(v) % p) for v in vals])


def unwords(raw):
    raw = bytes(raw)
    return list(struct.unpack("=%dQ" % (len(raw) // 8), raw))


def lifted(p, vals, rnd):
    """the same residues as unreduced words in [p, 2^64) wherever one exists: v + k p for a random k, the largest k now and then"""
    out = []
    for i, v in enumerate(vals):
        v %= p
        kmax = (2**64 - 1 - v) // p
        out.append(v + p * (kmax if i % 3 == 0 else rnd.randint(min(1, kmax), kmax)))
    return out


def fixture_words(p, c):
    """the word operands of a fixture case: every recorded operand reduced mod p (multi_inv's planted zeros applied)"""
    f = {k: [int(v) % p for v in c[k]] for k in ("a", "b", "xs", "ys", "in") if k in c}
    if c["op"] == "multi_inv":
        for i in c["zeros"]:
            f["in"][i] = 0
    return f


def recorded(c):
    return [c["q"], c["r"]] if c["op"] == "divmod" else [c["out"]]


def normal(c, outs):
    """outputs in the form the fixture records them: products, quotients, remainders and interpolants trimmed"""
    return [o if c["op"] in ("zpoly", "multi_inv", "multi_interp_4") else strip(o) for o in outs]
