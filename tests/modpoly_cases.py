"""Exact Python-int statements of the reference's polynomial arithmetic and batch inversion over ANY prime field (starks/polynomial.py:
116-150, starks/poly_utils.py:301-369, 412-440), the modulus a parameter -- shared by the host and GPU tests of the sh_mod_* polynomial
entries -- and the record format of tests/golden/mod_poly.json: an operand is a literal list or a seeded recipe ({"seed", "n", "big"}:
vec(p, ...), or {"product": [x, y]}), an output is {"len", "sha"} (sha256 of its 32-byte big-endian values) plus "vals" when it has at
most 8 values."""
import hashlib
import struct

MIMC_P = 2**256 - 2**32 * 351 + 1
BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
BLS12_381 = 52435875175126190479447740508185965837690552500527637822603658699938581184513
GOLDILOCKS = 2**64 - 2**32 + 1
BABYBEAR = 15 * 2**27 + 1
KOALABEAR = 2**31 - 2**24 + 1
# modulus -> (2-adicity of p - 1, smallest quadratic non-residue)
FIELDS = {
    BN254: (28, 5), BLS12_381: (32, 5), GOLDILOCKS: (32, 7), BABYBEAR: (27, 11), KOALABEAR: (24, 3),
    65537: (16, 3), 12289: (12, 11), 193: (6, 5), 97: (5, 5), MIMC_P: (32, 3),
}
FIXTURE_MODULI = [BN254, BLS12_381, GOLDILOCKS, 65537, 97]
MAX_ROOT_LOG = 26
OP_MUL, OP_DIVMOD, OP_ZPOLY, OP_LAGRANGE = 0, 1, 2, 3


def two_adic_root(p, g=None):
    """(root of order exactly 2^k, k), k = min(2-adicity of p - 1, 26), from the non-residue g (default: the smallest)"""
    s = ((p - 1) & -(p - 1)).bit_length() - 1
    if g is None:
        g = 2
        while pow(g, (p - 1) // 2, p) != p - 1:
            g += 1
    assert pow(g, (p - 1) // 2, p) == p - 1
    k = min(s, MAX_ROOT_LOG)
    return pow(g, (p - 1) >> k, p), k


def pow2_at_least(n):
    s = 2
    while s < n:
        s *= 2
    return s


def max_transform(op, na, nb=0):
    """the largest transform the drivers run (sh_mod_poly_max_transform's contract in include/starkhip.h)"""
    if op == OP_MUL:
        return pow2_at_least(na + nb - 1) if na and nb else 0
    if op == OP_DIVMOD:
        if nb == 0 or na < nb:
            return 0
        L = na - nb + 1
        s = pow2_at_least(2 * L - 1)
        m = 1
        while m < L:
            s = max(s, pow2_at_least(2 * m + min(2 * m, L) - 2))
            m *= 2
        return max(s, pow2_at_least(na)) if nb > 1 else s
    if op == OP_ZPOLY:
        return pow2_at_least(na) if na else 0
    return 2 * pow2_at_least(na) if na else 0


def seeded(seed, i):
    """BLAKE2s(seed_le64 || i_le64) as a 256-bit integer"""
    return int.from_bytes(hashlib.blake2s(struct.pack("<QQ", seed, i)).digest(), "big")


def vec(p, seed, n, big=0):
    """n values mod p; every big-th one replaced by an unreduced value in [p, 2^256) of the same residue"""
    v = [seeded(seed, i) % p for i in range(n)]
    if big:
        for i in range(0, n, big):
            v[i] += p * ((2**256 - 1 - v[i]) // p)
    return v


def operand(p, spec):
    if isinstance(spec, list):
        return spec
    if "product" in spec:
        x, y = spec["product"]
        return mul(p, operand(p, x), operand(p, y))
    return vec(p, spec["seed"], spec["n"], spec.get("big", 0))


def record(vals):
    vals = [int(v) for v in vals]
    rec = {"len": len(vals), "sha": hashlib.sha256(b"".join(v.to_bytes(32, "big") for v in vals)).hexdigest()}
    if len(vals) <= 8:
        rec["vals"] = vals
    return rec


def matches(rec, vals):
    return record(vals) == rec


def resolved(golden):
    """the fixture's cases with every operand expanded to its list of ints: a list of dicts with "p", "op", "name" and the fields"""
    out = []
    for c in golden["cases"]:
        p = int(c["p"])
        out.append({f: operand(p, v) if f in ("a", "b", "xs", "ys", "in") else v for f, v in c.items()} | {"p": p})
    return out


def wire(p, vals):
    """32-byte big-endian values; a negative or oversized int is stored as its residue"""
    return b"".join((int(v) if 0 <= int(v) < 2**256 else int(v) % p).to_bytes(32, "big") for v in vals)


def ints(raw):
    return [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]


def strip(v):
    v = list(v)
    while v and v[-1] == 0:
        v.pop()
    return v


def mul(p, a, b):
    if not a or not b:
        return []
    a = [x % p for x in a]
    b = [x % p for x in b]
    c = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                c[i + j] += x * y
    return [v % p for v in c]


def divmod_(p, a, b):
    """long division by a divisor with a nonzero last coefficient: (q, r), len(q) = max(na - nb + 1, 0), len(r) = min(na, nb - 1)"""
    a = [x % p for x in a]
    b = [x % p for x in b]
    nq = max(len(a) - len(b) + 1, 0)
    q = [0] * nq
    inv = pow(b[-1], p - 2, p)
    for k in range(nq - 1, -1, -1):
        c = a[k + len(b) - 1] * inv % p
        q[k] = c
        if c:
            for j, y in enumerate(b):
                a[k + j] = (a[k + j] - c * y) % p
    return q, a[:min(len(a), len(b) - 1)]


def zpoly(p, xs):
    r = [1]
    for x in xs:
        x %= p
        r = [((r[k - 1] if k else 0) - x * (r[k] if k < len(r) else 0)) % p for k in range(len(r) + 1)]
    return r


def lagrange(p, xs, ys):
    """O(n^2): Z / (X - x_i) by synthetic division, d_i = prod_{j != i} (x_i - x_j), weights y_i / d_i with 1 for a zero d_i"""
    xs = [x % p for x in xs]
    ys = [y % p for y in ys]
    n = len(xs)
    Z = zpoly(p, xs)
    out = [0] * n
    for i in range(n):
        num = [0] * n  # Z / (X - x_i)
        carry = 0
        for k in range(n, 0, -1):
            carry = (Z[k] + carry * xs[i]) % p if k < n else Z[k]
            num[k - 1] = carry
        d = 1
        for j in range(n):
            if j != i:
                d = d * (xs[i] - xs[j]) % p
        w = ys[i] * (pow(d, p - 2, p) if d else 1) % p
        if w:
            for k in range(n):
                out[k] += num[k] * w
    return [v % p for v in out]


def multi_inv(p, vals):
    """the device contract: the inverse, 0 for a value == 0 mod p"""
    return [pow(v % p, p - 2, p) if v % p else 0 for v in vals]


def multi_interp_4(p, xs, ys):
    """rows of four points (flat lists of 4 rows values) -> flat coefficients, a zero denominator counting as 1"""
    out = []
    for r in range(0, len(xs), 4):
        out += lagrange(p, xs[r:r + 4], ys[r:r + 4])
    return out


def horner(p, coeffs, x):
    y = 0
    for c in reversed(coeffs):
        y = (y * x + c) % p
    return y
