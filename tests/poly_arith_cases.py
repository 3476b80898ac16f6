"""Exact Python-int statements of the reference's polynomial arithmetic in the MiMC field (starks/polynomial.py:116-150,
starks/poly_utils.py:322-369), shared by the host and GPU tests of the device polynomial arithmetic, and the record format of
tests/golden/poly_arith.json: an operand is a literal list or a seeded recipe ({"seed", "n", "big"}: vec(), or {"product": [x, y]}),
an output is {"len", "sha"} (sha256 of its canonical wire bytes) plus "vals" when it has at most 8 coefficients."""
import hashlib
import struct

P = 2**256 - 2**32 * 351 + 1


def seeded(seed, i):
    """BLAKE2s(seed_le64 || i_le64) as a 256-bit integer"""
    return int.from_bytes(hashlib.blake2s(struct.pack("<QQ", seed, i)).digest(), "big")


def vec(seed, n, big=0):
    """n values mod p; every big-th one replaced by an unreduced value in [p, 2^256)"""
    v = [seeded(seed, i) % P for i in range(n)]
    if big:
        for i in range(0, n, big):
            v[i] = P + v[i] % (2**256 - P)
    return v


def operand(spec):
    if isinstance(spec, list):
        return spec
    if "product" in spec:
        x, y = spec["product"]
        return mul([v % P for v in operand(x)], [v % P for v in operand(y)])
    return vec(spec["seed"], spec["n"], spec.get("big", 0))


def record(vals):
    vals = [int(v) for v in vals]
    rec = {"len": len(vals), "sha": hashlib.sha256(b"".join(v.to_bytes(32, "big") for v in vals)).hexdigest()}
    if len(vals) <= 8:
        rec["vals"] = vals
    return rec


def resolved(golden):
    """the fixture with every operand expanded to its list of ints"""
    return {k: [{f: operand(v) if f in ("a", "b", "xs", "ys") else v for f, v in c.items()} for c in cases]
            if isinstance(cases, list) else cases for k, cases in golden.items()}


def matches(rec, vals):
    """the coefficients `vals` (ints, trailing zeros stripped) are the recorded output"""
    return record(vals) == rec


def wire(vals):
    return b"".join((int(v) if 0 <= int(v) < 2**256 else int(v) % P).to_bytes(32, "big") for v in vals)


def ints(raw):
    return [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]


def strip(v):
    v = list(v)
    while v and v[-1] == 0:
        v.pop()
    return v


def mul(a, b):
    if not a or not b:
        return []
    c = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            c[i + j] = (c[i + j] + x * y) % P
    return c


def divmod_(a, b):
    """long division by a divisor with a nonzero last coefficient: (q, r), len(q) = max(na - nb + 1, 0), len(r) = min(na, nb - 1)"""
    a = [x % P for x in a]
    b = [x % P for x in b]
    nq = max(len(a) - len(b) + 1, 0)
    q = [0] * nq
    inv = pow(b[-1], P - 2, P)
    for k in range(nq - 1, -1, -1):
        c = a[k + len(b) - 1] * inv % P
        q[k] = c
        for j, y in enumerate(b):
            a[k + j] = (a[k + j] - c * y) % P
    return q, a[:min(len(a), len(b) - 1)]


def zpoly(xs):
    r = [1]
    for x in xs:
        r = mul(r, [(-x) % P, 1])
    return r


def lagrange(xs, ys):
    """O(n^2): Z / (X - x_i) by synthetic division, d_i = prod_{j != i} (x_i - x_j), weights y_i / d_i with 1 for a zero d_i"""
    xs = [x % P for x in xs]
    ys = [y % P for y in ys]
    n = len(xs)
    Z = zpoly(xs)
    out = [0] * n
    for i in range(n):
        num = [0] * n  # Z / (X - x_i)
        carry = 0
        for k in range(n, 0, -1):
            carry = (Z[k] + carry * xs[i]) % P if k < n else Z[k]
            num[k - 1] = carry
        d = 1
        for j in range(n):
            if j != i:
                d = d * (xs[i] - xs[j]) % P
        w = ys[i] * (pow(d, P - 2, P) if d else 1) % P
        for k in range(n):
            out[k] = (out[k] + num[k] * w) % P
    return out


def horner(coeffs, x):
    y = 0
    for c in reversed(coeffs):
        y = (y * x + c) % P
    return y
