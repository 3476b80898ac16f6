"""Operands and exact expected results for every primitive of starks_amd/csrc/fp256.cuh, as run elementwise by tests/native/fp256_ops.hip.
Shared by tests/test_field_arith_host.py (CPU: the header's portable C paths) and tests/test_gpu_field_arith.py (GPU: the inline-asm
paths and the C paths with the ballot).

The header keeps values lazily reduced in [0, 2^256).  Which representative an op returns is fixed by its arithmetic, and the models
below compute it with Python integers: a sum folds each carry out of limb 7 back as + c (2^256 == c, c = 2^256 - p), a difference adds
p back while it is negative, and a product folds hi * 2^256 + lo to lo + hi * c until it fits.  Each model is checked against the plain
residue (== the exact value mod p) for every case, so the tests pin both the residue and the exact bytes.

The rare carry and borrow continuations of the header are named in BRANCHES; every vector there is shown, by emulating the limbs up to
the condition the header's comment states, to take its branch.  `layouts` places them on chosen lanes of a wave."""
import functools
import os
import random

import native_harness

P = 2**256 - 2**32 * 351 + 1
M = 1 << 256
C = M - P                       # 351 * 2^32 - 1
M64 = (1 << 64) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "native", "fp256_ops.hip")
I4 = pow(7, (P - 1) // 4, P)    # the 4th root of unity the NTT's 4-point butterfly multiplies by
TWO128 = 1 << 128
INV4 = pow(4, P - 2, P)
SPECIAL_LIMBS = (0, 1, 0x15e, 0xfffffea1, 0xffffffff)   # 0, 1, limb 1 of c, limb 1 of p, all ones
N_RANDOM = 100000
N_RANDOM_SLOW = {"pow": 4000, "inv": 1000}


# ---- the representative each op returns ----------------------------------------------------------------------------------------
def fold(v):
    """hi * 2^256 + lo -> lo + hi * c until below 2^256: fp_reduce_wide, fp_reduce_13 and the carry fold of fp_add."""
    while v >= M:
        v = (v & (M - 1)) + (v >> 256) * C
    return v


def m_add(a, b):
    return fold(a + b)


def m_sub(a, b):
    d = a - b
    while d < 0:        # a borrow: the 256-bit difference d + 2^256 == d + c, and d + 2^256 - c = d + p
        d += P
    return d


def mul2_wide(x, w, w128):
    return (x & (TWO128 - 1)) * w + (x >> 128) * w128


def m_mul(a, b):
    return fold(a * b)


def m_pow(a, e):
    r = 1
    while e:
        if e & 1:
            r = m_mul(r, a)
        a = m_mul(a, a)
        e >>= 1
    return r


def m_inv(a):
    r, b = 1, a
    for i in range(256):
        if ((P - 2) >> i) & 1:
            r = m_mul(r, b)
        b = m_mul(b, b)
    return r


def canon(a):
    return a - P if a >= P else a


def m_div4(a):
    return (a + ((-a) & 3) * P) >> 2


# op -> (operand widths in u32 words, result words, model, exact residue or None where the model is exact)
OPS = {
    "add": ((8, 8), 8, m_add, lambda a, b: (a + b) % P),
    "sub": ((8, 8), 8, m_sub, lambda a, b: (a - b) % P),
    "neg": ((8,), 8, lambda a: m_sub(0, a), lambda a: -a % P),
    "mul": ((8, 8), 8, m_mul, lambda a, b: a * b % P),
    "sqr": ((8,), 8, lambda a: m_mul(a, a), lambda a: a * a % P),
    "mulaa": ((8,), 8, lambda a: m_mul(a, a), lambda a: a * a % P),
    "mul2": ((8, 8, 8), 8, lambda x, w, w128: fold(mul2_wide(x, w, w128)), lambda x, w, w128: x * w % P),
    "mulwide": ((8, 8), 16, lambda a, b: a * b, None),
    "mul2wide": ((8, 8, 8), 13, mul2_wide, None),
    "redwide": ((16,), 8, fold, lambda t: t % P),
    "red13": ((13,), 8, fold, lambda t: t % P),
    "div4": ((8,), 8, m_div4, lambda a: a * INV4 % P),
    "canon": ((8,), 8, canon, lambda a: a % P),
    "eqcanon": ((8, 8), 1, lambda a, b: int((a - b) % P == 0), None),
    "pow": ((8, 2), 8, m_pow, lambda a, e: pow(a, e, P)),
    "inv": ((8,), 8, m_inv, lambda a: pow(a, P - 2, P)),
}


# ---- the rare branches, emulated limb by limb up to the condition each one tests ---------------------------------------------------
def add_branches(a, b):
    """fp_add: -> (carry out of limb 1 after the fold of + c into limbs 0..1, second wrap out of limb 7)"""
    s = a + b
    if s < M:
        return (0, 0)
    s -= M
    return (int((s & M64) + C > M64), int(s + C >= M))


def sub_branches(a, b):
    """fp_sub: -> (borrow out of limb 1 after the fold of - c from limbs 0..1, second borrow out of limb 7)"""
    d = a - b
    if d >= 0:
        return (0, 0)
    s = d + M
    return (int((s & M64) < C), int(s < C))


def wide_branches(t):
    """fp_reduce_wide: R = lo + hi c (10 limbs), then R[0..7] + D with D = (R >> 256) c on limbs 0..2:
    -> (carry out of limb 2, wrap out of limb 7 into fp_add_c_masked_low)"""
    R = (t & (M - 1)) + (t >> 256) * C
    D = (R >> 256) * C
    assert D < 1 << 96
    lo = R & (M - 1)
    return (int((lo & ((1 << 96) - 1)) + D >= 1 << 96), int(lo + D >= M))


def r13_branches(t):
    """fp_reduce_13: lo[0..5] + D[0..5] with D = hi c, hi = t >> 256 < 2^129: -> (carry out of limb 5, its wrap out of limb 7)"""
    assert t < 1 << 385
    lo, D = t & (M - 1), (t >> 256) * C
    return (int((lo & ((1 << 192) - 1)) + D >= 1 << 192), int(lo + D >= M))


def _adds(rng, lo64, top, count):
    """add operands a + b = 2^256 + s with s & (2^64 - 1) drawn by lo64 and s below `top`"""
    out = []
    while len(out) < count:
        s = (rng.randrange(top >> 64) << 64) | lo64(rng)
        if s < top and s + 1 < M:
            a = rng.randrange(s + 1, M)
            out.append((a, M + s - a))
    return out


def _subs(rng, lo64, top, count):
    """sub operands a - b = s - 2^256 with s & (2^64 - 1) drawn by lo64 and 0 < s below `top`"""
    out = []
    while len(out) < count:
        s = (rng.randrange(top >> 64) << 64 if top > 1 << 64 else 0) | lo64(rng)
        if 0 < s < top:
            a = rng.randrange(0, s)
            out.append((a, a + M - s))
    return out


def _branch_vectors():
    rng = random.Random(20261015)
    B = {}
    # fp_add: s = a + b - 2^256 with limb 1 at the carry threshold; below 2^256 - c the propagation stops inside limb 7
    B["add: limb-1 carry after the fold"] = ("add", (1, 0), [(M - 1, (1 << 64) - 4)] + _adds(rng, lambda r: M64 - r.randrange(C - 1), M - C, 5))
    wraps = [(M - 1, M - 1), (M - 1, M - (1 << 32) + 6)]
    for s in (M - C, M - 2, M - 1 - rng.randrange(1, C)):
        a = rng.randrange(s + 1, M)
        wraps.append((a, M + s - a))
    B["add: second wrap"] = ("add", (1, 1), wraps)
    # fp_sub: s = a - b + 2^256 with limb 1 at the borrow threshold; below c the borrow leaves limb 7 a second time
    B["sub: limb-1 borrow"] = ("sub", (1, 0), [((7 << 64) + 2, M - 1)] + _subs(rng, lambda r: r.randrange(C), M, 5))
    B["sub: second borrow"] = ("sub", (1, 1), [(0, M - 5), (0, P + 1)] + _subs(rng, lambda r: r.randrange(C), C, 4))
    # Every branch of the two reductions is reached through a product (fp_mul, fp_mul2); `redwide` and `red13` run the same
    # products' raw values as well (rare_operands).
    # fp_reduce_wide through fp_mul.  The limb-2 carry by a bounded search over random products of operands near 2^256, where the
    # second fold's D = (R >> 256) c is largest (~2^-14 per product).
    found = []
    for _ in range(1000000):
        a, b = M - 1 - rng.getrandbits(250), M - 1 - rng.getrandbits(250)
        if wide_branches(a * b) == (1, 0):
            found.append((a, b))
            if len(found) == 4:
                break
    B["reduce_wide: limb-2 carry"] = ("mul", (1, 0), found)
    # The wrap: a product a b == t (mod p) with c <= t < 2c is returned as t + p >= 2^256 before the wrap, whenever
    # lo + hi c >= 2p -- so a = t / b mod p for a random b.
    wraps = []
    while len(wraps) < 4:
        b = rng.randrange(1, P)
        t = C + rng.randrange(C)
        a = t * pow(b, P - 2, P) % P
        if wide_branches(a * b) == (1, 1):
            wraps.append((a, b))
    B["reduce_wide: wrap out of limb 7"] = ("mul", (1, 1), wraps)
    # fp_reduce_13 through fp_mul2.  w = 2^64 (w128 = 2^192 < p): t = x 2^64, hi = x >> 192, lo = (x mod 2^192) << 64.  With
    # x mod 2^128 all ones and hi >= 2^23, lo mod 2^192 + hi c passes 2^192; with x mod 2^192 all ones it passes 2^256 too.
    # The two x with w = I4 were found by search (tests/test_gpu_parity.py::test_rare_carry_branches).
    w64 = (1 << 64, 1 << 192)
    i4 = (I4, (I4 << 128) % P)
    c5 = [(0xff6a2ad1abf9806db549b1ee5fa97b878013931d44877dfc3495ef6a863f1f72,) + i4,
          (0x73733a361e4774862b504d594c9ae08db9c050b30568b5b6e336370c0edcc14a,) + i4]
    c5 += [((rng.randrange(1 << 23, 1 << 64) << 192) | (rng.randrange(M64) << 128) | (TWO128 - 1),) + w64 for _ in range(3)]
    B["reduce_13: limb-5 carry"] = ("mul2", (1, 0), c5)
    B["reduce_13: wrap out of limb 7"] = ("mul2", (1, 1), [(M - 1,) + w64] + [((rng.randrange(1 << 23, 1 << 64) << 192) | ((1 << 192) - 1),) + w64
                                                                           for _ in range(3)])
    return B


def taken(op, ops):
    """the branch flags of one operand tuple of a product or sum op"""
    if op == "add":
        return add_branches(*ops)
    if op == "sub":
        return sub_branches(*ops)
    if op == "neg":
        return sub_branches(0, *ops)
    if op in ("mul", "mulwide"):
        return wide_branches(ops[0] * ops[1])
    if op in ("mul2", "mul2wide"):
        return r13_branches(mul2_wide(*ops))
    if op == "redwide":
        return wide_branches(ops[0])
    if op == "red13":
        return r13_branches(ops[0])
    return (0, 0)


BRANCHES = _branch_vectors()


def rare_operands(op):
    """{branch name: operand tuples of `op` that take it}: the branch vectors, and their images for the ops that reach the same code"""
    base = {"neg": "sub", "mulwide": "mul", "redwide": "mul", "mul2wide": "mul2", "red13": "mul2"}.get(op, op)
    out = {}
    for name, (bop, _, vecs) in BRANCHES.items():
        if bop != base:
            continue
        if op == "neg":   # 0 - (b - a): the same s = a - b + 2^256, so the same limbs
            vecs = [(b - a,) for a, b in vecs]
        elif op == "redwide":
            vecs = [(a * b,) for a, b in vecs]
        elif op == "red13":
            vecs = [(mul2_wide(*v),) for v in vecs]
        out[name] = vecs
    return out


# ---- edges and random operands -------------------------------------------------------------------------------------------------
def _limbs(ls):
    return sum(v << (32 * i) for i, v in enumerate(ls))


def edge_values():
    E = [0, 1, 2, 3, P - 2, P - 1, P, P + 1, P + 2, C - 1, C, C + 1, M - 1, M - 2, 1 << 255, TWO128 - 1, TWO128 + 1, (1 << 32) - 1]
    # limb 1 at the carry (2^32 - 351 ..) and borrow (.. 350) thresholds, limb 0 and the upper limbs at their extremes
    for l1 in ((1 << 32) - 351, (1 << 32) - 350, (1 << 32) - 2, (1 << 32) - 1, 0, 1, 349, 350):
        for l0 in (0, 0xffffffff):
            for up in (0, 0xffffffff):
                E.append(_limbs([l0, l1] + [up] * 6))
    rng = random.Random(5)
    for _ in range(24):
        E.append(_limbs([rng.choice(SPECIAL_LIMBS) for _ in range(8)]))
    return E


def _biased(rng, bits=256):
    return _limbs([rng.choice(SPECIAL_LIMBS) if rng.random() < 0.5 else rng.getrandbits(32) for _ in range(bits // 32)])


def _value(rng, k, bits=256):
    """k % 3: uniform over [0, 2^bits), uniform over [0, p), limbs biased to SPECIAL_LIMBS"""
    k %= 3
    if k == 0 or bits != 256:
        return rng.getrandbits(bits) if k != 2 else _biased(rng, bits)
    return rng.randrange(P) if k == 1 else _biased(rng)


def _pair128(w, lazy):
    """(w, w 2^128 mod p), the second image canonical or as fp_mul leaves it"""
    return (w, m_mul(w, TWO128) if lazy else (w << 128) % P)


def edge_cases(op):
    E = edge_values()
    widths = OPS[op][0]
    if widths == (8, 8):
        return [(a, b) for a in E for b in E]
    if widths == (8,):
        return [(a,) for a in E]
    if widths == (8, 8, 8):
        return [(x,) + _pair128(w, (i + j) & 1) for i, x in enumerate(E) for j, w in enumerate(E)]
    if op == "pow":
        es = [0, 1, 2, 3, 5, (1 << 64) - 1, 1 << 63, (P - 1) & M64, (P - 2) & M64, 0xfffffea0ffffffff]
        return [(a, e) for a in E for e in es]
    if op == "redwide":
        T = [a * b for a in E[:30] for b in E[:30]] + [(1 << 512) - 1, M * (M - 1), (M - 1) * (M - 1) + M - 1, M, M * P, P * P]
        return [(t,) for t in T] + [(_limbs(ls),) for ls in _limb_rows(16)]
    if op == "red13":
        T = [mul2_wide(x, *_pair128(w, 0)) for x in E[:30] for w in E[:30]]
        T += [(1 << 385) - 1, 1 << 384, (1 << 384) - 1, M, M - 1, M * C, ((M - 1) << 128) + M - 1]
        return [(t,) for t in T] + [(_limbs(ls) & ((1 << 385) - 1),) for ls in _limb_rows(13)]
    raise KeyError(op)


def _limb_rows(n):
    rng = random.Random(n)
    return [[rng.choice(SPECIAL_LIMBS) for _ in range(n)] for _ in range(64)]


def random_cases(op, count=None):
    rng = random.Random("fp256:" + op)
    count = count or N_RANDOM_SLOW.get(op, N_RANDOM)
    widths = OPS[op][0]
    out = []
    for k in range(count):
        if widths == (8, 8):
            a = _value(rng, k)
            if op == "eqcanon" and k % 4 == 3:   # equal residues, as the same value and as the two representatives below 2^256
                a = rng.randrange(C)
                out.append((a, a + P) if k & 4 else (a + P, a))
                continue
            out.append((a, _value(rng, k // 3)))
        elif widths == (8,):
            out.append((_value(rng, k),))
        elif widths == (8, 8, 8):
            out.append((_value(rng, k),) + _pair128(_value(rng, k // 3), k & 1))
        elif op == "pow":
            out.append((_value(rng, k), rng.getrandbits(rng.choice((4, 16, 64)))))
        elif op == "redwide":
            out.append((_value(rng, k, 512),) if k & 1 else (_value(rng, k) * _value(rng, k // 3),))
        elif op == "red13":
            out.append((_value(rng, k, 384) | (rng.getrandbits(1) << 384),) if k & 1 else
                       (mul2_wide(_value(rng, k), *_pair128(_value(rng, k // 3), 0)),))
    return out


# ---- placement on the device: one element per thread, element j on lane j mod 64 (block sizes that are multiples of 64) ---------
def _ordinary(op, rng):
    """an operand tuple that takes no rare branch"""
    while True:
        ops = _fresh(op, rng)
        if taken(op, ops) == (0, 0):
            return ops


def _fresh(op, rng):
    widths = OPS[op][0]
    if widths == (8, 8):
        return (rng.randrange(M), rng.randrange(M))
    if widths == (8,):
        return (rng.randrange(M),)
    if widths == (8, 8, 8):
        return (rng.randrange(M),) + _pair128(rng.randrange(M), 0)
    if op == "pow":
        return (rng.randrange(M), rng.getrandbits(64))
    if op == "redwide":
        return (rng.getrandbits(512),)
    return (rng.getrandbits(385),)


def layouts(op):
    """-> operand tuples, whole waves then a last wave of 13: each rare vector on every lane 0..63 among ordinary lanes; two rare
    lanes per wave (5 and 40, 0 and 63, 31 and 32); a wave of 64 rare lanes; waves mixing the branches; rare lanes in the partial
    last wave.  Empty of rare lanes for an op that reaches none of the branches, which still gets the partial wave."""
    rng = random.Random("layout:" + op)
    rare = [v for vecs in rare_operands(op).values() for v in vecs]
    waves = []

    def wave(slots):
        w = [_ordinary(op, rng) for _ in range(64)]
        for lane, v in slots.items():
            w[lane] = v
        waves.append(w)
    for v in rare:
        for lane in range(64):
            wave({lane: v})
        for lanes in ((5, 40), (0, 63), (31, 32)):
            wave({lanes[0]: v, lanes[1]: rare[(rare.index(v) + 1) % len(rare)]})
        wave({lane: v for lane in range(64)})
    if rare:
        wave({lane: rare[lane % len(rare)] for lane in range(64)})                  # every lane rare, branches mixed
        wave({lane: rare[lane % len(rare)] for lane in range(0, 64, 3)})            # mixed with ordinary lanes
        wave({lane: rare[(lane * 7) % len(rare)] for lane in range(33, 64, 2)})     # upper half only
    tail = [_ordinary(op, rng) for _ in range(13)]
    for i, lane in enumerate((0, 7, 12)):
        if rare:
            tail[lane] = rare[i % len(rare)]
    return [v for w in waves for v in w] + tail


# ---- records and expected bytes ------------------------------------------------------------------------------------------------
def encode(op, cases):
    widths = OPS[op][0]
    return b"".join(v.to_bytes(4 * w, "little") for ops in cases for v, w in zip(ops, widths))


def expected(op, cases):
    """the model's result records; every model result is also checked against the plain residue"""
    _, out_words, model, residue = OPS[op]
    res = []
    for ops in cases:
        r = model(*ops)
        assert 0 <= r < 1 << (32 * out_words), (op, ops)
        if residue is not None:
            assert r % P == residue(*ops), (op, ops)
        res.append(r.to_bytes(4 * out_words, "little"))
    return b"".join(res)


@functools.lru_cache(maxsize=None)
def case_set(op, part):
    """part "main": edges then random operands; part "layout": `layouts(op)`.  -> (operand tuples, input bytes, expected bytes)"""
    cases = edge_cases(op) + random_cases(op) if part == "main" else layouts(op)
    return cases, encode(op, cases), expected(op, cases)


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def build_harness(exe, defines=(), csrc=None):
    """hipcc for gfx950 with the library's flags (-O3, the inline asm on) plus `defines`"""
    return native_harness.build(HARNESS, exe, defines, csrc)


def run_jobs(exe, mode, jobs, workdir, timeout=600):
    """jobs: (op, part, grid, block, tag) -> {tag: result bytes}.  One process runs every job."""
    return native_harness.run_jobs(exe, mode, jobs, workdir, lambda op, part: (len(case_set(op, part)[0]), case_set(op, part)[1]),
                                   timeout)


def mismatches(op, part, got, block=64, limit=5):
    """the first few elements whose result differs from the model, as readable text (lane: within a wave of `block`-thread blocks)"""
    cases, _, want = case_set(op, part)
    w = 4 * OPS[op][1]
    bad = []
    for i in range(len(cases)):
        g, e = got[i * w:(i + 1) * w], want[i * w:(i + 1) * w]
        if g != e:
            bad.append("element %d (lane %d): operands %s: got %s want %s" % (
                i, i % block % 64, [hex(v) for v in cases[i]], hex(int.from_bytes(g, "little")), hex(int.from_bytes(e, "little"))))
            if len(bad) == limit:
                break
    return "%s/%s: %s" % (op, part, "; ".join(bad))
