"""Operands and exact expected results for the run-time-modulus field arithmetic -- every function of starks_amd/csrc/fpm.cuh (8 x u32
limbs, R = 2^256) and starks_amd/csrc/fp64m.cuh (one 64-bit word, R = 2^64) and the small functions the items headers build on them --
as run elementwise by tests/native/modarith_ops.hip.  Shared by tests/test_modarith_host.py (CPU: the host compile) and
tests/test_gpu_modarith.py (GPU: the device compile, with __umul64hi, the uint4 accesses and the modulus block as a kernel argument).

Every result of these functions is canonical (in [0, p)), so the models are plain residues of Python integers and the comparison is on
exact bytes.  The contracts, as the headers state them:
  mul(a, b)       any a, canonical b      -> a b R^-1 mod p          sqr(a) = mul(a, a), a canonical
  add, sub, neg   canonical operands      -> the sum, difference, negation mod p
  to_mont(a) = a R, from_mont(a) = a R^-1, canon(a) = coef(a) = a mod p, from_limbs(256 bits) = its residue: any value
  pow(a, e), pow_limbs(a, e)              a canonical, in Montgomery form -> (a R^-1)^e R mod p; e = 0 gives R mod p
  half(x)         canonical x             -> x / 2 mod p             below_p(a) = [a < p], any a
  mulp(x, y) = x y mod p, any x and y     msub(a, b) = a - b mod p, any a, canonical b
  inv1(x) = x^(p - 2) mod p, any x, prime moduli only (Fermat); x = 0 mod p gives 0, as the power of 0 does (p - 2 >= 1)
  wire            fpm: the byte-reversed value and its image back; f64: 24 zero bytes, then the word big-endian

The operand classes the headers' comments single out are named by the *_classes functions, which emulate the header's steps up to the
condition; REACHABLE says on which moduli each one can occur (and why not on the others), and class_vectors holds, per modulus, at
least MIN_CLASS vectors of every reachable class -- found by construction and a bounded seeded search, asserted when the set is built.

Counts per op and modulus in part "main": the edge set crossed with itself (about 40 x 40 for the two-operand ops), the class vectors,
and N_RANDOM = 20 000 seeded random operands (2 000 for pow, 500 for pow_limbs and inv1).  Building every set and its expected bytes
takes about 30 s of Python in total on one CPU core, so the counts are the ones the work started from."""
import functools
import os
import random

import modntt_cases as mc
import native_harness
import ntt64_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "native", "modarith_ops.hip")
BITS = {"fpm": 256, "f64": 64}
LIMB = {"fpm": 32, "f64": 64}      # the word of the Montgomery reduction: n0inv = -p^-1 mod 2^LIMB
MODULI = {
    "fpm": dict(mc.MODULI, p256_189=2**256 - 189, f3=3, above255=2**255 + 95),
    "f64": dict(nc.MODULI),
}
N_RANDOM = 20000
N_RANDOM_SLOW = {"pow": 2000, "pow_limbs": 500, "inv1": 500}
MIN_CLASS = 8
SEARCH_LIMIT = 200000
M32 = (1 << 32) - 1


def is_prime(p):
    """Miller-Rabin over fixed bases: exact below 3.3 10^24, and no composite of this module's list passes"""
    if p < 2:
        return False
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41)
    for q in bases:
        if p % q == 0:
            return p == q
    d, s = p - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in bases:
        x = pow(a, d, p)
        if x in (1, p - 1):
            continue
        for _ in range(s - 1):
            x = x * x % p
            if x == p - 1:
                break
        else:
            return False
    return True


# ---- models: (p, R, operands) -> the result as an integer of the result record's width -----------------------------------------------
def _rinv(p, R):
    return pow(R, -1, p)


def _wire_fpm(w):
    v = int.from_bytes(w.to_bytes(32, "little"), "big")   # fpm_from_wire_words: limb i = bswap(word 7 - i)
    return v | (w << 256)                                  # ... and fpm_to_wire_words of it: the words again


def _wire_f64(x):
    return int.from_bytes(bytes(24) + x.to_bytes(8, "big"), "little")


def _pow(p, R, a, e):
    return pow(a * _rinv(p, R) % p, e, p) * R % p


# op -> (operand kinds, result width in records, model).  Kinds: "any" below R, "canon" below p, "e64" / "e256" exponents, "limbs" a
# 256-bit value.  An fpm record is 32 bytes whatever it holds; an f64 record is 8 bytes, a "limbs" operand four of them.
_COMMON = {
    "add": (("canon", "canon"), 1, lambda p, R, a, b: (a + b) % p),
    "sub": (("canon", "canon"), 1, lambda p, R, a, b: (a - b) % p),
    "neg": (("canon",), 1, lambda p, R, a: -a % p),
    "mul": (("any", "canon"), 1, lambda p, R, a, b: a * b * _rinv(p, R) % p),
    "sqr": (("canon",), 1, lambda p, R, a: a * a * _rinv(p, R) % p),
    "to_mont": (("any",), 1, lambda p, R, a: a * R % p),
    "from_mont": (("any",), 1, lambda p, R, a: a * _rinv(p, R) % p),
    "canon": (("any",), 1, lambda p, R, a: a % p),
    "pow": (("canon", "e64"), 1, _pow),
    "half": (("canon",), 1, lambda p, R, x: x * ((p + 1) // 2) % p),
    "coef": (("any",), 1, lambda p, R, a: a % p),
    "mulp": (("any", "any"), 1, lambda p, R, x, y: x * y % p),
    "msub": (("any", "canon"), 1, lambda p, R, a, b: (a - b) % p),
    "inv1": (("any",), 1, lambda p, R, x: pow(x % p, p - 2, p)),
}
OPS = {
    "fpm": dict(_COMMON, wire=(("any",), 2, lambda p, R, w: _wire_fpm(w)), pow_limbs=(("canon", "e256"), 1, _pow),
                below_p=(("any",), 1, lambda p, R, a: int(a < p))),
    "f64": dict(_COMMON, wire=(("any",), 4, lambda p, R, x: _wire_f64(x)), from_limbs=(("limbs",), 1, lambda p, R, v: v % p)),
}
PRIME_ONLY = ("inv1",)


def ops_of(family, name):
    """the ops run for a modulus: inv1 (Fermat) only where it is prime"""
    prime = is_prime(MODULI[family][name])
    return [op for op in sorted(OPS[family]) if prime or op not in PRIME_ONLY]


def _unit(family):
    return BITS[family] // 8


def _width(family, kind):
    return 32 if kind == "limbs" else _unit(family)


# ---- the operand classes, emulated up to the condition each header comment names -----------------------------------------------------
def mul_classes(family, p, a, b):
    """-> (classes, result).  f64_mul: lo, hi = a b; m = lo n0inv; mp = hi word of m p; s = hi + mp ("carry": out of 64 bits);
    s2 = s + (lo != 0) ("wrap": the + 1 wraps the word; "lo_zero": no + 1); f64_cond_sub on (s2, carry or wrap).
    fpm_mul: eight CIOS rounds on a nine-word sum; "ninth": the ninth word is set between two rounds, "top": after the last one;
    fpm_cond_sub.  Both: "taken" / "not_taken": the subtraction; "sum_eq_p": the sum is p exactly; "zero": the result is 0."""
    R, w = 1 << BITS[family], LIMB[family]
    W = (1 << w) - 1
    n0inv = -pow(p, -1, 1 << w) & W
    cls = set()
    if family == "f64":
        t = a * b
        lo, hi = t & W, t >> 64
        mp = ((lo * n0inv & W) * p) >> 64
        s = hi + mp
        if s >> 64:
            cls.add("carry")
        s2 = (s & W) + (lo != 0)
        if s2 >> 64:
            cls.add("wrap")
        if lo == 0:
            cls.add("lo_zero")
        top, t = bool(cls & {"carry", "wrap"}), s2 & W
    else:
        t = 0
        for i in range(8):
            t += a * ((b >> (32 * i)) & M32)
            t = (t + ((t & M32) * n0inv & M32) * p) >> 32
            assert t < 1 << 257
            if t >> 256:
                cls.add("ninth" if i < 7 else "top")
        top, t = "top" in cls, t & (R - 1)
    take = top or t >= p
    cls.add("taken" if take else "not_taken")
    if not top and t == p:
        cls.add("sum_eq_p")
    r = (t - p) % R if take else t
    if r == 0:
        cls.add("zero")
    return cls, r


def add_classes(family, p, a, b):
    """fpm_add / f64_add: "carry": the sum leaves the word or words; "eq_p": it is p exactly"""
    s = a + b
    return ({"carry"} if s >> BITS[family] else set()) | ({"eq_p"} if s == p else set())


def sub_classes(family, p, a, b):
    """fpm_sub / f64_sub: "borrow": a < b, p is added back; "equal": the operands are the same"""
    return ({"borrow"} if a < b else set()) | ({"equal"} if a == b else set())


def half_classes(family, p, x):
    """mf_half / m6_half: "odd_carry": x is odd and x + p leaves the word or words (the bit shifted back in); "odd"; "even" """
    if not x & 1:
        return {"even"}
    return {"odd_carry"} if (x + p) >> BITS[family] else {"odd"}


def coef_classes(family, p, c):
    """me_coef / m6e_coef: "below": c < p, returned as it is; "above": at or above p, the reducing product"""
    return {"below"} if c < p else {"above"}


CLASSIFY = {
    "mul": lambda f, p, v: mul_classes(f, p, *v)[0],
    "add": lambda f, p, v: add_classes(f, p, *v),
    "sub": lambda f, p, v: sub_classes(f, p, *v),
    "half": lambda f, p, v: half_classes(f, p, *v),
    "coef": lambda f, p, v: coef_classes(f, p, *v),
}
# the classes a layout treats as rare lanes among ordinary ones
RARE = {
    "mul": ("lo_zero", "carry", "wrap", "ninth", "top", "sum_eq_p", "zero"),
    "add": ("carry", "eq_p"),
    "sub": ("borrow", "equal"),
    "half": ("odd_carry", "odd"),
    "coef": ("above",),
}


def reachable(family, p, op):
    """The classes of `op` that operands within its contract can reach over p.  With R the word or words:
    add "carry" and half "odd_carry": both operands are below p (half adds p itself), so the sum is below 2 p and leaves R only
      for p > R / 2.
    f64_mul "carry": hi < p and mp < p, so hi + mp reaches 2^64 only for p > 2^63.  "wrap": s + 1 = 2^64 makes the sum R exactly,
      and the sum is below 2 p: again p > 2^63 only.
    fpm_mul "top": the final sum is below 2 p, so it reaches 2^256 only for p > 2^255.  "ninth": after round i, with k = 32 (i + 1),
      the sum is below a (b mod 2^k) / 2^k + p.  For p < 2^k that is below p (2^(256 - k) + 1), which reaches 2^256 only if
      p > 2^k - 1; for p >= 2^k it is below 2^256 - 2^(256 - k) + p, which needs p > 2^(256 - k): together p > 2^128.  Between
      2^128 and 2^255 it takes a first operand at or above p, which fpm_mul's contract allows.
    "lo_zero" belongs to f64_mul alone: fpm_mul forms no low word."""
    R = 1 << BITS[family]
    if op == "mul":
        out = {"taken", "not_taken", "zero", "sum_eq_p"}
        if family == "f64":
            out |= {"lo_zero"} | ({"carry", "wrap"} if 2 * p > R else set())
        else:
            out |= ({"top"} if 2 * p > R else set()) | ({"ninth"} if p > 1 << 128 else set())
        return out
    if op == "add":
        return {"eq_p"} | ({"carry"} if 2 * p > R else set())
    if op == "sub":
        return {"borrow", "equal"}
    if op == "half":
        # "odd" without the carry is an odd x below R - p: none for p = R - 1
        return {"even"} | ({"odd"} if R - p > 1 else set()) | ({"odd_carry"} if 2 * p > R else set())
    if op == "coef":
        return {"below", "above"}
    return set()


def _near(rng, top, bits=20):
    """a value just below `top` (at least 0)"""
    return max(0, top - 1 - rng.getrandbits(rng.choice((0, 3, bits))))


def _candidates(family, p, op, rng):
    """operand tuples of `op`, within its contract, aimed at its classes by construction, then random ones without end"""
    R = 1 << BITS[family]
    if op == "mul":
        for k in range(1, 64):
            a, b = _near(rng, R), _near(rng, p)
            yield (a, b)                                   # both large: the carry, the ninth word, the top bit
            yield (k * p if k * p < R else p, 1 + rng.randrange(p - 1))           # a multiple of p: the sum is p exactly
            yield (rng.randrange(R), 0)
            yield (0, rng.randrange(p))
            yield ((rng.getrandbits(32) << 32) % R, (rng.getrandbits(31) << 32) % p)   # f64: both multiples of 2^32, low word 0
            try:                                           # a b = R^2 (mod p): the result is R mod p = R - p for p > R / 2, where
                yield (a, R * R * pow(a, -1, p) % p)       # the larger representative of the sum is R itself (f64: the + 1 wraps)
                if 2 * p > R:                              # a result r >= R - p: the larger representative r + p of the sum is at
                    r = R - p + rng.randrange(2 * p - R)   # or above R (f64: the carry; fpm: the top bit), however close p is to R / 2
                    yield (a, r * R * pow(a, -1, p) % p)
            except ValueError:
                pass
            for bits in range(32, 256, 32):                # fpm: low limbs of b all ones drive the sum of a middle round past 2^256
                b = rng.randrange(p) | ((1 << bits) - 1)
                if b < p:
                    yield (a, b)
        if 2 * p > R:                                      # p barely above R / 2 (2^255 + 95): the sum reaches R only with a, b and
            for i in range(1, 65):                         # the quotient m all within 2 p - R of their tops, (i + m) p = i j (mod R)
                for j in range(1, 257):                    # for a = R - i, b = p - j: a scan of the small i, j (5 and 114 is one)
                    yield (R - i, p - j)
        while True:
            yield (_value(rng, rng.randrange(3), family, p), rng.randrange(p))
    elif op in ("add", "sub"):
        for k in range(64):
            a = rng.randrange(p)
            yield (a, (p - a) % p if op == "add" else a)   # the sum is p / equal operands
            yield (_near(rng, p), _near(rng, p))
            yield tuple(sorted((a, rng.randrange(p))))     # a <= b
        while True:
            yield (rng.randrange(p), rng.randrange(p))
    elif op == "half":
        for k in range(64):
            yield (_near(rng, p),)
            x = (R - p + rng.getrandbits(16)) | 1          # odd and x + p >= R; canonical only for p > R / 2
            yield (x if x < p else rng.randrange(p),)
            x = rng.randrange(min(p, R - p)) | 1           # odd and x + p < R, when it is below both bounds
            yield (x if x < min(p, R - p) else rng.randrange(p),)
        while True:
            yield (rng.randrange(p),)
    elif op == "coef":
        for k in range(64):
            yield (p + rng.randrange(R - p),)
            yield (min(R - 1, p + rng.getrandbits(8)),)
            yield (_near(rng, p),)
        while True:
            yield (rng.randrange(R),)


@functools.lru_cache(maxsize=None)
def class_vectors(family, name, op):
    """{class: at least MIN_CLASS operand tuples that the classifier shows to be of it}, for every reachable class of `op` over the
    modulus: a bounded search over `_candidates`.  Fails here, on the CPU, when a reachable class stays thin."""
    p = MODULI[family][name]
    want = reachable(family, p, op)
    found = {c: [] for c in sorted(want)}
    if not want:
        return found
    rng = random.Random("classes:%s:%s:%s" % (family, name, op))
    gen = _candidates(family, p, op, rng)
    for _ in range(SEARCH_LIMIT):
        if all(len(v) >= MIN_CLASS for v in found.values()):
            break
        ops = next(gen)
        if op == "mul":
            cls, r = mul_classes(family, p, *ops)
            assert r == OPS[family]["mul"][2](p, 1 << BITS[family], *ops), (family, name, ops)   # the emulation is the function
        else:
            cls = CLASSIFY[op](family, p, ops)
        assert cls <= want, (family, name, op, cls, ops)   # what `reachable` rules out does not occur
        for c in cls & want:
            if len(found[c]) < MIN_CLASS:
                found[c].append(ops)
    thin = {c: len(v) for c, v in found.items() if len(v) < MIN_CLASS}
    assert not thin, "%s %s %s: classes with fewer than %d vectors: %s" % (family, name, op, MIN_CLASS, thin)
    return found


def classes_of(family, name, op, ops):
    return CLASSIFY[op](family, MODULI[family][name], ops)


# ---- edges and random operands -------------------------------------------------------------------------------------------------
def _limbs(ls):
    return sum(v << (32 * i) for i, v in enumerate(ls))


def _special_limbs(p):
    return sorted({0, 1, M32} | {(p >> (32 * i)) & M32 for i in range(8)})


def edge_values(family, p, bits=None):
    """_edges(p) of tests/test_modntt_host.py resp. tests/test_ntt64_host.py, and: p - 2, p + 2, 2 p, 2 p +- 1, R mod p, R^2 mod p,
    multiples of 2^32 and 2^64, rows of limbs drawn from {0, 1, 0xffffffff, a limb of p}; whatever fits below 2^bits"""
    bits = bits or BITS[family]
    R = 1 << BITS[family]
    E = {0, 1, 2, p - 1, p, p + 1, (p + 1) // 2, (1 << bits) - 1, 1 << (bits - 1)}
    E |= {int("ffffffff00000000" * 4, 16)} if bits == 256 else {0xffffffff00000000, 0x00000000ffffffff}
    E |= {p - 2, p + 2, 2 * p - 1, 2 * p, 2 * p + 1, R % p, R * R % p}
    for sh in (32, 64):
        E |= {k << sh for k in (1, 3, M32, (1 << (bits - sh)) - 1)}
    rng = random.Random("rows:%d" % p)
    sp = _special_limbs(p)
    E |= {_limbs([rng.choice(sp) for _ in range(bits // 32)]) for _ in range(12)}
    return sorted(v for v in E if 0 <= v < 1 << bits)


def _value(rng, k, family, p, bits=None):
    """k % 3: uniform below 2^bits, uniform below p, limbs biased to {0, 1, 0xffffffff, a limb of p}"""
    bits = bits or BITS[family]
    k %= 3
    if k == 0:
        return rng.getrandbits(bits)
    if k == 1:
        return rng.randrange(p)
    sp = _special_limbs(p)
    return _limbs([rng.choice(sp) if rng.random() < 0.5 else rng.getrandbits(32) for _ in range(bits // 32)])


def _fit(kind, v, p):
    return v % p if kind == "canon" else v


def _exponents(kind, p):
    top = 64 if kind == "e64" else 256
    return sorted({0, 1, 2, 3, 5, (1 << top) - 1, 1 << (top - 1), (p - 1) & ((1 << top) - 1), (p - 2) & ((1 << top) - 1), 1 << (top // 2)})


def edge_cases(family, name, op):
    p = MODULI[family][name]
    kinds = OPS[family][op][0]
    if kinds == ("limbs",):
        E = edge_values(family, p, 256) + [p << 192, (p << 192) - 1, mc.MIMC_P, 1 << 64, (1 << 64) - 1]
        return [(v,) for v in E if v < 1 << 256]
    E = edge_values(family, p)
    if kinds[-1] in ("e64", "e256"):
        A = E if kinds[-1] == "e64" else E[::3]
        return [(_fit(kinds[0], a, p), e) for a in A for e in _exponents(kinds[-1], p)]
    if len(kinds) == 1:
        return [(_fit(kinds[0], a, p),) for a in E]
    return [(_fit(kinds[0], a, p), _fit(kinds[1], b, p)) for a in E for b in E]


def random_cases(family, name, op, count=None):
    p = MODULI[family][name]
    kinds = OPS[family][op][0]
    rng = random.Random("modarith:%s:%s:%s" % (family, name, op))
    out = []
    for k in range(count or N_RANDOM_SLOW.get(op, N_RANDOM)):
        if kinds == ("limbs",):
            out.append((_value(rng, k, family, p, 256),))
        elif kinds[-1] == "e64":
            out.append((_fit(kinds[0], _value(rng, k, family, p), p), rng.getrandbits(rng.choice((4, 16, 64)))))
        elif kinds[-1] == "e256":
            out.append((_fit(kinds[0], _value(rng, k, family, p), p), rng.getrandbits(rng.choice((8, 64, 256)))))
        elif len(kinds) == 1:
            out.append((_fit(kinds[0], _value(rng, k, family, p), p),))
        else:
            out.append((_fit(kinds[0], _value(rng, k, family, p), p), _fit(kinds[1], _value(rng, k // 3, family, p), p)))
    return out


# ---- placement on the device: one element per thread, element j on lane j mod 64 (block sizes that are multiples of 64) ---------
def _fresh(family, p, op, rng, small=False):
    """random operands within the op's contract; small: an "any" operand is drawn below p (over a small modulus no other draw is)"""
    kinds = OPS[family][op][0]
    draw = {"any": lambda: rng.randrange(p) if small else rng.getrandbits(BITS[family]), "canon": lambda: rng.randrange(p),
            "limbs": lambda: rng.getrandbits(256), "e64": lambda: rng.getrandbits(64), "e256": lambda: rng.getrandbits(256)}
    return tuple(draw[k]() for k in kinds)


def _ordinary(family, p, op, rng):
    """an operand tuple of none of the op's rare classes"""
    for attempt in range(10000):
        ops = _fresh(family, p, op, rng, attempt & 1)
        if op not in RARE or not CLASSIFY[op](family, p, ops) & set(RARE[op]):
            return ops
    raise AssertionError("no ordinary operands for %s %s over %d" % (family, op, p))


def layouts(family, name, op):
    """-> operand tuples, whole waves then a last wave of 13.  An op with classes: each rare vector (two per rare class) on lane 0, 31,
    32 and 63 in turn among ordinary lanes; two rare lanes per wave (5 and 40, 0 and 63, 31 and 32); a wave of 64 rare lanes per
    class; waves mixing the classes, with and without ordinary lanes, and one with the classes split between the wave's halves;
    rare lanes in the partial last wave.  pow and pow_limbs: waves whose lanes hold exponents of every bit length, 0 and 1
    included, so that the lanes of a wave leave the square-and-multiply loop at different rounds.  Every other op: two waves and
    the partial one."""
    p = MODULI[family][name]
    rng = random.Random("layout:%s:%s:%s" % (family, name, op))
    waves = []

    def wave(slots):
        w = [_ordinary(family, p, op, rng) for _ in range(64)]
        for lane, v in slots.items():
            w[lane] = v
        waves.append(w)
    rare = []
    if op in RARE:
        found = class_vectors(family, name, op)
        rare = [v for c in RARE[op] for v in found.get(c, [])[:2]]
        for i, v in enumerate(rare):
            for lane in (0, 31, 32, 63):
                wave({lane: v})
        for i, lanes in enumerate(((5, 40), (0, 63), (31, 32))):
            wave({lanes[0]: rare[i % len(rare)], lanes[1]: rare[(i + 1) % len(rare)]})
        for c in RARE[op]:
            if found.get(c):
                wave({lane: found[c][lane % len(found[c])] for lane in range(64)})
        wave({lane: rare[lane % len(rare)] for lane in range(64)})                  # every lane rare, classes mixed
        wave({lane: rare[lane % len(rare)] for lane in range(0, 64, 3)})            # mixed with ordinary lanes
        wave({lane: rare[(lane * 7) % len(rare)] for lane in range(32, 64)})        # the upper half only
    elif op in ("pow", "pow_limbs"):
        top = 64 if op == "pow" else 256
        step = top // 64

        def exponent(bits):
            return 0 if bits == 0 else rng.getrandbits(bits - 1) | (1 << (bits - 1))
        for lengths in ([step * lane for lane in range(64)], [top - step * lane for lane in range(64)],
                        [(lane * 37) % 65 for lane in range(64)], [0, 1, top, 2] * 16):
            wave({lane: (rng.randrange(p), exponent(bits)) for lane, bits in enumerate(lengths)})
    else:
        wave({})
        wave({})
    tail = [_ordinary(family, p, op, rng) for _ in range(13)]
    for i, lane in enumerate((0, 7, 12)):
        if rare:
            tail[lane] = rare[i % len(rare)]
        elif op in ("pow", "pow_limbs"):
            tail[lane] = (rng.randrange(p), i)
    return [v for w in waves for v in w] + tail


# ---- records and expected bytes ------------------------------------------------------------------------------------------------
def encode(family, name, op, cases):
    """the input file: the modulus record, then the operand records"""
    widths = [_width(family, k) for k in OPS[family][op][0]]
    return MODULI[family][name].to_bytes(_unit(family), "little") + b"".join(
        v.to_bytes(w, "little") for ops in cases for v, w in zip(ops, widths))


def expected(family, name, op, cases):
    """the model's result records; every operand is checked to be within the op's contract"""
    p, R = MODULI[family][name], 1 << BITS[family]
    kinds, out_units, model = OPS[family][op]
    w = out_units * _unit(family)
    res = []
    for ops in cases:
        for v, k in zip(ops, kinds):
            assert 0 <= v < (p if k == "canon" else 1 << 64 if k == "e64" else 1 << 256 if k in ("e256", "limbs") else R), (op, k, ops)
        res.append(model(p, R, *ops).to_bytes(w, "little"))
    return b"".join(res)


@functools.lru_cache(maxsize=8)
def operands(family, name, op, part):
    """part "main": the edges crossed, the class vectors, then random operands; part "layout": `layouts`"""
    if part == "layout":
        return layouts(family, name, op)
    found = class_vectors(family, name, op) if op in CLASSIFY else {}
    return edge_cases(family, name, op) + [v for c in sorted(found) for v in found[c]] + random_cases(family, name, op)


@functools.lru_cache(maxsize=8)
def case_set(family, name, op, part):
    """-> (operand tuples, input bytes, expected bytes)"""
    cases = operands(family, name, op, part)
    return cases, encode(family, name, op, cases), expected(family, name, op, cases)


# ---- the harness ---------------------------------------------------------------------------------------------------------------
def build_harness(exe, defines=(), csrc=None):
    """hipcc for gfx950 with the library's flags plus `defines`"""
    return native_harness.build(HARNESS, exe, defines, csrc)


def job(family, name, op, part, grid, block, tag):
    """a job of `run_jobs`: the harness's op is family_op, the input file is per (op, modulus, part)"""
    return ("%s_%s" % (family, op), "%s.%s" % (name, part), grid, block, tag)


def _inputs(jop, jpart):
    family, op = jop.split("_", 1)
    name, part = jpart.rsplit(".", 1)
    cases = operands(family, name, op, part)
    return len(cases), encode(family, name, op, cases)


def run_jobs(exe, mode, jobs, workdir, timeout=600):
    """jobs: `job` tuples -> {tag: result bytes}.  One process runs every job."""
    return native_harness.run_jobs(exe, mode, jobs, workdir, _inputs, timeout)


def mismatches(family, name, op, part, got, block=64, limit=5):
    """the first few elements whose result differs from the model, as readable text (lane: within a wave of `block`-thread blocks)"""
    cases, _, want = case_set(family, name, op, part)
    w = OPS[family][op][1] * _unit(family)
    bad = []
    if len(got) != len(want):
        bad.append("%d result bytes, expected %d" % (len(got), len(want)))
    for i in range(len(cases)):
        g, e = got[i * w:(i + 1) * w], want[i * w:(i + 1) * w]
        if g != e:
            note = " classes %s" % sorted(classes_of(family, name, op, cases[i])) if op in CLASSIFY else ""
            bad.append("element %d (lane %d): operands %s%s: got %s want %s" % (
                i, i % block % 64, [hex(v) for v in cases[i]], note, hex(int.from_bytes(g, "little")), hex(int.from_bytes(e, "little"))))
            if len(bad) >= limit:
                break
    return "%s %s (p = %s) %s/%s: %s" % (family, name, hex(MODULI[family][name]), op, part, "; ".join(bad))
