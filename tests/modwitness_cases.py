"""The case grid of the generic-modulus witness generator's tests (test_modwitness_host.py, test_gpu_modwitness.py): the moduli, the
systems and the exact oracle (oracle/pyoracle.py: get_computational_trace with p = the modulus), computed once per case and process.

A trace needs only ring operations, so the moduli include what the generic prover refuses (BabyBear: 7 is a quadratic residue),
composites (15, and 2^256 - 1 = the largest odd 256-bit value, every limb all-ones) and 3, the smallest modulus.  P43 lies above the
MiMC prime: a reduction modulo the MiMC prime anywhere would show there.

Values are kept AS STORED: an input or coefficient may be x + p (or, for the inputs of small moduli, 2^256 - 1) where that fits in
256 bits; the oracle reduces them as field(v) does."""
import functools
import hashlib
import json
import os

import modntt_cases as mc
import modstark_cases as sc
from oracle import pyoracle

MIMC_P = mc.MIMC_P
P43 = sc.P43
ALL_ONES = 2**256 - 1
MODULI = {"bn254": mc.BN254, "bls12_381": mc.BLS12_381, "goldilocks": mc.GOLDILOCKS, "babybear": mc.BABYBEAR, "mimc": MIMC_P, "p43": P43,
          "f257": 257, "f17": 17, "f3": 3, "allones": ALL_ONES, "f15": 15}
TOP = 2**256

LINEAR_1, MIMC_2, CUBIC_1, MIXED_3, QUINTIC_9, ZERO_2 = sc.LINEAR_1, sc.MIMC_2, sc.CUBIC_1, sc.MIXED_3, sc.QUINTIC_9, sc.ZERO_2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _w9_256_terms():
    """the 256-term width-9 system of tests/golden/stark_variants.json, as {exponent tuple: coefficient} per dimension"""
    with open(os.path.join(GOLDEN, "stark_variants.json")) as fh:
        c = [x for x in json.load(fh)["cases"] if x["name"] == "w9_256_terms"][0]
    import stark_variants as sv
    return sv.step_polys(c), [sv.unit_inputs(c, u) for u in range(3)]


W9_256, W9_INPUTS = _w9_256_terms()
# 256 terms, every exponent 255, coefficient 2: one step is about 34600 products on one lane, more than a dispatch's budget
HEAVY = [{tuple((t * 7 + v) % 256 if v == t % 9 else 255 for v in range(9)): 2 for t in range(c, 256, 9)} for c in range(9)]


def edge_systems(p):
    """(name, step polynomials, inputs of two units) -- the edge systems of test_witness_host.py with coefficients taken mod p"""
    return [
        ("exponent_255", [{(255, 0): 1}, {(3, 255): 2 % p, (0, 0): 1}], [[3, 5], [p - 2, 1]]),
        ("coefficients_0_and_p_minus_1", [{(1, 0): p - 1, (0, 1): 0}, {(1, 1): p - 1, (0, 0): 3 % p}], [[5, 7], [p - 1, 2]]),
        ("constant_terms_only", [{(0, 0, 0): 9 % p}, {(0, 0, 0): 1}, {(0, 0, 0): 0}], [[1, 2, 3], [0, 0, 0]]),
        ("fib_from_zero", [{(0, 1): 1}, {(0, 1): 1, (1, 0): 1}], [[0, 1], [0, 0]]),
        ("width_9_dense", [{tuple(int(v == c or v == (c + 1) % 9) * (1 + (c % 3)) for v in range(9)): (c + 1) % p, (0,) * 9: c % p}
                           for c in range(9)], [list(range(1, 10)), [0] * 9]),
    ]


class Case(object):
    """`len(inputs)` units of one system over MODULI[name]; inputs and coefficients as stored (any value below 2^256)"""

    def __init__(self, name, system, sp, steps, inputs):
        self.name, self.system, self.sp, self.steps, self.inputs = name, system, sp, steps, inputs
        self.p, self.width, self.batch = MODULI[name], len(sp), len(inputs)
        self.id = "%s-%s-s%d" % (name, system, steps)
        assert all(0 <= v < TOP for u in inputs for v in u) and all(0 <= c < TOP for d in sp for c in d.values())

    def terms(self):
        """-> (coefs wire bytes, exps bytes, counts list): sorted monomial order, starks_amd.stark.pack_step_polys' layout, the
        coefficients as stored"""
        coefs, exps, counts = [], bytearray(), []
        for poly in self.sp:
            items = sorted(poly.items())
            counts.append(len(items))
            for k, c in items:
                coefs.append(c)
                exps += bytes(k)
        return mc.wire(coefs), bytes(exps), counts

    def input_wire(self):
        return mc.wire([v for u in self.inputs for v in u])

    def input_limbs(self):
        return b"".join(int(v).to_bytes(32, "little") for u in self.inputs for v in u)


def _plus_p(vals, p):
    """x + p where that fits in 256 bits"""
    return [v + p if v + p < TOP else v for v in vals]


def _grid():
    out = []
    for name in sorted(MODULI):
        p = MODULI[name]
        rnd = __import__("random").Random(name)
        for tag, sp, steps in (("linear1", LINEAR_1, 7), ("mimc2", MIMC_2, 65), ("mixed3", MIXED_3, 33), ("quintic9", QUINTIC_9, 9),
                               ("zero2", ZERO_2, 5)):
            ins = [[rnd.randrange(p) for _ in sp] for _ in range(2)]
            out.append(Case(name, tag, sp, steps, ins))
        for tag, sp, ins in edge_systems(p):
            for steps in (1, 3, 1000):
                out.append(Case(name, tag, sp, steps, ins))
        # a coefficient stored as 1 + p (it must count as 1, in the plan and in the kernel's staging) and inputs stored as x + p
        unit = [{(1, 0): (1 + p) if 1 + p < TOP else 1}, {(1, 0): (1 + p) if 1 + p < TOP else 1, (0, 3): 1, (0, 0): (2 % p + p) if 2 % p + p < TOP else 2 % p}]
        raw = [_plus_p([42 % p, 3 % p], p), _plus_p([p - 1, 0], p)]
        if p < 2**64:
            raw.append([ALL_ONES, ALL_ONES - 1])  # any 256-bit value is an input
        out.append(Case(name, "stored_plus_p", unit, 100, raw))
    for name in ("bn254", "goldilocks"):
        out.append(Case(name, "w9_256_terms", W9_256, 70, [[v % MODULI[name] for v in u] for u in W9_INPUTS]))
    return out


GRID = _grid()
HEAVY_CASE = Case("bn254", "heavy", HEAVY, 3, [list(range(2, 11))])
_BY_ID = {c.id: c for c in GRID + [HEAVY_CASE]}
assert len(_BY_ID) == len(GRID) + 1


@functools.lru_cache(maxsize=None)
def _want(case_id):
    c = _BY_ID[case_id]
    return b"".join(mc.wire([v for col in pyoracle.get_computational_trace(u, c.steps, c.sp, c.p) for v in col]) for u in c.inputs)


def want_wire(c):
    """the exact witness [batch][width][steps] in canonical wire form, computed once per process"""
    return _want(c.id)


def want_limbs(c):
    w = want_wire(c)
    return b"".join(w[i:i + 32][::-1] for i in range(0, len(w), 32))


def trace_wire(p, inputs, steps, sp):
    return mc.wire([v for col in pyoracle.get_computational_trace(inputs, steps, sp, p) for v in col])


def sha(b):
    return hashlib.sha256(b).hexdigest()


# the four cases of tests/golden/mod_witness.json (generate_mod_witness.py): (modulus name, step polynomials, steps, inputs)
FIXTURE = {
    "bn254-mimc2": ("bn254", MIMC_2, 64, [2, 5]),
    "goldilocks-mixed3": ("goldilocks", MIXED_3, 64, [3, 4, 5]),
    "babybear-cubic1": ("babybear", CUBIC_1, 64, [3]),
    "p43-const": ("p43", sc.CUBE_1, 16, [P43 - 1]),
}
