"""The case grid of the packed-word witness generator's tests (test_mod64witness_host.py, test_gpu_mod64witness.py): modwitness_cases'
systems over the moduli below 2^64, with ntt64_cases' words helpers, and the exact oracle (oracle/pyoracle.py:
get_computational_trace with p = the modulus), computed once per case and process.

A trace needs only ring operations, so the moduli include what the packed prover refuses (BabyBear, KoalaBear and 3: 7 is a quadratic
residue) and the composites 15 and 2^64 - 1 (every bit of the word set).  BIG18 = 2^64 - 1835007 lies above 2^63: its sums carry out of
the word.

Values are kept AS STORED: an input word may be x + p where that fits 64 bits, 2^64 - 1 or 2^64 - 2; a coefficient (a 32-byte wire
value) may be 1 + p.  The oracle reduces them as field(v) does."""
import functools
import hashlib

import modntt_cases as mc
import modwitness_cases as wc
import ntt64_cases as nc
from oracle import pyoracle

GOLDILOCKS, BIG18, ALL_ONES = nc.GOLDILOCKS, nc.BIG18, nc.ALL_ONES
MODULI = {"goldilocks": GOLDILOCKS, "big18": BIG18, "babybear": nc.BABYBEAR, "koalabear": nc.KOALABEAR, "f65537": 65537, "f257": 257,
          "f17": 17, "f3": 3, "f15": 15, "allones": ALL_ONES}
TOP = 2**64

LINEAR_1, MIMC_2, CUBIC_1, MIXED_3, QUINTIC_9, ZERO_2 = wc.LINEAR_1, wc.MIMC_2, wc.CUBIC_1, wc.MIXED_3, wc.QUINTIC_9, wc.ZERO_2
CUBE_1 = wc.sc.CUBE_1
W9_256, W9_INPUTS, HEAVY, edge_systems = wc.W9_256, wc.W9_INPUTS, wc.HEAVY, wc.edge_systems
wire, words, ints = mc.wire, nc.words, nc.ints


class Case(object):
    """`len(inputs)` units of one system over MODULI[name]; inputs as stored (any 64-bit word), coefficients as stored (any value below
    2^256)"""

    def __init__(self, name, system, sp, steps, inputs):
        self.name, self.system, self.sp, self.steps, self.inputs = name, system, sp, steps, inputs
        self.p, self.width, self.batch = MODULI[name], len(sp), len(inputs)
        self.id = "%s-%s-s%d" % (name, system, steps)
        assert all(0 <= v < TOP for u in inputs for v in u) and all(0 <= c < 2**256 for d in sp for c in d.values())

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
        return wire(coefs), bytes(exps), counts

    def input_words(self):
        return words([v for u in self.inputs for v in u])

    def input_limbs(self):
        """the same stored values zero-extended to sh_dev_mod_ntt's limb layout: what the generic generator takes"""
        return nc.limbs([v for u in self.inputs for v in u])


def _plus_p(vals, p):
    """x + p where that fits a word"""
    return [v + p if v + p < TOP else v for v in vals]


def _grid():
    out = []
    for name in sorted(MODULI):
        p = MODULI[name]
        rnd = __import__("random").Random("m6w-" + name)
        for tag, sp, steps in (("linear1", LINEAR_1, 7), ("mimc2", MIMC_2, 65), ("mixed3", MIXED_3, 33), ("quintic9", QUINTIC_9, 9),
                               ("zero2", ZERO_2, 5)):
            ins = [[rnd.randrange(p) for _ in sp] for _ in range(2)]
            out.append(Case(name, tag, sp, steps, ins))
        for tag, sp, ins in edge_systems(p):
            for steps in (1, 3, 1000):
                out.append(Case(name, tag, sp, steps, ins))
        # a coefficient stored as 1 + p (it must count as 1, in the plan and in the kernel's staging), inputs stored as x + p where that
        # fits a word, and 2^64 - 1 and 2^64 - 2 for every modulus: any 64-bit word is an input
        unit = [{(1, 0): 1 + p}, {(1, 0): 1 + p, (0, 3): 1, (0, 0): 2 % p + p}]
        raw = [_plus_p([42 % p, 3 % p], p), _plus_p([p - 1, 0], p), [TOP - 1, TOP - 2]]
        out.append(Case(name, "stored_plus_p", unit, 100, raw))
    for name in ("goldilocks", "allones"):
        out.append(Case(name, "w9_256_terms", W9_256, 70, [[v % MODULI[name] for v in u] for u in W9_INPUTS]))
    return out


GRID = _grid()
HEAVY_CASE = Case("big18", "heavy", HEAVY, 3, [list(range(2, 11))])
_BY_ID = {c.id: c for c in GRID + [HEAVY_CASE]}
assert len(_BY_ID) == len(GRID) + 1


def trace_words(p, inputs, steps, sp):
    """one unit's exact witness [width][steps] as native words"""
    return words([v for col in pyoracle.get_computational_trace(inputs, steps, sp, p) for v in col])


@functools.lru_cache(maxsize=None)
def _want(case_id):
    c = _BY_ID[case_id]
    return b"".join(trace_words(c.p, u, c.steps, c.sp) for u in c.inputs)


def want_words(c):
    """the exact witness [batch][width][steps] as canonical native words, computed once per process"""
    return _want(c.id)


def sha(b):
    return hashlib.sha256(b).hexdigest()


# the four cases of tests/golden/mod64_witness.json (generate_mod64_witness.py): (modulus name, step polynomials, steps, inputs)
FIXTURE = {
    "goldilocks-mixed3": ("goldilocks", MIXED_3, 64, [3, 4, 5]),
    "babybear-cubic1": ("babybear", CUBIC_1, 64, [3]),
    "big18-mimc2": ("big18", MIMC_2, 64, [2, 5]),
    "allones-const": ("allones", CUBE_1, 16, [ALL_ONES - 1]),
}
