"""The case grid of the packed-word STARK prover's tests (test_mod64stark_host.py, test_gpu_mod64stark.py): modstark_cases' shapes, step
polynomials and Case machinery over the moduli below 2^64, with ntt64_cases' words helpers, and the exact oracle (oracle/pyoracle.py:
get_computational_trace, mk_stark_proof, verify_stark_proof, stark_flat with p = the modulus), computed once per case and process.

G2 is the reference's 7^((p - 1) // (steps * ext)) (stark.py:205): the grid holds the moduli over which it has order steps * ext.
BIG18 = 2^64 - 1835007 lies above 2^63: its sums carry out of 64 bits, and the constant trace p - 1 over it (X' = X^3 from p - 1) makes
every opened P value a word with its top bit set."""
import functools
import random
import struct

import modntt_cases as mc
import modstark_cases as sc
import ntt64_cases as nc
from modstark_cases import SHAPES, LINEAR_1, MIMC_2, CUBIC_1, MIXED_3, QUINTIC_9, ZERO_2, CUBE_1  # noqa: F401 (re-exported)
from oracle import pyoracle

GOLDILOCKS, BIG18 = nc.GOLDILOCKS, nc.BIG18
MODULI = {"goldilocks": GOLDILOCKS, "big18": BIG18, "f65537": 65537, "f257": 257, "f17": 17}
# refused with SH_ERR_ROOT_ORDER: 7 is a quadratic residue (BabyBear, KoalaBear, 3), or p - 1 has too few factors of two
BABYBEAR, KOALABEAR, P64_59 = nc.BABYBEAR, nc.KOALABEAR, nc.P64_59


class Case(sc.Case):
    """sc.Case over MODULI above, with the values as native 8-byte words beside the wire forms; in a plus_p case every fifth witness
    and input word is stored as v + p where that fits 64 bits, every fifth coefficient (a 32-byte wire value) as v + p"""

    def __init__(self, name, shape, steps, ext, sp, batch=1, samples=80, plus_p=False, inputs=None, tag=""):
        self.name, self.shape, self.steps, self.ext, self.sp = name, shape, steps, ext, sp
        self.batch, self.samples, self.plus_p = batch, samples, plus_p
        self.p, self.width, self.n, self.degree = MODULI[name], len(sp), steps * ext, sc.degree_of(sp)
        self.id = "%s-%s-b%d-s%d%s%s" % (name, shape, batch, samples, "-plusp" if plus_p else "", tag)
        rnd = random.Random(self.id)
        self.inputs = inputs if inputs is not None else [[rnd.randrange(self.p) for _ in range(self.width)] for _ in range(batch)]

    def _stored_words(self, vals):
        if not self.plus_p:
            return list(vals)
        return [v + self.p if i % 5 == 2 and v + self.p < 2**64 else v for i, v in enumerate(vals)]

    def witness_words(self, witnesses=None):
        w = self.witnesses() if witnesses is None else witnesses
        return nc.words(self._stored_words([v for unit in w for col in unit for v in col]))

    def input_words(self):
        return nc.words(self._stored_words([v for inp in self.inputs for v in inp]))

    def witness_wire(self, witnesses=None):
        """the same stored values as 32-byte wire values: what the generic prover takes"""
        return mc.wire(nc.ints(self.witness_words(witnesses)))

    def input_wire(self):
        return mc.wire(nc.ints(self.input_words()))

    def blob(self, witnesses=None):
        """what tests/native/mod64stark_host.cpp reads for the case"""
        counts, coefs, exps = self.terms()
        return self.witness_words(witnesses) + self.input_words() + struct.pack("<%dI" % self.width, *counts) + mc.wire(coefs) + exps


def _grid():
    out = []
    for name in sorted(MODULI):
        for shape, (steps, ext, sp) in SHAPES.items():
            if name == "f17" and shape != "s2":
                continue  # 17 - 1 = 16 points is all its group has
            out.append(Case(name, shape, steps, ext, sp))
    out.append(Case("goldilocks", "s32", 32, 8, MIXED_3, batch=3, samples=7))
    out.append(Case("big18", "s8", 8, 8, MIMC_2, batch=3))
    out.append(Case("f65537", "s8zero", 8, 8, ZERO_2))
    out.append(Case("big18", "s8zero", 8, 8, ZERO_2, batch=3))
    # plus p: MIXED_3's first column X1' = X1 + 1 stays small from a small input, so v + p fits a word over the large moduli too
    for name in ("goldilocks", "big18", "f257"):
        out.append(Case(name, "s32", 32, 8, MIXED_3, plus_p=True, inputs=[[5, 3, 2]]))
    out.append(Case("f65537", "s8", 8, 8, MIMC_2, batch=3, plus_p=True))
    return out


GRID = _grid()
# the constant trace p - 1 over BIG18 (X' = X^3 from p - 1), steps 16, ext 8: every P value has its top bit set
BIG18_CONST = Case("big18", "s16const", 16, 8, CUBE_1, inputs=[[BIG18 - 1]])
# every single-element break of one small witness: proof 0 is the valid trace, proof 1 + (c * steps + k) has witness[c][k] + 1
BREAK_BASE = Case("goldilocks", "s8", 8, 8, MIMC_2, inputs=[[2, 5]], tag="-break")
HOST_GRID = [c for c in GRID if c.n <= 4096]

_BY_ID = {c.id: c for c in GRID + [BIG18_CONST, BREAK_BASE]}
assert len(_BY_ID) == len(GRID) + 2


@functools.lru_cache(maxsize=None)
def _oracle(case_id):
    c = _BY_ID[case_id]
    return [pyoracle.mk_stark_proof(w, inp, c.sp, c.steps, c.ext, p=c.p, samples=c.samples) for w, inp in zip(c.witnesses(), c.inputs)]


def oracle_proofs(c):
    """the nested proofs of the batch, computed once per process"""
    return _oracle(c.id)


def oracle_flat(c):
    return b"".join(pyoracle.stark_flat(p) for p in oracle_proofs(c))


def proof_len(c):
    return len(oracle_flat(c)) // c.batch


oracle_verify = sc.oracle_verify
opened_p_values = sc.opened_p_values


def broken_witnesses():
    """sc.broken_witnesses' construction over BREAK_BASE: -> (witnesses [1 + width * steps][width][steps], expected flags); the flag is
    the exact predicate -- a transition k -> k + 1, k + 1 < steps, that does not hold (the wrap-around row is not a constraint)"""
    c = BREAK_BASE
    base = c.witnesses()[0]
    units = [base]
    for col in range(c.width):
        for k in range(c.steps):
            w = [list(x) for x in base]
            w[col][k] = (w[col][k] + 1) % c.p
            units.append(w)
    flags = []
    for w in units:
        bad = False
        for k in range(c.steps - 1):
            nxt = pyoracle.get_computational_trace([w[j][k] for j in range(c.width)], 2, c.sp, c.p)
            bad = bad or any(nxt[j][1] != w[j][k + 1] for j in range(c.width))
        flags.append(1 if bad else 0)
    return units, flags


def break_batch():
    """BREAK_BASE's shape with every broken witness as one batch -> (case, witnesses, expected flags)"""
    units, want = broken_witnesses()
    base = BREAK_BASE
    return (Case(base.name, base.shape, base.steps, base.ext, base.sp, batch=len(units), inputs=base.inputs * len(units), tag="-breakbatch"),
            units, want)
