"""The case grid of the generic-modulus STARK prover's tests (test_modstark_host.py, test_gpu_modstark.py): the moduli, the smallest
shapes that reach each part of the prover, and the exact oracle (oracle/pyoracle.py: get_computational_trace, mk_stark_proof,
verify_stark_proof, stark_flat with p = the modulus), computed once per case and process.

G2 is the reference's 7^((p - 1) // (steps * ext)) (stark.py:205): the grid holds the moduli over which it has order steps * ext.
P43 = 2^256 - 43 * 2^32 + 1 lies above the MiMC prime: the constant trace p - 1 over it (X' = X^3 from p - 1) makes every opened
P value p - 1 >= MIMC_P, the one input on which a canonicalisation modulo the MiMC prime shows."""
import functools
import hashlib
import random
import struct

import modntt_cases as mc
from oracle import pyoracle

MIMC_P = mc.MIMC_P
P43 = 2**256 - 43 * 2**32 + 1
MODULI = {"bn254": mc.BN254, "bls12_381": mc.BLS12_381, "goldilocks": mc.GOLDILOCKS, "mimc": MIMC_P, "p43": P43, "f257": 257,
          "f65537": 65537, "f17": 17}
BABYBEAR = mc.BABYBEAR  # 7 is a quadratic residue: G2 never has full order

# step polynomials as {exponent tuple: coefficient} per dimension (the oracle's form)
LINEAR_1 = [{(1,): 3, (0,): 1}]                                                          # X' = 3 X + 1
MIMC_2 = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]                                           # the reference's MiMC formulation (test_stark.py:236-293)
CUBIC_1 = [{(3,): 1, (0,): 7}]                                                           # X' = X^3 + 7
MIXED_3 = [{(1, 0, 0): 1, (0, 0, 0): 1}, {(1, 1, 0): 1}, {(1, 0, 0): 2, (0, 0, 3): 1}]   # X1' = X1 + 1, X2' = X1 X2, X3' = X3^3 + 2 X1
QUINTIC_9 = ([{tuple(1 if j == i else 0 for j in range(9)): 1, (0,) * 9: i + 1} for i in range(8)]  # X_i' = X_i + i + 1
             + [{(1, 1, 1, 1, 1, 0, 0, 0, 0): 1, (0, 0, 0, 0, 0, 0, 0, 0, 1): 5}])       # X9' = X1 X2 X3 X4 X5 + 5 X9
ZERO_2 = [{(0, 0): 0}, {(1, 0): 1, (0, 1): 1, (0, 0): 1}]                                # X1' = 0 (the zero polynomial), X2' = X1 + X2 + 1
CUBE_1 = [{(3,): 1}]                                                                     # X' = X^3

SHAPES = {
    "s2": (2, 8, LINEAR_1),       # zero FRI rounds
    "s8": (8, 8, MIMC_2),         # one round
    "s16x4": (16, 4, CUBIC_1),    # the smallest ext a cubic admits
    "s32": (32, 8, MIXED_3),      # two rounds; over 257 the domain is the whole group
    "s8w9": (8, 8, QUINTIC_9),    # the maximum width, a degree-5 term
}


def degree_of(sp):
    return max(pyoracle.mv_degree(d) for d in sp)


class Case(object):
    """`batch` proofs of one shape over MODULI[name]; proof b starts from inputs[b]"""

    def __init__(self, name, shape, steps, ext, sp, batch=1, samples=80, plus_p=False, inputs=None, tag=""):
        self.name, self.shape, self.steps, self.ext, self.sp = name, shape, steps, ext, sp
        self.batch, self.samples, self.plus_p = batch, samples, plus_p
        self.p, self.width, self.n, self.degree = MODULI[name], len(sp), steps * ext, degree_of(sp)
        self.id = "%s-%s-b%d-s%d%s%s" % (name, shape, batch, samples, "-plusp" if plus_p else "", tag)
        rnd = random.Random(self.id)
        self.inputs = inputs if inputs is not None else [[rnd.randrange(self.p) for _ in range(self.width)] for _ in range(batch)]

    def witnesses(self):
        """[batch][width][steps] residues"""
        return [pyoracle.get_computational_trace(inp, self.steps, self.sp, self.p) for inp in self.inputs]

    def _stored(self, vals):
        """every fifth value as v + p where that fits in 256 bits (plus_p cases)"""
        if not self.plus_p:
            return list(vals)
        return [v + self.p if i % 5 == 2 and v + self.p < 2**256 else v for i, v in enumerate(vals)]

    def witness_wire(self, witnesses=None):
        w = self.witnesses() if witnesses is None else witnesses
        return mc.wire(self._stored([v for unit in w for col in unit for v in col]))

    def input_wire(self):
        return mc.wire(self._stored([v for inp in self.inputs for v in inp]))

    def terms(self):
        """-> (counts, coefficient ints as stored, exponent bytes): sorted monomial order, starks_amd.stark.pack_step_polys' layout"""
        counts, coefs, exps = [], [], bytearray()
        for poly in self.sp:
            items = sorted(poly.items())
            counts.append(len(items))
            for k, c in items:
                coefs.append(c % self.p)
                exps += bytes(k)
        return counts, self._stored(coefs), bytes(exps)

    def terms_blob(self):
        counts, coefs, exps = self.terms()
        return struct.pack("<%dI" % self.width, *counts) + mc.wire(coefs) + exps


def _grid():
    out = []
    for name in sorted(MODULI):
        for shape, (steps, ext, sp) in SHAPES.items():
            if name == "f17" and shape != "s2":
                continue  # 17 - 1 = 16 points is all its group has
            out.append(Case(name, shape, steps, ext, sp))
    out.append(Case("bn254", "s8", 8, 8, MIMC_2, batch=3))
    out.append(Case("goldilocks", "s32", 32, 8, MIXED_3, batch=3, samples=7))
    out.append(Case("bn254", "s16x4", 16, 4, CUBIC_1, samples=7))
    out.append(Case("bls12_381", "s8zero", 8, 8, ZERO_2))
    out.append(Case("f65537", "s8zero", 8, 8, ZERO_2, batch=3))
    for name in ("bn254", "goldilocks", "f257"):
        out.append(Case(name, "s32", 32, 8, MIXED_3, plus_p=True))
    out.append(Case("bn254", "s8", 8, 8, MIMC_2, batch=3, plus_p=True))
    return out


GRID = _grid()
# the constant trace p - 1 over P43 (X' = X^3 from p - 1), steps 16, ext 8
P43_CONST = Case("p43", "s16const", 16, 8, CUBE_1, inputs=[[P43 - 1]])
# every single-element break of one small witness: proof 0 is the valid trace, proof 1 + (c * steps + k) has witness[c][k] + 1
BREAK_BASE = Case("bn254", "s8", 8, 8, MIMC_2, inputs=[[2, 5]], tag="-break")
HOST_GRID = [c for c in GRID if c.n <= 4096]

# the three cases of tests/golden/mod_stark.json (generate_mod_stark.py)
FIXTURE = {
    "bn254-s8-w2": Case("bn254", "s8", 8, 8, MIMC_2, inputs=[[2, 5]], tag="-fix"),
    "goldilocks-s16x4-w1": Case("goldilocks", "s16x4", 16, 4, CUBIC_1, inputs=[[3]], tag="-fix"),
    "p43-const": P43_CONST,
}

_BY_ID = {c.id: c for c in GRID + [P43_CONST, BREAK_BASE] + list(FIXTURE.values())}
assert len(_BY_ID) == len(GRID) + 2 + len(FIXTURE) - 1  # P43_CONST is both


@functools.lru_cache(maxsize=None)
def _oracle(case_id):
    c = _BY_ID[case_id]
    return [pyoracle.mk_stark_proof(w, inp, c.sp, c.steps, c.ext, p=c.p, samples=c.samples) for w, inp in zip(c.witnesses(), c.inputs)]


def oracle_proofs(c):
    """the nested proofs of the batch, computed once per process"""
    return _oracle(c.id)


def oracle_flat(c):
    return b"".join(pyoracle.stark_flat(p) for p in oracle_proofs(c))


def oracle_verify(c, proof, b=0):
    w = c.witnesses()[b]
    return pyoracle.verify_stark_proof(proof, [col[-1] for col in w], c.inputs[b], c.sp, c.steps, c.ext, p=c.p, samples=c.samples)


def proof_len(c):
    return len(oracle_flat(c)) // c.batch


def broken_witnesses():
    """-> (witnesses [1 + width * steps][width][steps], expected flags): every single-element break of BREAK_BASE's witness; the flag
    is the exact predicate -- a transition k -> k + 1, k + 1 < steps, that does not hold (the wrap-around row is not a constraint)"""
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


def opened_p_values(flat, c):
    """the P values (element 0 .. width - 1 of a packed leaf) of every leaf and sibling leaf the spot checks of proof 0 open"""
    lg, k = c.n.bit_length() - 1, 3 * c.width
    off, out = 64, []
    for _ in range(c.samples):
        for _ in range(2):
            for leaf in range(2):
                out += mc.ints(flat[off + 32 * k * leaf:off + 32 * k * leaf + 32 * c.width])
            off += 64 * k + 32 * (lg - 1)
        off += 32 * (lg + 1)
    return out


def recorded(c):
    """what tests/golden/mod_stark.json keeps of a case: the inputs' recipe and the flat proof's length, digest, roots and head"""
    flat = oracle_flat(c)
    return {"modulus": c.name, "p": c.p, "steps": c.steps, "ext": c.ext, "width": c.width, "inputs": c.inputs[0],
            "step_polys": [[[list(k), v] for k, v in sorted(d.items())] for d in c.sp],
            "len": len(flat), "sha256": hashlib.sha256(flat).hexdigest(), "m_root": flat[:32].hex(), "l_root": flat[32:64].hex(),
            "head": flat[:64].hex()}
