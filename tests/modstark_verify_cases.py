"""Proofs for the tests of the STARK verifiers over any prime modulus (test_modstark_verify_host.py, test_gpu_modstark_verify.py): the
oracle's proofs of tests/modstark_cases.py's grid, and proofs that exactly one check of the verifier can reject.  No forged Merkle tree is
needed for those: a proof of an honest trace is rejected by the transition check alone when the verifier is given another step-polynomial
coefficient of the same degree, and by the boundary check alone when it is given inputs or outputs off by one.
The expected status is always oracle/pyoracle.verify_stark_proof with p = the modulus the verifier is given: an AssertionError means
rejected."""
import functools
import struct

import modntt_cases as mc
import modstark_cases as sc
import modverify_cases as fvc
from modverify_cases import INVALID, OK, REJECTED, ROOT_ORDER, UNSUPPORTED, b32  # noqa: F401
from oracle import pyoracle as po
from verify_batch_layout import flips, stark_regions

SINGLE_CHECK_IDS = ["bn254-s8-b1-s80", "goldilocks-s16x4-b1-s80", "f257-s32-b1-s80", "bn254-s8w9-b1-s80"]


def unpack(flat, steps, ext, width, degree, samples):
    """the flat layout (include/starkhip.h) -> the reference's [m_root, l_root, branches, fri_proof]"""
    n = steps * ext
    lg, k = n.bit_length() - 1, 3 * width
    off, branches = 64, []
    for _ in range(samples):
        for _ in range(2):
            br = [flat[off:off + 32 * k], flat[off + 32 * k:off + 64 * k]]
            off += 64 * k
            br += [flat[off + 32 * i:off + 32 * i + 32] for i in range(lg - 1)]
            off += 32 * (lg - 1)
            branches.append(br)
        branches.append([flat[off + 32 * i:off + 32 * i + 32] for i in range(lg + 1)])
        off += 32 * (lg + 1)
    return [flat[0:32], flat[32:64], branches, fvc.unpack(flat[off:], n, steps * degree, 40)]


def _plus(v, p, on):
    return v + p if on and v + p < 2**256 else v


class Proof(object):
    """one flat proof with the arguments a verifier takes: the modulus it verifies over, the shape, the step polynomials (the oracle's
    dict form), the inputs and outputs as STORED (any 256-bit integers); store_plus_p stores the coefficients as v + p too"""

    def __init__(self, p, steps, ext, sp, samples, flat, inputs, outputs, tag, store_plus_p=False):
        self.p, self.steps, self.ext, self.sp, self.samples, self.flat = p, steps, ext, sp, samples, flat
        self.inputs, self.outputs, self.id, self.store_plus_p = list(inputs), list(outputs), tag, store_plus_p
        self.width, self.degree, self.n = len(sp), sc.degree_of(sp), steps * ext
        self._oracle = None

    def shape(self):
        return (self.p, self.steps, self.ext, self.width, self.samples, len(self.flat), self.terms_blob())

    def terms(self):
        """-> (counts, coefficient ints as stored, exponent bytes) in sorted monomial order"""
        counts, coefs, exps = [], [], bytearray()
        for poly in self.sp:
            items = sorted(poly.items())
            counts.append(len(items))
            for k, c in items:
                coefs.append(_plus(c % self.p, self.p, self.store_plus_p))
                exps += bytes(k)
        return counts, coefs, bytes(exps)

    def terms_blob(self):
        counts, coefs, exps = self.terms()
        return struct.pack("<%dI" % self.width, *counts) + mc.wire(coefs) + exps

    def oracle(self):
        """pyoracle.verify_stark_proof's decision as a status, computed once"""
        if self._oracle is None:
            try:
                po.verify_stark_proof(unpack(self.flat, self.steps, self.ext, self.width, self.degree, self.samples), self.outputs, self.inputs,
                                      self.sp, self.steps, self.ext, p=self.p, samples=self.samples)
                self._oracle = OK
            except AssertionError:
                self._oracle = REJECTED
        return self._oracle

    def derive(self, tag, **changes):
        kw = dict(p=self.p, steps=self.steps, ext=self.ext, sp=self.sp, samples=self.samples, flat=self.flat, inputs=self.inputs,
                  outputs=self.outputs, store_plus_p=self.store_plus_p)
        kw.update(changes)
        return Proof(tag=self.id + tag, **kw)


@functools.lru_cache(maxsize=None)
def _honest(case_id):
    c = sc._BY_ID[case_id]
    flat, plen = sc.oracle_flat(c), sc.proof_len(c)
    return tuple(Proof(c.p, c.steps, c.ext, c.sp, c.samples, flat[b * plen:(b + 1) * plen], c.inputs[b], [col[-1] for col in w],
                       "%s#%d" % (c.id, b))
                 for b, w in enumerate(c.witnesses()))


def honest(c):
    """the oracle's proofs of a modstark_cases.Case (residues as inputs and outputs, whatever the case's plus_p stores for the prover)"""
    return list(_honest(c.id))


def other_constant(sp):
    """the step polynomials with one coefficient off by one and every degree unchanged: the constant term of the first dimension that
    has one, else the first term of the last dimension (1 -> 2)"""
    out = [dict(d) for d in sp]
    for d in out:
        zero = (0,) * len(sp)
        if zero in d:
            d[zero] += 1
            return out
    key = sorted(out[-1])[0]
    out[-1][key] += 1
    return out


def wrong_constant(P):
    """only the transition check can reject"""
    return P.derive("-const", sp=other_constant(P.sp))


def wrong_input(P):
    """only the boundary check can reject"""
    return P.derive("-in", inputs=[(P.inputs[0] + 1) % P.p] + P.inputs[1:])


def wrong_output(P):
    return P.derive("-out", outputs=P.outputs[:-1] + [(P.outputs[-1] + 1) % P.p])


def single_check(c):
    """[honest, wrong constant, wrong input, wrong output] of proof 0 of the case"""
    P = honest(c)[0]
    return [P, wrong_constant(P), wrong_input(P), wrong_output(P)]


def region_flips(P, per_region=1):
    """one single-bit flip per region of the layout"""
    regions, end = stark_regions(P.steps, P.ext, P.width, P.degree, P.samples)
    assert end == len(P.flat)
    return [P.derive("-" + name, flat=flat) for name, flat in flips(P.flat, regions, per_region, P.n + P.width)]


def stored_plus_p(P):
    """inputs, outputs and coefficients stored as v + p (where that fits in 256 bits): the same residues"""
    return P.derive("-plusp", inputs=[_plus(v, P.p, True) for v in P.inputs], outputs=[_plus(v, P.p, True) for v in P.outputs],
                    store_plus_p=True)


def p43_const():
    """(the constant trace p - 1 over P43: every opened P value is at or above the MiMC prime; the same bytes verified with the MiMC
    prime as the modulus)"""
    P = honest(sc.P43_CONST)[0]
    return P, P.derive("-as-mimc", p=sc.MIMC_P)


@functools.lru_cache(maxsize=None)
def _not_row0(case_id):
    c = sc._BY_ID[case_id]
    w = c.witnesses()[0]
    inp = [(c.inputs[0][0] + 1) % c.p] + c.inputs[0][1:]
    flat = po.stark_flat(po.mk_stark_proof(w, inp, c.sp, c.steps, c.ext, p=c.p, samples=c.samples))
    return Proof(c.p, c.steps, c.ext, c.sp, c.samples, flat, inp, [col[-1] for col in w], c.id + "-notrow0")


def not_row0(c):
    """a valid trace proved with inputs that are not its row 0 (the prover asserts nothing there), verified with those inputs"""
    return _not_row0(c.id)
