"""Proofs for the tests of the FRI verifiers over any odd modulus (test_modverify_host.py, test_gpu_modverify.py): the honest grid of
tests/modfri_cases.py, and proofs built so that exactly one check of the verifier can reject them.  The exact oracle is
oracle/pyoracle.verify_low_degree_proof(..., p=...): an AssertionError means rejected."""
import functools

import modfri_cases as fc
import modntt_cases as mc
from modfri_cases import MODULI, root_of
from oracle import pyoracle as po

OK, INVALID, ROOT_ORDER, UNSUPPORTED, REJECTED = 0, -1, -2, -6, -9


def b32(x):
    return int(x).to_bytes(32, "big")


def unpack(flat, n, md, samples=40, later=40):
    """the flat layout -> the reference's nested proof; `later` = the sample count of the rounds after the first (the prover's 40)"""
    out, off, first = [], 0, True
    while md > 16:
        lg = n.bit_length() - 1
        s = samples if first else later
        root2, off = flat[off:off + 32], off + 32
        branches = []
        for _ in range(s):
            bset = []
            for ln in (lg - 1, lg + 1, lg + 1, lg + 1, lg + 1):
                bset.append([flat[off + 32 * k:off + 32 * k + 32] for k in range(ln)])
                off += 32 * ln
            branches.append(bset)
        out.append([root2, branches])
        n, md, first = n // 4, md // 4, False
    out.append([flat[off + 32 * k:off + 32 * k + 32] for k in range(n)])
    assert off + 32 * n == len(flat)
    return out


def oracle_status(p, flat, merkle_root, n, w, md, exclude=0, samples=40):
    """the oracle's decision on a flat proof as a status: OK or REJECTED"""
    try:
        po.verify_low_degree_proof(unpack(flat, n, md, samples), merkle_root, w, md, p=p, exclude_multiples_of=exclude,
                                   fri_spot_check_security_factor=samples)
        return OK
    except AssertionError:
        return REJECTED


class Proof(object):
    """one flat proof with the arguments a verifier takes"""

    def __init__(self, name, n, md, flat, merkle_root, exclude=0, samples=40, tag=""):
        self.name, self.p, self.n, self.md, self.flat, self.merkle_root = name, MODULI[name], n, md, flat, merkle_root
        self.exclude, self.samples, self.root = exclude, samples, root_of(name, n)
        self.id = "%s-%d/%d-x%d-s%d%s" % (name, n, md, exclude, samples, tag)

    def oracle(self):
        return oracle_status(self.p, self.flat, self.merkle_root, self.n, self.root, self.md, self.exclude, self.samples)

    def with_flat(self, flat, tag):
        return Proof(self.name, self.n, self.md, flat, self.merkle_root, self.exclude, self.samples, tag)


def honest(c):
    """the batch of a modfri_cases.Case as Proofs"""
    plen = len(fc.oracle_flat(c)) // c.batch
    flat = fc.oracle_flat(c)
    return [Proof(c.name, c.n, c.md, flat[b * plen:(b + 1) * plen], fc.merkle_root(c, b), c.exclude, c.samples, "-b%d" % b)
            for b in range(c.batch)]


@functools.lru_cache(maxsize=None)
def from_coeffs(name, n, md, coeffs, exclude=0, samples=40):
    """the reference prover's proof of the polynomial `coeffs` (a tuple), whatever its degree"""
    p, w = MODULI[name], root_of(name, n)
    co = list(coeffs)
    flat = po.proof_flat(po.prove_low_degree(co, w, md, p=p, exclude_multiples_of=exclude, fri_spot_check_security_factor=samples))
    root = po.merkelize(mc.transform(co, n, p, w))[1]
    return Proof(name, n, md, flat, root, exclude, samples, "-c%d" % len(co))


# (modulus, n, md, exclude): shapes at which a polynomial of md + 1 coefficients passes every branch and row and fails the final layer
DEGREE_SHAPES = [("bn254", 64, 32, 0), ("c2", 64, 32, 0), ("f257", 64, 32, 0), ("goldilocks", 256, 128, 0), ("f65537", 1024, 256, 8),
                 ("p43", 1024, 256, 8), ("bn254", 16, 8, 0), ("f257", 16, 8, 0), ("c2", 16, 8, 4)]


def degree_pair(name, n, md, exclude):
    """(md coefficients: accepted, md + 1 coefficients with the top one 1: only the final layer's degree bound rejects)"""
    p = MODULI[name]
    lo = tuple((7 * i + 3) % p for i in range(md))
    hi = tuple((7 * i + 3) % p for i in range(md)) + (1,)
    return from_coeffs(name, n, md, lo, exclude), from_coeffs(name, n, md, hi, exclude)


FOLD_SHAPES = [("bn254", 64, 32, 0), ("c2", 256, 128, 0), ("f257", 256, 128, 0), ("babybear", 1024, 256, 8)]


@functools.lru_cache(maxsize=None)
def wrong_fold(name, n, md, exclude, nudge):
    """A proof whose first column is the fold at special_x + nudge instead of at special_x = field(the committed root), with everything
    after it honest for that column: every Merkle branch verifies and the later rounds and the final layer are a valid proof of the
    column, so only the first round's row checks can reject it.  nudge = 0 is the honest proof, nudge = p folds at the same residue."""
    p, w = MODULI[name], root_of(name, n)
    coeffs = [(5 * i + 1) % p for i in range(md)]
    values = po.fft_1d(coeffs, p, w)
    xs = po.get_power_cycle(w, p)
    m = po.merkelize(values)
    column = po.fri_fold(values, xs, (int.from_bytes(m[1], "big") + nudge) % p, p)
    m2 = po.merkelize(column)
    q = n // 4
    out = [m2[1]]
    for y in po.get_pseudorandom_indices(m2[1], q, 40, exclude_multiples_of=exclude):
        out += po.mk_branch(m2, y)
        for j in range(4):
            out += po.mk_branch(m, y + q * j)
    w4 = pow(w, 4, p)
    rest = po.prove_low_degree(po.inv_fft_poly(column, p, w4), w4, md // 4, p=p, exclude_multiples_of=exclude)
    return Proof(name, n, md, b"".join(out) + po.proof_flat(rest), m[1], exclude, 40, "-nudge%d" % (nudge if nudge < p else -1))


def unreduced(delta=0):
    """A zero-round Goldilocks proof (n = 16, md = 8) of 3 + x + 4 x^2 whose 16 values are stored as v + p; value 11 is off by `delta`.
    The committed root is the tree over the bytes as stored."""
    p, w = MODULI["goldilocks"], root_of("goldilocks", 16)
    stored = [v + p for v in po.fft_1d([3, 1, 4], p, w)]
    stored[11] += delta
    return Proof("goldilocks", 16, 8, b"".join(b32(v) for v in stored), po.merkelize(stored)[1], tag="-unreduced%d" % delta)
