"""The case grid of the packed-word FRI commit's tests (test_mod64fri_host.py, test_gpu_mod64fri.py), built from modfri_cases.Case and
ntt64_cases: every modulus below 2^64 of modfri_cases.MODULI with modfri_cases' own shapes -- the same case ids, so modfri_cases'
cached oracle proofs are reused --, and three moduli of ntt64_cases beside them: KoalaBear, BIG18 = 2^64 - 1835007 (a prime above 2^63:
sums, and the x + p of the fold's halving, carry out of 64 bits) and 2^64 - 59 (2-adicity 2: the zero-round commit at n = 4 only).

A case's coefficients are 8-byte words.  For a modfri_cases shape they are that case's 256-bit coefficients modulo p: the oracle reduces
its input, so the proof is the same.  For the new moduli they are ntt64_cases.inputs: every fifth one at or above p where 2^64 - p
leaves room.  The oracle is oracle/pyoracle.py with p = the modulus, exact."""
import functools

import modfri_cases as fc
import ntt64_cases as nc
from oracle import pyoracle

BIG18 = nc.BIG18
MODULI = {k: v for k, v in fc.MODULI.items() if v < 2**64}
MODULI.update(koalabear=nc.KOALABEAR, big18=nc.BIG18, p64_59=nc.P64_59)
NEW = ("koalabear", "big18", "p64_59")


def root_of(name, n):
    return nc.root_of(name, n) if name in NEW else fc.root_of(name, n)


class Case(fc.Case):
    """a modfri_cases.Case over a modulus below 2^64, its coefficients as words"""

    def __init__(self, name, n, md, n_coeffs, exclude=0, samples=40, batch=1, const=None, verify=True):
        if name not in NEW:
            fc.Case.__init__(self, name, n, md, n_coeffs, exclude, samples, batch, const, verify)
            return
        self.name, self.n, self.md, self.n_coeffs = name, n, md, n_coeffs  # modfri_cases knows neither the modulus nor its roots
        self.exclude, self.samples, self.batch, self.const, self.verify = exclude, samples, batch, const, verify
        self.p, self.root = MODULI[name], nc.root_of(name, n)
        self.id = "%s-n%d-md%d-c%d-x%d-s%d-b%d%s" % (name, n, md, n_coeffs, exclude, samples, batch, "-const" if const is not None else "")

    def coeffs(self):
        if self.const is not None:
            return [self.const] * (self.batch * self.n_coeffs)
        if self.name in NEW:
            return nc.inputs(self.n * 31 + self.md + self.batch, self.batch * self.n_coeffs, self.p)
        return [v % self.p for v in fc.Case.coeffs(self)]

    def words(self):
        return nc.words(self.coeffs())

    def wire(self):
        """the same values as 32-byte wire, what sh_mod_fri_prove takes"""
        return fc.mc.wire(self.coeffs())


def _grid():
    out = []
    for c in fc.GRID:  # modfri_cases' own shapes for every modulus below 2^64
        if c.name in MODULI:
            out.append(Case(c.name, c.n, c.md, c.n_coeffs, c.exclude, c.samples, c.batch, c.const, c.verify))
    out += [Case("koalabear", 16, 16, 3), Case("koalabear", 64, 32, 32), Case("koalabear", 256, 128, 128)]
    out += [Case("big18", 16, 16, 16), Case("big18", 64, 32, 32), Case("big18", 256, 128, 128), Case("big18", 4096, 1024, 1000)]
    out.append(Case("big18", 64, 32, 30, batch=3))
    # the reference's verifier asks every round for the count it is given, its prover gives later rounds 40 (modfri_cases._grid): a
    # two-round proof with 80 samples cannot be verified, the one-round case can
    out += [Case("big18", 256, 128, 100, samples=7), Case("big18", 256, 64, 64, samples=80)]
    out.append(Case("big18", 1024, 256, 256, exclude=8))
    # the constant polynomial p - 1: every leaf, column value and final value is p - 1, its top bit set
    out += [Case("big18", 64, 32, 1, const=BIG18 - 1), Case("big18", 16, 16, 1, const=BIG18 - 1)]
    out.append(Case("p64_59", 4, 1, 1))
    return out


GRID = _grid()
# both tree forms in one commit: n * batch is above MERKLE_SERIAL_MAX_LEAVES = 2^15, the later rounds are below it (GPU half only)
BOTH_TREE_FORMS = Case("big18", 1 << 14, 1 << 11, 1 << 11, batch=3)
HOST_GRID = [c for c in GRID if c.n <= 4096]
_BY_ID = {c.id: c for c in GRID + [BOTH_TREE_FORMS]}


@functools.lru_cache(maxsize=None)
def _oracle(case_id):
    c = _BY_ID[case_id]
    co = c.coeffs()
    return [pyoracle.prove_low_degree(co[b * c.n_coeffs:(b + 1) * c.n_coeffs], c.root, c.md, p=c.p, exclude_multiples_of=c.exclude,
                                      fri_spot_check_security_factor=c.samples) for b in range(c.batch)]


def oracle_proofs(c):
    """the nested proofs of the batch, computed once per process; a modfri_cases shape shares modfri_cases' cache"""
    return fc.oracle_proofs(c) if c.name not in NEW else _oracle(c.id)


def oracle_flat(c):
    return b"".join(pyoracle.proof_flat(p) for p in oracle_proofs(c))


def merkle_root(c, b=0):
    """the commitment the proof of polynomial b speaks about: the root of the tree over its evaluations"""
    co = c.coeffs()[b * c.n_coeffs:(b + 1) * c.n_coeffs]
    return pyoracle.merkelize(fc.mc.transform(co, c.n, c.p, c.root))[1]


def oracle_verify(c, proof, b=0):
    return pyoracle.verify_low_degree_proof(proof, merkle_root(c, b), c.root, c.md, p=c.p, exclude_multiples_of=c.exclude,
                                            fri_spot_check_security_factor=c.samples)
