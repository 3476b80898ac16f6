"""The case grid of the generic-modulus FRI commit's tests (test_modfri_host.py, test_gpu_modfri.py): the moduli of modntt_cases.py and
two more, the shapes at which each part of the commit can go wrong, and the exact oracle (oracle/pyoracle.py, parameterised by p).

P43 = 2^256 - 43 * 2^32 + 1 is prime and lies ABOVE the MiMC prime (2-adicity 32, 7 is a non-residue): the constant polynomial p - 1
over it makes every leaf, column value and final value p - 1 >= MIMC_P, the one input on which a canonicalisation modulo the MiMC
prime shows (random values land in [MIMC_P, p) with probability about 2^-216).  C2 = 257 * 65537 is composite; its roots come by CRT
from 3 in both factors."""
import functools

import modntt_cases as mc
from oracle import pyoracle

P43 = 2**256 - 43 * 2**32 + 1
C2 = 257 * 65537
C2_ROOTS = {64: 11083977, 256: 16122384}

MODULI = dict(mc.MODULI, p43=P43, c2=C2)
MIMC_P = mc.MIMC_P


def root_of(name, n):
    """a root w of order exactly n in Z/MODULI[name] with w^(n/2) = -1"""
    if name == "p43":
        return pow(pow(7, (P43 - 1) >> 32, P43), (1 << 32) // n, P43)
    if name == "c2":
        return C2_ROOTS[n] if n in C2_ROOTS else pow(C2_ROOTS[256], 256 // n, C2)
    return mc.root_of(name, n)


def max_log(name):
    return {"p43": 32, "c2": 8}.get(name) or mc.max_log(name)


class Case(object):
    """one commit: `batch` polynomials of n_coeffs coefficients over MODULI[name], on the n-point domain"""

    def __init__(self, name, n, md, n_coeffs, exclude=0, samples=40, batch=1, const=None, verify=True):
        self.name, self.n, self.md, self.n_coeffs = name, n, md, n_coeffs
        self.exclude, self.samples, self.batch, self.const, self.verify = exclude, samples, batch, const, verify
        self.p, self.root = MODULI[name], root_of(name, n)
        self.id = "%s-n%d-md%d-c%d-x%d-s%d-b%d%s" % (name, n, md, n_coeffs, exclude, samples, batch, "-const" if const is not None else "")

    def coeffs(self):
        """batch * n_coeffs values below 2^256, every fifth one at or above p (modntt_cases.inputs)"""
        if self.const is not None:
            return [self.const] * (self.batch * self.n_coeffs)
        return mc.inputs(self.n * 31 + self.md + self.batch, self.batch * self.n_coeffs, self.p)

    def wire(self):
        return mc.wire(self.coeffs())

    def rounds(self):
        r, md = 0, self.md
        while md > 16:
            r, md = r + 1, md // 4
        return r


def _grid():
    out = []
    every = sorted(MODULI)
    # zero rounds: the final layer is all there is
    for name in every:
        out += [Case(name, 16, 16, 3), Case(name, 16, 16, 16), Case(name, 4, 1, 1)]
        out.append(Case(name, 1, 1, 1, verify=False))  # the reference's verifier cannot merkelize one value
    with_64 = [m for m in every if m not in ("f17", "composite")]
    # one round, final layer = the column
    out += [Case(name, 64, 32, 32) for name in with_64]
    # two rounds
    out += [Case(name, 256, 128, 128) for name in ("f257", "f65537", "c2", "bn254", "goldilocks")]
    out += [Case(name, 1024, 256, 256, exclude=8) for name in ("f65537", "babybear", "bls12_381", "p43")]
    # three rounds, a short input
    out += [Case(name, 4096, 1024, 1000) for name in ("bn254", "goldilocks")]
    # sample counts of the first round
    # (the reference's verifier asks every round for the count it is given, its prover gives later rounds 40: a two-round proof with
    # 80 samples is well formed and cannot be verified, fri.py:262-266 against fri.py:268-366; the one-round case beside it can)
    out += [Case("bn254", 256, 128, 100, samples=7), Case("goldilocks", 256, 128, 128, samples=80, verify=False),
            Case("goldilocks", 256, 64, 64, samples=80)]
    # batches
    out += [Case("bn254", 64, 32, 30, batch=3), Case("bls12_381", 1024, 256, 256, batch=3)]
    # above the MiMC prime: every hashed and written value is p - 1
    out += [Case("p43", 64, 32, 1, const=P43 - 1), Case("p43", 16, 16, 1, const=P43 - 1)]
    return out


GRID = _grid()
# both tree forms in one commit: n * batch is above MERKLE_SERIAL_MAX_LEAVES = 2^15, the later rounds are below it (GPU half only)
BOTH_TREE_FORMS = Case("bn254", 1 << 14, 1 << 11, 1 << 11, batch=3)
HOST_GRID = [c for c in GRID if c.n <= 4096]

# the three cases of tests/golden/mod_fri.json (generate_mod_fri.py)
FIXTURE = {
    "bn254-64": Case("bn254", 64, 32, 32),
    "f65537-256-x4": Case("f65537", 256, 128, 128, exclude=4),
    "p43-const": Case("p43", 64, 32, 1, const=P43 - 1),
}


@functools.lru_cache(maxsize=None)
def _oracle(case_id):
    c = _BY_ID[case_id]
    co, proofs, traces = c.coeffs(), [], []
    for b in range(c.batch):
        tr = []
        proofs.append(pyoracle.prove_low_degree(co[b * c.n_coeffs:(b + 1) * c.n_coeffs], c.root, c.md, p=c.p, exclude_multiples_of=c.exclude,
                                                fri_spot_check_security_factor=c.samples, trace=tr))
        traces.append(tr)
    return proofs, traces


_BY_ID = {c.id: c for c in GRID + [BOTH_TREE_FORMS] + list(FIXTURE.values())}


def oracle_proofs(c):
    """the nested proofs of the batch, computed once per process"""
    return _oracle(c.id)[0]


def oracle_traces(c):
    return _oracle(c.id)[1]


def oracle_flat(c):
    return b"".join(pyoracle.proof_flat(p) for p in oracle_proofs(c))


def merkle_root(c, b=0):
    """the commitment the proof of polynomial b speaks about: the root of the tree over its evaluations"""
    co = c.coeffs()[b * c.n_coeffs:(b + 1) * c.n_coeffs]
    return pyoracle.merkelize(mc.transform(co, c.n, c.p, c.root))[1]


def oracle_verify(c, proof, b=0):
    return pyoracle.verify_low_degree_proof(proof, merkle_root(c, b), c.root, c.md, p=c.p, exclude_multiples_of=c.exclude,
                                            fri_spot_check_security_factor=c.samples)


def fold_challenges(p, xs, row):
    """0, 1, p - 1, p, 2^256 - 1, the domain point xs[row] (the row through it returns that row's own value) and the negative of one"""
    return [0, 1, p - 1, p, 2**256 - 1, xs[row], (p - xs[(row + 1) % len(xs)]) % p]


def recorded(c):
    """what tests/golden/mod_fri.json keeps of a case: the digest and the head of the flat proof, each round's two roots and ys"""
    import hashlib
    flat = oracle_flat(c)
    return {"modulus": c.name, "p": c.p, "n": c.n, "maxdeg_plus_1": c.md, "n_coeffs": c.n_coeffs, "exclude": c.exclude, "root": c.root,
            "len": len(flat), "sha256": hashlib.sha256(flat).hexdigest(), "head": flat[:64].hex(), "rounds": oracle_traces(c)[0]}
