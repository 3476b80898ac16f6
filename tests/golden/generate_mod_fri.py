#!/usr/bin/env python3
"""Golden vectors of the FRI commit over other moduli: imports the LIVE reference (read-only, /root/reference) and writes
tests/golden/mod_fri.json.  Run in the build container only -- the reference never travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_mod_fri.py

The FRI driver (SmoothSubgroupFRI) is a comment block in the reference (starks/fri.py:176-366), so it cannot be imported.  `ref_prove`
below drives the reference's live primitives -- NonBinaryFFT, merkelize, multi_interp_4, get_pseudorandom_indices, mk_branch -- in the
order that comment block prescribes (fri.py:189-266), exactly as tests/golden/generate.py does over the MiMC prime, with
F = IntegersModP(p): every arithmetic step is executed by reference code, only the sequencing is written here.

Three cases (tests/modfri_cases.py: FIXTURE): BN254 at n = 64, 65537 at n = 256 with exclude_multiples_of = 4, and the constant
polynomial p - 1 over P43 = 2^256 - 43 * 2^32 + 1, a prime above the MiMC prime.  Per case: the SHA-256 and the first 64 bytes of the
flat proof, each round's two roots and sampled indices.  Inputs are stored as their recipe (modfri_cases.Case.coeffs).

Fixtures hold data only (inputs, outputs, digests) -- no reference source text.
"""
import hashlib
import json
import os
import sys

sys.dont_write_bytecode = True
sys.setrecursionlimit(10000)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from modfri_cases import FIXTURE  # noqa: E402
sys.path.insert(0, "/root/reference")
from starks.fft import NonBinaryFFT  # noqa: E402
from starks.merkle_tree import merkelize, mk_branch  # noqa: E402
from starks.modp import IntegersModP  # noqa: E402
from starks.poly_utils import multi_interp_4  # noqa: E402
from starks.polynomial import polynomials_over  # noqa: E402
from starks.utils import get_power_cycle, get_pseudorandom_indices  # noqa: E402


def ref_prove(F, f, root_of_unity, maxdeg_plus_1, exclude_multiples_of=0, samples=40, trace=None):
    values = NonBinaryFFT(F, root_of_unity).fft(f)
    if maxdeg_plus_1 <= 16:
        return [[x.to_bytes() for x in values]]
    xs = get_power_cycle(root_of_unity, F)
    assert len(values) == len(xs)
    m = merkelize(values)
    special_x = F(m[1])
    q = len(xs) // 4
    x_polys = multi_interp_4(
        F,
        [[xs[i + q * j] for j in range(4)] for i in range(q)],
        [[values[i + q * j] for j in range(4)] for i in range(q)])
    column = [p(special_x) for p in x_polys]
    m2 = merkelize(column)
    ys = get_pseudorandom_indices(m2[1], len(column), samples, exclude_multiples_of=exclude_multiples_of)
    branches = []
    for y in ys:
        branches.append([mk_branch(m2, y)] + [mk_branch(m, y + q * j) for j in range(4)])
    if trace is not None:
        trace.append({"n": len(xs), "root_m": m[1].hex(), "root_m2": m2[1].hex(), "ys": ys})
    o = [m2[1], branches]
    column_poly = NonBinaryFFT(F, root_of_unity ** 4).inv_fft(column)
    # the recursion does not forward `samples`: later rounds use the default 40 (fri.py:262-266)
    return [o] + ref_prove(F, column_poly, root_of_unity ** 4, maxdeg_plus_1 // 4, exclude_multiples_of=exclude_multiples_of, trace=trace)


def proof_flat(proof):
    out = []
    for root, branches in proof[:-1]:
        out.append(root)
        for bset in branches:
            for b in bset:
                out.extend(b)
    out.extend(proof[-1])
    return b"".join(out)


def main():
    cases = {}
    for key, c in FIXTURE.items():
        F = IntegersModP(c.p)
        poly = polynomials_over(F).factory([F(v) for v in c.coeffs()])
        trace = []
        flat = proof_flat(ref_prove(F, poly, F(c.root), c.md, exclude_multiples_of=c.exclude, samples=c.samples, trace=trace))
        cases[key] = {"modulus": c.name, "p": c.p, "n": c.n, "maxdeg_plus_1": c.md, "n_coeffs": c.n_coeffs, "exclude": c.exclude,
                      "root": c.root, "len": len(flat), "sha256": hashlib.sha256(flat).hexdigest(), "head": flat[:64].hex(),
                      "rounds": trace}
    with open(os.path.join(HERE, "mod_fri.json"), "w") as fh:
        fh.write('{"cases": {\n%s}}\n' % ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in cases.items()))


if __name__ == "__main__":
    main()
