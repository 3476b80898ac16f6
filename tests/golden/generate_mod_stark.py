#!/usr/bin/env python3
"""Golden vectors of STARK.mk_proof over other moduli: imports the LIVE reference (read-only, /root/reference) and writes
tests/golden/mod_stark.json.  Run in the build container only -- the reference never travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_mod_stark.py

starks/stark.py is made importable exactly as tests/golden/generate.py makes it (_load_ref_stark: an FRI class whose two methods are the
sequencing of the reference's live primitives is put into the imported starks.fri module object, in memory), with F = IntegersModP(p)
in place of the MiMC field: the reference's STARK is generic in self.field (stark.py:204-225).  The commit behind it is
generate_mod_fri.py's ref_prove, which takes the field as an argument.  The witness comes from air.get_computational_trace, laid out as
AIR.generate_witness does (air.py:121-123).

Three cases (tests/modstark_cases.py: FIXTURE): BN254 at steps 8, ext 8, width 2; Goldilocks at steps 16, ext 4, width 1; the constant
trace p - 1 over P43 = 2^256 - 43 * 2^32 + 1, a prime above the MiMC prime.  Per case: the flat proof's length, SHA-256, the two roots
and the first 64 bytes.  Inputs are stored as their recipe.

Fixtures hold data only (inputs, outputs, digests) -- no reference source text.
"""
import contextlib
import hashlib
import io
import json
import os
import sys

sys.dont_write_bytecode = True
sys.setrecursionlimit(10000)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from modstark_cases import FIXTURE  # noqa: E402
import generate_mod_fri as gmf  # noqa: E402  (puts the reference on sys.path; ref_prove, proof_flat)
from starks.modp import IntegersModP  # noqa: E402


def load_ref_stark():
    import starks.fri as rfri

    class FRI(object):
        def __init__(self, field):
            self.field = field

        def generate_proximity_proof(self, f, root_of_unity, maxdeg_plus_1, exclude_multiples_of=0, fri_spot_check_security_factor=40):
            return gmf.ref_prove(self.field, f, root_of_unity, maxdeg_plus_1, exclude_multiples_of, fri_spot_check_security_factor)

    rfri.FRI = FRI
    import starks.stark as rstark
    return rstark


def main():
    from starks.air import get_computational_trace
    from starks.poly_utils import multivariates_over
    rstark = load_ref_stark()
    cases = {}
    for key, c in FIXTURE.items():
        F = IntegersModP(c.p)
        mv = multivariates_over(F, c.width).factory
        step_polys = [mv({k: F(v) for k, v in d.items()}) for d in c.sp]
        inputs = [F(v) for v in c.inputs[0]]
        with contextlib.redirect_stdout(io.StringIO()):
            trace, _ = get_computational_trace(inputs, c.steps, c.width, step_polys)
            witness = [[trace[i][j] for i in range(c.steps)] for j in range(c.width)]
            boundary = [(0, j, inputs[j]) for j in range(c.width)]
            m_root, l_root, branches, fri_proof = rstark.STARK(F, c.steps, c.ext, c.width, step_polys).mk_proof(witness, boundary)
        flat = m_root + l_root + b"".join(b"".join(br) for br in branches) + gmf.proof_flat(fri_proof)
        cases[key] = {"modulus": c.name, "p": c.p, "steps": c.steps, "ext": c.ext, "width": c.width, "inputs": c.inputs[0],
                      "step_polys": [[[list(k), v] for k, v in sorted(d.items())] for d in c.sp],
                      "len": len(flat), "sha256": hashlib.sha256(flat).hexdigest(), "m_root": m_root.hex(), "l_root": l_root.hex(),
                      "head": flat[:64].hex()}
        print("%s: %d bytes" % (key, len(flat)))
    with open(os.path.join(HERE, "mod_stark.json"), "w") as fh:
        fh.write('{"cases": {\n%s}}\n' % ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in cases.items()))


if __name__ == "__main__":
    main()
