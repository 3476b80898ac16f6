#!/usr/bin/env python3
"""Golden vectors of the computational trace over other moduli: imports the LIVE reference and writes tests/golden/mod_witness.json.
Run where the reference is present -- it never travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_mod_witness.py

The trace is the reference's air.get_computational_trace over F = IntegersModP(p) with multivariates_over(F, width) step polynomials,
laid out as AIR.generate_witness does (air.py:121-123: witness[dim][step]) and serialised with the elements' own to_bytes (32 bytes
big-endian, modp.py:94-95).  AIR's constructor itself asserts steps == 2**9 - 1 (air.py:94) and is not used, exactly as in
generate_mod_stark.py.

Four cases (tests/modwitness_cases.py: FIXTURE): BN254 MiMC at 64 steps, Goldilocks width 3 at 64, BabyBear X^3 + 7 at 64 (a modulus
the generic prover refuses), and the constant trace p - 1 over P43 = 2^256 - 43 * 2^32 + 1 at 16 steps.  Per case: the inputs, the step
polynomials and the SHA-256 of the witness bytes.  tests/test_modwitness_host.py checks that oracle/pyoracle.py's trace hashes to the
same value, which pins the oracle of every other test to the reference for moduli other than the MiMC prime.

Fixtures hold data only (inputs, step polynomials, digests) -- no reference source text.
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
from modwitness_cases import FIXTURE, MODULI  # noqa: E402
import generate_mod_fri  # noqa: E402,F401  (puts the reference on sys.path)
from starks.modp import IntegersModP  # noqa: E402


def main():
    from starks.air import get_computational_trace
    from starks.poly_utils import multivariates_over
    cases = {}
    for key, (name, sp, steps, inputs) in FIXTURE.items():
        p, width = MODULI[name], len(sp)
        F = IntegersModP(p)
        mv = multivariates_over(F, width).factory
        step_polys = [mv({k: F(v) for k, v in d.items()}) for d in sp]
        with contextlib.redirect_stdout(io.StringIO()):
            trace, _ = get_computational_trace([F(v) for v in inputs], steps, width, step_polys)
        witness = [[trace[i][j] for i in range(steps)] for j in range(width)]
        raw = b"".join(x.to_bytes() for col in witness for x in col)
        assert len(raw) == 32 * width * steps
        cases[key] = {"modulus": name, "p": p, "steps": steps, "width": width, "inputs": inputs,
                      "step_polys": [[[list(k), v] for k, v in sorted(d.items())] for d in sp],
                      "sha256": hashlib.sha256(raw).hexdigest(), "last": [int(col[-1]) for col in witness]}
        print("%s: %d bytes" % (key, len(raw)))
    with open(os.path.join(HERE, "mod_witness.json"), "w") as fh:
        fh.write('{"cases": {\n%s}}\n' % ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in cases.items()))


if __name__ == "__main__":
    main()
