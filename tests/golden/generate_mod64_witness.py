#!/usr/bin/env python3
"""Golden vectors of the computational trace over moduli below 2^64, as packed words: imports the LIVE reference and writes
tests/golden/mod64_witness.json.  Run where the reference is present -- it never travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_mod64_witness.py

The trace is the reference's air.get_computational_trace over F = IntegersModP(p) with multivariates_over(F, width) step polynomials,
laid out as AIR.generate_witness does (air.py:121-123: witness[dim][step]), each element written as one native (little-endian) 8-byte
word: what sh_mod64_stark_witness returns.  AIR's constructor itself asserts steps == 2**9 - 1 (air.py:94) and is not used, exactly as
in generate_mod_witness.py.

Four cases (tests/mod64witness_cases.py: FIXTURE): Goldilocks width 3 at 64 steps, BabyBear X^3 + 7 at 64 (a modulus the provers
refuse), BIG18 = 2^64 - 1835007 MiMC at 64 (sums carry out of the word), and the constant trace p - 1 of X' = X^3 over the composite
2^64 - 1 at 16 steps.  Per case: the inputs, the step polynomials, the SHA-256 of the words and the last row.
tests/test_mod64witness_host.py checks that oracle/pyoracle.py's trace hashes to the same value, which pins the oracle of every other
test of the packed-word generator to the reference.

Fixtures hold data only (inputs, step polynomials, digests) -- no reference source text.
"""
import contextlib
import hashlib
import io
import json
import os
import struct
import sys

sys.dont_write_bytecode = True
sys.setrecursionlimit(10000)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from mod64witness_cases import FIXTURE, MODULI  # noqa: E402
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
        witness = [[int(trace[i][j]) for i in range(steps)] for j in range(width)]
        raw = struct.pack("<%dQ" % (width * steps), *[x for col in witness for x in col])
        cases[key] = {"modulus": name, "p": p, "steps": steps, "width": width, "inputs": inputs,
                      "step_polys": [[[list(k), v] for k, v in sorted(d.items())] for d in sp],
                      "sha256": hashlib.sha256(raw).hexdigest(), "last": [col[-1] for col in witness]}
        print("%s: %d bytes" % (key, len(raw)))
    with open(os.path.join(HERE, "mod64_witness.json"), "w") as fh:
        fh.write('{"cases": {\n%s}}\n' % ",\n".join('"%s": %s' % (k, json.dumps(v)) for k, v in cases.items()))


if __name__ == "__main__":
    main()
