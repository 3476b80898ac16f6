#!/usr/bin/env python3
"""Golden vectors of the packed-word transform (starks/fft.py:316-345: fft_1d and mul_polys with a modulus below 2^64 as an argument):
imports the LIVE reference (read-only, /root/reference) and writes tests/golden/mod64_ntt.json.  Run in the build container only -- the
reference never travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_mod64_ntt.py

Per modulus (Goldilocks, BabyBear, 65537) and n = 8, 64, 1024: the reference's own fft_1d forward, inverse and zero-padded (n / 2 + 1
inputs) outputs, and mul_polys of n / 2 + 1 by n / 4 + 1 coefficients.  Inputs are stored as their recipe (tests/ntt64_cases.py:
inputs(seed, count, p) -- every fifth value is at or above p, the reference reduces it through IntegersModP), outputs as
tests/modntt_cases.py: recorded keeps them: every value at n = 8, the SHA-256 of the 32-byte big-endian form with the first four values
and the last one at n = 64 and 1024.

Fixtures hold data only (inputs, outputs) -- no reference source text.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from modntt_cases import recorded  # noqa: E402
from ntt64_cases import MODULI, inputs, root_of  # noqa: E402
sys.path.insert(0, "/root/reference")
from starks.fft import fft_1d, mul_polys  # noqa: E402
from starks.modp import IntegersModP  # noqa: E402


def main():
    cases = []
    for k, name in enumerate(["goldilocks", "babybear", "f65537"]):
        p = MODULI[name]
        F = IntegersModP(p)
        for n in (8, 64, 1024):
            w = root_of(name, n)
            seed = 8000 + 10 * k + n
            full = [F(v) for v in inputs(seed, n, p)]
            short = [F(v) for v in inputs(seed + 1, n // 2 + 1, p)]
            a = [F(v) for v in inputs(seed + 2, n // 2 + 1, p)]
            b = [F(v) for v in inputs(seed + 3, n // 4 + 1, p)]
            cases.append({"modulus": name, "p": p, "n": n, "root": w, "seed": seed,
                          "forward": recorded(fft_1d(F, full, p, F(w))),
                          "inverse": recorded(fft_1d(F, full, p, F(w), inv=True)),
                          "padded": recorded(fft_1d(F, short, p, F(w))),
                          "mul_polys": recorded(mul_polys(a, b, F(w)))})
    with open(os.path.join(HERE, "mod64_ntt.json"), "w") as fh:
        fh.write('{"cases": [\n%s]}\n' % ",\n".join(json.dumps(c) for c in cases))


if __name__ == "__main__":
    main()
