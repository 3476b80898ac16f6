#!/usr/bin/env python3
"""Golden vectors of polynomial evaluation over OTHER prime fields (starks/polynomial.py:158-164, Polynomial.__call__ over
IntegersModP(p)): imports the LIVE reference (read-only, /root/reference) and writes tests/golden/mod_poly_eval.json.  Run in the build
container only -- the reference never travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_mod_poly_eval.py

The moduli are modpoly_cases.FIXTURE_MODULI (BN254 r, BLS12-381 r, Goldilocks, 65537 and 97) and the cases those of
generate_poly_eval.py: the zero polynomial and a constant, the point 0, repeated points and all points equal, trailing zeros,
negative and unreduced inputs, random shapes up to 1000 x 64.  Inputs are what is handed to the reference: ints in [0, 2^256) (some
>= p), and in one case negative ints; the reference reduces them through IntegersModP.  Seeded inputs are stored as their recipe and
the values P(x_i) as length + sha256, with the values themselves when short (tests/modpoly_cases.py: operand, record).

Fixtures hold data only (inputs, outputs, digests) -- no reference source text.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import modpoly_cases as mp  # noqa: E402
from modpoly_cases import operand, record  # noqa: E402
sys.path.insert(0, "/root/reference")
from starks.modp import IntegersModP  # noqa: E402
from starks.polynomial import polynomials_over  # noqa: E402


def S(seed, n, big=0):
    return {"seed": seed, "n": n, "big": big}


def cases_of(p, tag):
    F = IntegersModP(p)
    POLY = polynomials_over(F)
    out = []

    def case(name, coefs, xs):
        poly = POLY([F(c) for c in operand(p, coefs)])
        out.append({"p": p, "op": "eval", "name": name, "a": coefs, "xs": xs, "out": record([int(poly(F(x))) for x in operand(p, xs)])})

    for k, (n, m) in enumerate([(2, 1), (3, 2), (7, 3), (8, 4), (9, 5), (64, 8), (129, 17), (255, 31), (1000, 64), (1024, 33)]):
        case("random_%d_%d" % (n, m), S(tag + 900 + k, n, 5), S(tag + 950 + k, m, 3))
    case("zero_poly", [], S(tag + 990, 4, 2))
    case("constant", S(tag + 991, 1, 1), S(tag + 992, 5, 2))
    xs = operand(p, S(tag + 993, 12))
    xs[2] = 0
    xs[5] = xs[6] = xs[0]
    case("zero_and_repeated_x", S(tag + 994, 40, 4), xs)
    case("all_points_equal", S(tag + 995, 17), [xs[1]] * 6)
    case("only_zero_point", S(tag + 996, 33, 2), [0, 0, 0])
    case("trailing_zeros", operand(p, S(tag + 997, 10)) + [0, 0, 0, p, 0], S(tag + 998, 7))
    case("negative", [-1, -(p + 2), 5, 2**256 - 1], [-3, 2**256 - 1, p, p + 1])
    case("unreduced_all", [p + 1] * 9, [2**256 - 1, p + 7])
    return out


def main():
    cases = []
    for k, p in enumerate(mp.FIXTURE_MODULI):
        cases += cases_of(p, 10000 * (k + 1))
    with open(os.path.join(HERE, "mod_poly_eval.json"), "w") as fh:  # one case per line
        fh.write('{"moduli": %s,\n"cases": [\n%s]}\n' % (json.dumps(mp.FIXTURE_MODULI), ",\n".join(json.dumps(c) for c in cases)))


if __name__ == "__main__":
    main()
