#!/usr/bin/env python3
"""Golden vectors of polynomial evaluation (starks/polynomial.py:158-164, Polynomial.__call__): imports the LIVE reference
(read-only, /root/reference) and writes tests/golden/poly_eval.json.  Run in the build container only -- the reference never
travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_poly_eval.py

Coefficients and points are what is handed to the reference: ints in [0, 2^256) (some >= p, unreduced wire values), and in one case
negative ints; the reference reduces them through IntegersModP.  Seeded inputs are stored as their recipe (tests/poly_arith_cases.py:
operand), the values P(x_i) as a list of ints, one per point.  The cases include n = 0 (the zero polynomial: every value is 0), n = 1,
the point 0, repeated points, trailing zero coefficients (which the reference strips), up to 2^10 coefficients and 2^6 points.

Fixtures hold data only (inputs, outputs) -- no reference source text.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from poly_arith_cases import operand  # noqa: E402
sys.path.insert(0, "/root/reference")
from starks.modp import IntegersModP  # noqa: E402
from starks.polynomial import polynomials_over  # noqa: E402

P = 2**256 - 2**32 * 351 + 1
F = IntegersModP(P)
POLY = polynomials_over(F)


def main():
    def S(seed, n, big=0):
        return {"seed": seed, "n": n, "big": big}

    cases = []

    def case(name, coefs, xs):
        poly = POLY([F(c) for c in operand(coefs)])
        cases.append({"name": name, "coefs": coefs, "xs": xs, "out": [int(poly(F(x))) for x in operand(xs)]})

    for k, (n, m) in enumerate([(2, 1), (3, 2), (7, 3), (8, 4), (9, 5), (64, 8), (129, 17), (255, 31), (1000, 64), (1024, 33)]):
        case("random_%d_%d" % (n, m), S(900 + k, n, 5), S(950 + k, m, 3))
    case("zero_poly", [], S(990, 4, 2))
    case("constant", S(991, 1, 1), S(992, 5, 2))
    xs = operand(S(993, 12))
    xs[2] = 0
    xs[5] = xs[6] = xs[0]
    case("zero_and_repeated_x", S(994, 40, 4), xs)
    case("all_points_equal", S(995, 17), [xs[1]] * 6)
    case("only_zero_point", S(996, 33, 2), [0, 0, 0])
    case("trailing_zeros", operand(S(997, 10)) + [0, 0, 0, P, 0], S(998, 7))
    case("negative", [-1, -(P + 2), 5, 2**256 - 1], [-3, 2**256 - 1, P, P + 1])
    case("unreduced_all", [P + 1] * 9, [2**256 - 1, P + 7])
    with open(os.path.join(HERE, "poly_eval.json"), "w") as fh:
        fh.write('{"p": %d,\n"eval": [\n%s]}\n' % (P, ",\n".join(json.dumps(c) for c in cases)))


if __name__ == "__main__":
    main()
