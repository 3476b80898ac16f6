#!/usr/bin/env python3
"""Golden vectors of polynomial products, divmod, zpoly and lagrange_interp (starks/polynomial.py:116-150,
starks/poly_utils.py:322-369): imports the LIVE reference (read-only, /root/reference) and writes tests/golden/poly_arith.json.
Run in the build container only -- the reference never travels to the GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_poly_arith.py

Inputs are what is handed to the reference: ints in [0, 2^256) (some >= p, unreduced wire values), and for lagrange_interp also
negative ints; the reference reduces them through IntegersModP.  Seeded inputs are stored as their recipe and outputs (the
reference's coefficients, trailing zeros stripped) as length + sha256, with the values themselves when short
(tests/poly_arith_cases.py: operand, record).  The lagrange cases include repeated x's (the reference's multi_inv turns their zero
denominators into 1, poly_utils.py:317), all-zero ys, n = 0 and n = 1.  The reference's lagrange_interp is O(n^3): n <= 128.

Fixtures hold data only (inputs, outputs) -- no reference source text.
"""
import contextlib
import io
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from poly_arith_cases import operand, record  # noqa: E402
sys.path.insert(0, "/root/reference")
from starks.modp import IntegersModP  # noqa: E402
from starks.polynomial import polynomials_over  # noqa: E402
from starks.poly_utils import lagrange_interp, zpoly  # noqa: E402

P = 2**256 - 2**32 * 351 + 1
F = IntegersModP(P)
POLY = polynomials_over(F)


def ints(poly):
    return [int(c) for c in poly.coefficients]


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):  # the reference's zpoly prints its result
        return fn(*args)


def main():
    def S(seed, n, big=0):
        return {"seed": seed, "n": n, "big": big}

    mul = []
    for k, (na, nb) in enumerate([(1, 1), (1, 7), (3, 4), (16, 17), (33, 64), (100, 1), (128, 129), (5, 200)]):
        a, b = S(100 + k, na, 5), S(200 + k, nb, 7)
        mul.append({"a": a, "b": b, "out": record(ints(POLY(operand(a)) * POLY(operand(b))))})
    divm = []
    cases = [("deg0", 40, 1, False), ("deg1", 40, 2, False), ("monic", 64, 9, True), ("nonmonic", 65, 9, False),
             ("equal", 17, 17, False), ("short", 5, 9, False), ("exact", 0, 0, False), ("big", 200, 77, False),
             ("half", 128, 65, False), ("one_coeff", 1, 1, False)]
    for k, (name, na, nb, monic) in enumerate(cases):
        if name == "exact":
            b = S(400 + k, 21, 4)
            a = {"product": [S(300 + k, 50, 3), b]}
        else:
            a, b = S(300 + k, na, 6), S(400 + k, nb, 5)
            if monic:
                b = operand(b)[:-1] + [1]
        qq, rr = divmod(POLY(operand(a)), POLY(operand(b)))
        divm.append({"name": name, "a": a, "b": b, "q": record(ints(qq)), "r": record(ints(rr))})
    zp = []
    for k, n in enumerate([0, 1, 2, 3, 5, 8, 13, 64, 100, 129]):
        xs = S(500 + k, n, 4)
        zp.append({"xs": xs, "out": record(ints(quiet(zpoly, F, operand(xs))))})
    lag = []

    def lag_case(name, xs, ys):
        out = quiet(lagrange_interp, F, list(operand(xs)), list(operand(ys)))
        lag.append({"name": name, "xs": xs, "ys": ys, "out": record(ints(out))})

    for k, n in enumerate([0, 1, 2, 3, 4, 7, 16, 17, 33, 64, 100, 128]):
        lag_case("random_%d" % n, S(600 + k, n, 5), S(700 + k, n, 6))
    xs = operand(S(800, 20))
    xs[3] = xs[0]
    xs[7] = xs[8] = xs[9]
    lag_case("repeated", xs, S(801, 20))
    lag_case("all_repeated", [xs[0]] * 6, S(802, 6))
    lag_case("zero_ys", S(803, 12), [0] * 12)
    lag_case("zero_ys_repeated", [5, 5, 6], [0, 0, 0])
    lag_case("negative", [-1, -2, 3, -(P + 5), 2**256 - 1], [-7, 2**256 - 2, 0, 1, -P])
    lag_case("zero_x", [0, 1, 0, 2], [3, 4, 5, 6])
    lag_case("one", [P + 3], [P - 1])
    with open(os.path.join(HERE, "poly_arith.json"), "w") as fh:
        groups = [("mul", mul), ("divmod", divm), ("zpoly", zp), ("lagrange", lag)]  # one case per line
        fh.write('{"p": %d,\n' % P + ",\n".join('"%s": [\n%s]' % (k, ",\n".join(json.dumps(c) for c in v)) for k, v in groups) + "}\n")


if __name__ == "__main__":
    main()
