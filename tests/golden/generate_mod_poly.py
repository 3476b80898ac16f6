#!/usr/bin/env python3
"""Golden vectors of polynomial products, divmod, zpoly, lagrange_interp, multi_inv and multi_interp_4 over OTHER prime fields
(starks/polynomial.py:116-150, starks/poly_utils.py:301-369, 412-440 over IntegersModP(p)): imports the LIVE reference (read-only,
/root/reference) and writes tests/golden/mod_poly.json.  Run in the build container only -- the reference never travels to the GPU
box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_mod_poly.py

The moduli are BN254 r, BLS12-381 r, Goldilocks, 65537 and 97.  Inputs are what is handed to the reference: ints in [0, 2^256) (some
>= p, unreduced wire values), and for lagrange_interp also negative ints; the reference reduces them through IntegersModP.  Seeded
inputs are stored as their recipe and outputs as length + sha256, with the values themselves when short (tests/modpoly_cases.py:
operand, record).  Polynomial outputs are the reference's coefficients, trailing zeros stripped.  multi_inv is recorded on int inputs
reduced mod p (a zero int maps to 0: what the device computes); multi_interp_4 always hands field elements to multi_inv, so its
degenerate rows (a repeated x) carry the reference's 1.  A case whose largest transform exceeds what the field's 2-adicity admits is
not generated (97 admits transforms up to 32).  The reference's lagrange_interp is O(n^3): n <= 128.

Fixtures hold data only (inputs, outputs, digests) -- no reference source text.
"""
import contextlib
import io
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
from starks.poly_utils import lagrange_interp, multi_interp_4, multi_inv, zpoly  # noqa: E402


def ints(poly):
    return [int(c) for c in poly.coefficients]


def quiet(fn, *args):
    with contextlib.redirect_stdout(io.StringIO()):  # the reference's zpoly prints its result
        return fn(*args)


def S(seed, n, big=0):
    return {"seed": seed, "n": n, "big": big}


def cases_of(p, tag):
    F = IntegersModP(p)
    POLY = polynomials_over(F)
    admits = 1 << min(mp.FIELDS[p][0], mp.MAX_ROOT_LOG)
    out = []

    def fits(op, na, nb=0):
        return mp.max_transform(op, na, nb) <= admits

    def add(op, name, **f):
        out.append(dict({"p": p, "op": op, "name": name}, **f))

    for k, (na, nb) in enumerate([(1, 1), (1, 7), (3, 4), (16, 17), (33, 64), (100, 1), (128, 129), (5, 200)]):
        if fits(mp.OP_MUL, na, nb):
            a, b = S(tag + 100 + k, na, 5), S(tag + 200 + k, nb, 7)
            add("mul", "%dx%d" % (na, nb), a=a, b=b, out=record(ints(POLY(operand(p, a)) * POLY(operand(p, b)))))
    div = [("deg0", 40, 1, False), ("deg1", 40, 2, False), ("monic", 64, 9, True), ("nonmonic", 65, 9, False), ("equal", 17, 17, False),
           ("short", 5, 9, False), ("exact", 50 + 21 - 1, 21, False), ("big", 200, 77, False), ("half", 128, 65, False),
           ("one_coeff", 1, 1, False), ("small_monic", 12, 5, True), ("small_exact", 6 + 4 - 1, 4, False)]
    for k, (name, na, nb, monic) in enumerate(div):
        if not fits(mp.OP_DIVMOD, na, nb):
            continue
        if name.endswith("exact"):
            b = S(tag + 400 + k, nb, 4)
            a = {"product": [S(tag + 300 + k, na - nb + 1, 3), b]}
        else:
            a, b = S(tag + 300 + k, na, 6), S(tag + 400 + k, nb, 5)
            b = operand(p, b)
            b[-1] = 1 if monic else (b[-1] if b[-1] % p else 1)  # the leading coefficient must not vanish (small fields)
        qq, rr = divmod(POLY(operand(p, a)), POLY(operand(p, b)))
        add("divmod", name, a=a, b=b, q=record(ints(qq)), r=record(ints(rr)))
    for k, n in enumerate([0, 1, 2, 3, 5, 8, 13, 32, 64, 100, 129]):
        if fits(mp.OP_ZPOLY, n):
            xs = S(tag + 500 + k, n, 4)
            add("zpoly", "n%d" % n, xs=xs, out=record(ints(quiet(zpoly, F, operand(p, xs)))))

    def lag(name, xs, ys):
        if fits(mp.OP_LAGRANGE, len(operand(p, xs))):
            res = quiet(lagrange_interp, F, list(operand(p, xs)), list(operand(p, ys)))
            add("lagrange", name, xs=xs, ys=ys, out=record(ints(res)))

    for k, n in enumerate([0, 1, 2, 3, 4, 7, 16, 17, 33, 64, 100, 128]):
        lag("random_%d" % n, S(tag + 600 + k, n, 5), S(tag + 700 + k, n, 6))
    xs = operand(p, S(tag + 800, 16))
    xs[3] = xs[0]
    xs[7] = xs[8] = xs[9]
    lag("repeated", xs, S(tag + 801, 16))
    lag("all_repeated", [xs[0]] * 6, S(tag + 802, 6))
    lag("zero_ys", S(tag + 803, 12), [0] * 12)
    lag("zero_ys_repeated", [5, 5, 6], [0, 0, 0])
    lag("negative", [-1, -2, 3, -(p + 5), 2**256 - 1], [-7, 2**256 - 2, 0, 1, -p])
    lag("zero_x", [0, 1, 0, 2], [3, 4, 5, 6])
    lag("one", [p + 3], [p - 1])

    for k, n in enumerate([1, 5, 64, 300]):
        v = S(tag + 900 + k, n, 6)
        vals = [x % p for x in operand(p, v)]
        zeros = [i for i in (0, 3, n - 1) if i < n and n > 1]
        for i in zeros:
            vals[i] = 0
        add("multi_inv", "n%d" % n, **{"in": v, "zeros": zeros, "out": record([int(x) for x in multi_inv(F, vals)])})
    for k, rows in enumerate([1, 9, 40]):
        xs, ys = operand(p, S(tag + 950 + k, 4 * rows, 9)), S(tag + 960 + k, 4 * rows, 11)
        for r in range(rows):  # every 4th row repeats an x: a pair, a triple, all four
            if r % 4 == 1:
                xs[4 * r + 1] = xs[4 * r]
            elif r % 4 == 2 and r % 8 == 2:
                xs[4 * r + 1] = xs[4 * r + 3] = xs[4 * r]
            elif r % 4 == 2:
                xs[4 * r + 1] = xs[4 * r + 2] = xs[4 * r + 3] = xs[4 * r]
        yv = operand(p, ys)
        res = multi_interp_4(F, [[F(x) for x in xs[4 * r:4 * r + 4]] for r in range(rows)],
                             [[F(y) for y in yv[4 * r:4 * r + 4]] for r in range(rows)])
        flat = []
        for poly in res:
            c = ints(poly)
            flat += c + [0] * (4 - len(c))
        add("multi_interp_4", "rows%d" % rows, xs=xs, ys=ys, out=record(flat))
    return out


def main():
    cases = []
    for k, p in enumerate(mp.FIXTURE_MODULI):
        cases += cases_of(p, 10000 * (k + 1))
    with open(os.path.join(HERE, "mod_poly.json"), "w") as fh:  # one case per line
        fh.write('{"moduli": %s,\n"cases": [\n%s]}\n' % (json.dumps(mp.FIXTURE_MODULI), ",\n".join(json.dumps(c) for c in cases)))


if __name__ == "__main__":
    main()
