#!/usr/bin/env python3
"""Golden vectors of multi_inv and multi_interp_4 (starks/poly_utils.py:301-320, 412-440): imports the LIVE reference (read-only,
/root/reference) and writes tests/golden/poly_utils.json.  Run in the build container only -- the reference never travels to the
GPU box:
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_poly_utils.py

The reference's multi_inv tests the truthiness of each input (poly_utils.py:317): a Python int 0 maps to 0, a zero FIELD ELEMENT
(always truthy) maps to 1.  Both forms are recorded: "out_ints" = the reference on int inputs (what sh_multi_inv computes),
"out_elems" = the reference on field elements (what starks_amd.poly_utils.multi_inv returns for them).  multi_interp_4 always hands
field elements to multi_inv, so its degenerate rows (a repeated x, e_k = 0) carry the 1.

Fixtures hold data only (inputs, outputs, digests) -- no reference source text.
"""
import hashlib
import json
import os
import struct
import sys

sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
from starks.modp import IntegersModP  # noqa: E402
from starks.poly_utils import multi_interp_4, multi_inv  # noqa: E402
from starks.utils import get_power_cycle  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
P = 2**256 - 2**32 * 351 + 1
F = IntegersModP(P)


def hx(v):
    return int(v).to_bytes(32, "big").hex()


def sha(vals):
    return hashlib.sha256(b"".join(int(v).to_bytes(32, "big") for v in vals)).hexdigest()


def seeded(seed, i):
    """x_i = BLAKE2s(seed_le64 || i_le64) mod p  (tests/golden/generate.py)."""
    return int.from_bytes(hashlib.blake2s(struct.pack("<QQ", seed, i)).digest(), "big") % P


def small_field_cases(p, vectors):
    field = IntegersModP(p)
    out = []
    for v in vectors:
        out.append({"p": p, "in": v, "out_elems": [int(x) for x in multi_inv(field, [field(x) for x in v])],
                    "out_ints": [int(x) for x in multi_inv(field, list(v))]})
    return out


def mimc_case(name, vals, full):
    elems = multi_inv(F, [F(x) for x in vals])
    ints = multi_inv(F, list(vals))
    rec = {"name": name, "n": len(vals), "in_sha": sha(vals), "out_elems_sha": sha(elems), "out_ints_sha": sha(ints),
           "zeros": [i for i, x in enumerate(vals) if x % P == 0]}
    if full:
        rec.update({"in": [hx(x) for x in vals], "out_elems": [hx(x) for x in elems], "out_ints": [hx(x) for x in ints]})
    return rec


def zero_runs(seed, n, runs):
    vals = [seeded(seed, i) for i in range(n)]
    for a, b in runs:
        for i in range(a, min(b, n)):
            vals[i] = 0
    return vals


def interp_rows(field_p, rows, seed):
    """seeded rows; every 7th row repeats an x (pairs, a triple, all four equal)"""
    xs, ys = [], []
    for r in range(rows):
        x = [seeded(seed, 8 * r + k) % field_p for k in range(4)]
        y = [seeded(seed + 1, 8 * r + k) % field_p for k in range(4)]
        kind = r % 7
        if kind == 1:
            x[1] = x[0]
        elif kind == 2:
            x[3] = x[2]
        elif kind == 3:
            x[2] = x[1] = x[0]
        elif kind == 4:
            x = [x[0]] * 4
        elif kind == 5:
            x[2], x[3] = x[0], x[1]
        xs.append(x)
        ys.append(y)
    return xs, ys


def interp_case(name, p, xs, ys):
    field = IntegersModP(p)
    polys = multi_interp_4(field, [[field(v) for v in row] for row in xs], [[field(v) for v in row] for row in ys])
    return {"name": name, "p": p, "xs": [[hx(v) for v in row] for row in xs], "ys": [[hx(v) for v in row] for row in ys],
            # the polynomials as the reference returns them: trailing zero coefficients stripped
            "coeffs": [[hx(c) for c in poly.coefficients] for poly in polys]}


def main():
    out = {}
    # test_poly_utils.py:74-87 (Z/7), and small-field vectors with zeros (Z/7, Z/31)
    out["small"] = small_field_cases(7, [[6, 6, 6], [6, 1, 6], [0, 1, 1], [3, 0, 5], [0], [0, 0], [2, 4, 0, 6, 0, 1]]) + \
        small_field_cases(31, [[1, 2, 3, 30], [0, 5, 0, 7, 0], [17] * 9, [i for i in range(31)]])
    # test_poly_utils.py:88-104: x - 1 over the 4096th roots of unity, and Z(x) = x^512 - 1 on them (zeros every 8th)
    G2 = F(7) ** ((P - 1) // 4096)
    xs = get_power_cycle(G2, F)
    xs_minus_1 = [int(x - 1) for x in xs]
    z_evals = [int(xs[(i * 512) % 4096] - 1) for i in range(4096)]
    cases = [mimc_case("xs_minus_1_4096", xs_minus_1, False), mimc_case("z_evals_4096", z_evals, False)]
    # seeded vectors with runs of zeros; the first small enough to store whole
    cases.append(mimc_case("seeded_64_zero_runs", zero_runs(21, 64, [(0, 1), (9, 12), (63, 64)]), True))
    cases.append(mimc_case("seeded_1000_zero_runs", zero_runs(22, 1000, [(0, 3), (100, 164), (511, 520), (999, 1000)]), False))
    cases.append(mimc_case("seeded_5000_zero_tile", zero_runs(23, 5000, [(1024, 2048), (4095, 4100)]), False))
    cases.append(mimc_case("seeded_3_all_zero", [0, 0, 0], True))
    out["mimc"] = cases
    # multi_interp_4: test_poly_utils.py:158-169 (Z/7), seeded MiMC rows with degenerate ones, Z/31 rows
    out["interp"] = [
        interp_case("z7_identity", 7, [[1, 2, 3, 6]] * 2, [[1, 2, 3, 6]] * 2),
        interp_case("z7_degenerate", 7, [[1, 1, 3, 6], [2, 2, 2, 2], [0, 1, 2, 3]], [[1, 2, 3, 6], [5, 4, 3, 2], [0, 0, 0, 0]]),
        interp_case("z31_rows", 31, *interp_rows(31, 21, 31)),
        interp_case("mimc_rows_70", P, *interp_rows(P, 70, 41)),
    ]
    path = os.path.join(HERE, "poly_utils.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=0)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
