"""Exact Python-int statement of polynomial evaluation over ANY prime field (starks/polynomial.py:158-164, Polynomial.__call__), the
modulus a parameter -- shared by the host and GPU tests of sh_mod_poly_eval -- with the record format of tests/golden/mod_poly_eval.json
(tests/modpoly_cases.py: an operand is a literal list or a seeded recipe, an output {"len", "sha"} plus "vals" when short) and the
shape grids of both test files."""
from modpoly_cases import (BLS12_381, BN254, FIELDS, FIXTURE_MODULI, GOLDILOCKS, MIMC_P, horner, ints, matches, operand,  # noqa: F401
                           pow2_at_least, record, two_adic_root, vec, wire)

OP_EVAL = 4
MODULI = [3, 97, 65537, GOLDILOCKS, BN254, BLS12_381, MIMC_P]
IDS = {3: "f3", 97: "f97", 65537: "f65537", GOLDILOCKS: "goldilocks", BN254: "bn254", BLS12_381: "bls12_381", MIMC_P: "mimc"}
PE_WG, ME_GROUP, PE_MIN_T, PE_TARGET_WGS = 256, 4, 64, 2048
MAX_COEFS, MAX_TOTAL, MAX_POINTS = 1 << 25, 1 << 26, 1 << 20


def evaluate(p, coefs, xs, batch=1):
    """out[b][i] = sum_k coefs[b][k] xs[i]^k mod p, flat [batch][m]; coefs is flat [batch][n]"""
    n = len(coefs) // batch
    return [horner(p, coefs[b * n:(b + 1) * n], x % p) for b in range(batch) for x in xs]


def max_transform(n, m):
    """sh_mod_poly_max_transform(4, n, m): the tree path's root product"""
    return 2 * pow2_at_least(m) if n and m else 0


def direct_shape(n, m, batch, group=ME_GROUP):
    """pe_direct_shape: (W, T, G)"""
    G = group if m >= group else 1
    groups = (m + G - 1) // G
    W = 1
    while 2 * W * PE_WG * PE_MIN_T <= n and W * groups * batch < PE_TARGET_WGS:
        W *= 2
    return W, (n + W * PE_WG - 1) // (W * PE_WG), G


def direct_preferred(cost, n, m, batch):
    """pe_direct_preferred over five constants, the operations in the order poly_items.cuh writes them (doubles, like Python floats)"""
    products_per_us, floor_us, us_per_level, elements_per_us, us_per_row = cost
    N = pow2_at_least(m)
    C = (n + N - 1) // N
    lg, R = float(N.bit_length() - 1), float(batch) * float(C)
    direct = floor_us + float(batch) * float(n) * float(m) / products_per_us
    tree = us_per_level * lg + (float(N) * lg * lg + 3.0 * R * float(N) * lg) / elements_per_us + us_per_row * R
    return direct <= tree


# the constants of sh_poly_eval's rule as the parent commit has them (poly_items.cuh: PE_DIRECT_PRODUCTS_PER_US ... PE_TREE_US_PER_ROW)
MIMC_COST = (1.9e5, 50.0, 150.0, 8.0e4, 0.8)

SIZES = [0, 1, 2, 3, 7, 8, 9, 127, 128, 129, 255, 256, 257, 1000, 1025]
# tests/test_poly_eval_host.py's pruning: every pair with a small product, and the degenerate rows and columns in full
PAIRS = sorted({(n, m) for n in SIZES for m in SIZES if n * m <= 1025 * 9 or n in (0, 1) or m in (0, 1)} |
               {(1000, 1000), (1025, 129), (129, 1025), (1025, 1025), (128, 128), (1000, 3)})
BATCHES = [(0, 5, 3), (9, 7, 3), (128, 3, 4), (1025, 2, 3)]
WIDE = [(1 << 15, 1), ((1 << 15) + 5, 5)]  # W > 1


def inputs(p, n, m, batch=1, seed=0):
    """coefficients and points with every 5th / 3rd stored unreduced (the largest x + k p below 2^256), the point 0 and a repeated point"""
    coefs = vec(p, 7000 + seed + 13 * n + m, batch * n, 5)
    xs = vec(p, 8000 + seed + n + 17 * m, m, 3)
    if m > 2:
        xs[1] = 0
        xs[2] = xs[0]
    return coefs, xs
