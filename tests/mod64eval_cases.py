"""What the host and GPU tests of sh_mod64_poly_eval share: the exact statement, shape and rule formulas and grids of
tests/modeval_cases.py and the word packing and modulus table of tests/mod64poly_cases.py, all as they are, plus the constants of the
packed path (starks_amd/csrc/mod64eval_items.cuh) and the shapes at the edges of a point group.  A word input is any 64-bit value and
stands for its residue; an output word is canonical."""
import random

from modeval_cases import BATCHES, PAIRS, WIDE, direct_preferred, direct_shape, evaluate, inputs, max_transform  # noqa: F401
from mod64poly_cases import BIG, FIELDS, IDS, P63, lifted, unwords, words  # noqa: F401
from modpoly_cases import BABYBEAR, GOLDILOCKS, KOALABEAR, two_adic_root  # noqa: F401

M6E_GROUP = 4                                  # points per lane of the direct path (mod64eval_items.cuh: M6E_GROUP)
M6E_COST = (9.9e5, 67.0, 185.0, 1.14e4, 0.0)   # mod64eval_items.cuh: M6E_COST, the five constants in PeCost's order
# m = G - 1 runs one point per lane, G and G + 1 one full group and a group of one, 2 G + 1 two full groups and one point; n around one
# workgroup's 256 lanes
GROUP_MS = [M6E_GROUP - 1, M6E_GROUP, M6E_GROUP + 1, 2 * M6E_GROUP + 1]
GROUP_SHAPES = [(n, m) for n in (255, 256, 257) for m in GROUP_MS]
MAX_ROOT_LOG = 28


def admits(p, n, m):
    """the tree path fits the field: its largest transform against the order of two_adic_root(p)"""
    return max_transform(n, m) <= 1 << min(FIELDS[p], 26)


def word_inputs(p, n, m, batch=1, seed=0):
    """modeval_cases.inputs as words: every 5th coefficient and 3rd point stored unreduced where a word admits it (v + k p below 2^64),
    the point 0 and a repeated point"""
    coefs, xs = inputs(p, n, m, batch, seed)
    rnd = random.Random(91 * n + m + seed)

    def lift(vals, every):
        out = [v % p for v in vals]
        for i in range(0, len(out), every):
            kmax = (2**64 - 1 - out[i]) // p
            if kmax:
                out[i] += p * rnd.randint(1, kmax)
        return out
    return lift(coefs, 5), lift(xs, 3)
