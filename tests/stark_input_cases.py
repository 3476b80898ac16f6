"""Inputs of the STARK prover and the STARK batch verifier that a valid, canonical witness never produces (pure Python, no GPU):

A. lazily reduced limbs.  include/starkhip.h allows any representative in [0, 2^256) in every sh_dev_* buffer and wire inputs >= p.  Only
   the residues below R = 2^256 - p = 351 * 2^32 - 1 have a second representative x + p, so the systems here keep some columns below R at
   every step (constants, a counter) beside columns that grow large, and PATTERNS says which of those elements are stored as x + p.  The
   expected proof of a unit is the oracle's proof of the RESIDUES (oracle/fastoracle.py), whatever the pattern.
B. witnesses that are not valid traces.  witness_grid(W) breaks one element per unit -- every column, every step, four kinds -- of the
   width-W system of tests/golden/stark_variants.json; the expected flag of a unit is the exact predicate violated() on Python ints.

Shared by tests/test_stark_inputs_host.py (CPU: the grids hold what they claim, the oracle does not see representatives, the fixture's
small entries are regenerated), tests/test_gpu_stark_inputs.py (GPU) and tests/golden/generate_stark_inputs.py."""
import hashlib
import json
import os
import random

import stark_variants as sv

P = sv.P
R = 2**256 - P  # x < R  <=>  x + P < 2^256: the residues with two representatives
assert R == 351 * 2**32 - 1
FIXTURE = os.path.join(sv.ROOT, "tests", "golden", "stark_inputs.json")

OK, CONSTRAINT, REJECTED = 0, -8, -9


def wire(vals):
    """32-byte big-endian, NOT reduced (the values may be >= p)."""
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def limbs(vals):
    """limb form as sh_dev_upload takes it: 8 x u32 little-endian = the 32 bytes little-endian, not reduced."""
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def flat(nested):
    """[unit][column][step] (a witness) or [unit][column] (inputs, outputs) -> one list in memory order."""
    out = []
    for x in nested:
        if isinstance(x, (list, tuple)):
            out.extend(flat(x))
        else:
            out.append(x)
    return out


# ---- A. the systems ------------------------------------------------------------------------------------------------------------------
COUNTER_1 = [{(1,): 1, (0,): 1}]                                                  # X' = X + 1
CONST_CUBE_2 = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]                              # X1' = X1 (= r), X2' = X2^3 + X1
COUNTER_MUL_2 = [{(1, 0): 1, (0, 0): 1}, {(1, 1): 1}]                             # X1' = X1 + 1, X2' = X2 X1
COUNTER_CUBE_2 = [{(1, 0): 1, (0, 0): 1}, {(1, 0): 1, (0, 3): 1}]                 # X1' = X1 + 1, X2' = X2^3 + X1
MIXED_3 = [{(1, 0, 0): 1, (0, 0, 0): 1}, {(1, 1, 0): 1}, {(1, 0, 0): 1, (0, 0, 3): 1}]  # X1' = X1 + 1, X2' = X2 X1, X3' = X3^3 + X1
CONST_3 = [{(1, 0, 0): 1}, {(0, 1, 0): 1}, {(1, 0, 0): 1, (0, 1, 0): 1, (0, 0, 3): 1}]  # two constants, X3' = X3^3 + X1 + X2
ZERO_1 = [{(3,): 1}]                                                              # X' = X^3 from 0: the all-zero system

PATTERNS = ("canonical", "all", "row0_inputs", "last_row", "single_mid", "one_per_64", "random_half")


def _s(seed, i):
    return sv.seeded(seed, i)


def _g1(steps):
    return pow(7, (P - 1) // steps, P)


def repr_cases():
    """The representative-invariance cases: name, step polynomials, shape, one input row per unit (distinct), patterns to apply."""
    cases = [
        dict(name="w1_counter", sp=COUNTER_1, steps=64, ext=4, inputs=[[0], [1], [R - 64], [2**32 + 5]]),
        dict(name="w2_const_cube", sp=CONST_CUBE_2, steps=32, ext=8, inputs=[[0, _s(1, 0)], [1, _s(1, 1)], [R - 1, _s(1, 2)]]),
        dict(name="w2_counter_mul", sp=COUNTER_MUL_2, steps=64, ext=4,
             inputs=[[1, _s(2, 0)], [1001, _s(2, 1)], [R - 64, _s(2, 2)], [2**40, _s(2, 3)], [0, _s(2, 4)]]),
        dict(name="w3_mixed", sp=MIXED_3, steps=16, ext=8,
             inputs=[[7, _s(3, 0), _s(3, 1)], [R - 16, _s(3, 2), _s(3, 3)], [0, _s(3, 4), _s(3, 5)]]),
        dict(name="w3_const", sp=CONST_3, steps=64, ext=4,
             inputs=[[0, 1, _s(4, 0)], [1, R - 1, _s(4, 1)], [R - 1, 0, _s(4, 2)], [R - 1, R - 1, _s(4, 3)], [1, 1, _s(4, 4)]]),
        # X' = X^3 from 0: P = D = B = 0; stored as 0 ("canonical"), as p ("all") and mixed (the other patterns)
        dict(name="w1_all_zero", sp=ZERO_1, steps=16, ext=4, inputs=[[0], [0], [0]]),
        # X' = g1 X: the trace polynomial is P = x0 X, of degree 1, its own boundary interpolant, so B = 0 identically.  The values
        # are large: nothing here has a second representative, the case runs canonical only
        dict(name="w1_linear_b_zero", sp=[{(1,): _g1(16)}], steps=16, ext=4, inputs=[[3], [_s(5, 0)], [1]], patterns=("canonical",)),
    ]
    for c in cases:
        c["width"] = len(c["sp"])
        c["batch"] = len(c["inputs"])
        c.setdefault("patterns", PATTERNS)
    return cases


def traces(case):
    return [sv.trace(inp, case["steps"], case["sp"]) for inp in case["inputs"]]


def eligible(tr):
    """[(unit, column, step)] of the witness elements that may be stored as x + p, in memory order."""
    return [(u, c, k) for u, unit in enumerate(tr) for c, col in enumerate(unit) for k, v in enumerate(col) if v < R]


def selection(case, tr, pattern):
    """-> (set of (unit, column, step) stored as x + p, set of (unit, column) inputs given as x + p)."""
    steps, width = case["steps"], case["width"]
    el = eligible(tr)
    el_in = [(u, c) for u, inp in enumerate(case["inputs"]) for c, v in enumerate(inp) if v % P < R]
    if pattern == "canonical":
        return set(), set()
    if pattern == "all":
        return set(el), set(el_in)
    if pattern == "row0_inputs":
        return {e for e in el if e[2] == 0}, set(el_in)
    if pattern == "last_row":  # witness[c][-1] is the `out` of the boundary interpolant
        return {e for e in el if e[2] == steps - 1}, set()
    if pattern == "single_mid":
        mid = [e for e in el if e[0] == min(1, case["batch"] - 1) and e[2] == steps // 2]
        return set(mid[:1]), set()
    if pattern == "one_per_64":  # one unreduced element in every run of 64 consecutive elements that has an eligible one: mixed waves
        pick = {}
        for e in el:
            idx = (e[0] * width + e[1]) * steps + e[2]
            blk = idx // 64
            want = (blk * 37 + 11) % 64  # the lane differs from block to block
            if blk not in pick or abs(idx % 64 - want) < abs(pick[blk][0] % 64 - want):
                pick[blk] = (idx, e)
        return {e for _, e in pick.values()}, set()
    if pattern == "random_half":
        rng = random.Random(case["name"])
        return {e for e in el if rng.random() < 0.5}, {e for e in el_in if rng.random() < 0.5}
    raise ValueError(pattern)


def stored(case, tr, pattern):
    """-> (witness [unit][column][step], inputs [unit][column]) as the ints to store: residue, or residue + p where selected."""
    sel, sel_in = selection(case, tr, pattern)
    wit = [[[v + P if (u, c, k) in sel else v for k, v in enumerate(col)] for c, col in enumerate(unit)] for u, unit in enumerate(tr)]
    ins = [[v % P + P if (u, c) in sel_in else v % P for c, v in enumerate(inp)] for u, inp in enumerate(case["inputs"])]
    return wit, ins


def oracle_unit(witness, inputs, sp, steps, ext):
    """The flat proof bytes of one unit from the O(n log n) oracle."""
    from oracle import fastoracle, pyoracle
    return pyoracle.stark_flat(fastoracle.mk_stark_proof_fast(witness, inputs, sp, steps, ext))


def pack_terms_raw(sp_raw, width):
    """[[(exponents, coefficient)]] -> (term_coefs, term_exps, term_counts list) with every coefficient written AS GIVEN (below 2^256,
    possibly >= p) and the terms in the order given: what starks_amd.stark.pack_step_polys would reduce."""
    coefs, exps, counts = b"", b"", []
    for terms in sp_raw:
        counts.append(len(terms))
        for ex, cf in terms:
            assert len(ex) == width and 0 <= cf < 2**256
            coefs += cf.to_bytes(32, "big")
            exps += bytes(ex)
    return coefs, exps, counts


# coefficients as the prover's term upload may meet them: 1 written as 1 + p (the coefficient-is-one flag), a term whose coefficient
# is p (a zero term), c written as c + p.  Terms in sorted monomial order, as pack_step_polys orders them.
COEF_CASE = dict(
    name="w2_unreduced_coefficients", width=2, steps=32, ext=8, inputs=[[3, _s(6, 0)], [R - 1 + P, _s(6, 1)], [0, 5]],
    raw=[[((1, 0), 1 + P), ((2, 0), P)], [((0, 3), 5 + P), ((1, 0), 1 + P), ((1, 1), P)]],
    residues=[{(1, 0): 1, (2, 0): 0}, {(0, 3): 5, (1, 0): 1, (1, 1): 0}],
    without_zero_terms=[{(1, 0): 1}, {(0, 3): 5, (1, 0): 1}])


# ---- A. one width-2 and one width-3 case per quotient / lincomb regime ------------------------------------------------------------
def regime_cases():
    """narrow / middle / wide launches of the quotient and lincomb kernels (tests/stark_variants.regimes), each just large enough:
    middle = one proof above the two-lane threshold, wide = exactly STARK_WIDE_THREADS rows.  Column 0 is a counter from a small
    start, so the whole column may be stored as x + p.  The units' SHA-256 are in tests/golden/stark_inputs.json."""
    out = []
    for width, sp in ((2, COUNTER_CUBE_2), (3, MIXED_3)):
        for regime, steps, ext, batch in (("narrow", 64, 8, 3), ("middle", 1 << 12, 8, 17), ("wide", 1 << 12, 8, 64)):
            out.append(dict(name="w%d_%s" % (width, regime), regime=regime, width=width, sp=sp, steps=steps, ext=ext, batch=batch,
                            seed=7000 + width))
    return out


def regime_inputs(case, unit):
    w = case["width"]
    return [1 + 3 * unit] + [_s(case["seed"], unit * w + j) for j in range(1, w)]


# ---- B. the witness check -------------------------------------------------------------------------------------------------------------
def step_row(row, sp):
    """step_c(row) for every c, by the term evaluation of stark_variants.trace."""
    return [col[1] for col in sv.trace(row, 2, sp)]


def violated(w, sp):
    """The prover's contract on Python ints: some k in [0, steps - 2] and some c with w[c][k + 1] != step_c(w[.][k]) mod p.  The wrap
    transition (last -> 0) is not a constraint."""
    steps = len(w[0])
    for k in range(steps - 1):
        nxt = step_row([col[k] for col in w], sp)
        if any((w[c][k + 1] - nxt[c]) % P for c in range(len(w))):
            return True
    return False


GRID_STEPS = 8
KINDS = ("plus_1", "minus_1", "zero", "plus_p")


def _first_variant_case(width):
    with open(os.path.join(sv.ROOT, "tests", "golden", "stark_variants.json")) as fh:
        return [c for c in json.load(fh)["cases"] if c["width"] == width][0]


def witness_grid(width):
    """One batch for width W: the step polynomials and the extension factor of that width's first case of stark_variants.json, 8 steps
    (every such system passes stark_check_shape at 8 steps), one unit per (column, step, kind) with distinct small inputs per unit (so
    row 0 has a second representative), and an untouched unit in front, after every 16 and at the end.
    -> dict(width, steps, ext, sp, units=[dict(kind, c, k, inputs, residues, witness, bad)])."""
    vc = _first_variant_case(width)
    sp, ext, steps = sv.step_polys(vc), vc["ext"], GRID_STEPS
    units = []

    def add(kind, c, k):
        u = len(units)
        inputs = [2 + u * width + j for j in range(width)]
        w = sv.trace(inputs, steps, sp)
        if kind == "plus_1":
            w[c][k] = (w[c][k] + 1) % P
        elif kind == "minus_1":
            w[c][k] = (w[c][k] - 1) % P
        elif kind == "zero":
            if w[c][k] == 0:
                return
            w[c][k] = 0
        elif kind == "plus_p":
            if w[c][k] >= R:
                return
        res = [list(col) for col in w]
        if kind == "plus_p":
            w[c][k] += P
        units.append(dict(kind=kind, c=c, k=k, inputs=inputs, residues=res, witness=w, bad=violated(res, sp)))

    add("untouched", None, None)
    n = 0
    for c in range(width):
        for k in range(steps):
            for kind in KINDS:
                before = len(units)
                add(kind, c, k)
                n += len(units) - before
                if len(units) > before and n % 16 == 0:
                    add("untouched", None, None)
    add("untouched", None, None)
    return dict(name="grid_w%d" % width, width=width, steps=steps, ext=ext, sp=sp, units=units)


# all-periodic system: X1' = 3, X2' = X2.  From (3, 5) every transition holds, the wrap included; with witness[0][0] = 4 (and input 4)
# only the wrap transition last -> 0 of column 0 is broken, which is no constraint: a valid trace (nothing reads X1)
WRAP_SP = [{(0, 0): 3}, {(0, 1): 1}]
WRAP_CASE = dict(name="wrap_only", width=2, steps=16, ext=4, sp=WRAP_SP, inputs=[[3, 5], [4, 5], [3, 6]])

# the flat-index arithmetic of the check at size: 2^12 steps, width 2, batch 3; transition 0 broken in unit 0, transition steps - 2 in
# unit 2, unit 1 valid (its proof's SHA-256 is in the fixture)
SIZE_CASE = dict(name="size_2^12", width=2, steps=1 << 12, ext=8, sp=CONST_CUBE_2, inputs=[[42, 3], [43, 4], [44, 5]])


def size_case_units():
    c = SIZE_CASE
    ws = [sv.trace(inp, c["steps"], c["sp"]) for inp in c["inputs"]]
    ws[0][1][0] = (ws[0][1][0] + 1) % P                      # read by step_1 at k = 0 only
    ws[2][1][c["steps"] - 1] = (ws[2][1][c["steps"] - 1] + 1) % P  # the left side of transition steps - 2 only
    return ws


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def sha(b):
    return hashlib.sha256(b).hexdigest()


def regime_entry(case, units=None):
    """The fixture entry of a regime case: per-unit SHA-256 of the oracle's proof (of `units`, default all)."""
    out = []
    for u in (range(case["batch"]) if units is None else units):
        inp = regime_inputs(case, u)
        out.append(sha(oracle_unit(sv.trace(inp, case["steps"], case["sp"]), inp, case["sp"], case["steps"], case["ext"])))
    return out


def size_entry():
    c = SIZE_CASE
    return sha(oracle_unit(sv.trace(c["inputs"][1], c["steps"], c["sp"]), c["inputs"][1], c["sp"], c["steps"], c["ext"]))


def load_fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)
