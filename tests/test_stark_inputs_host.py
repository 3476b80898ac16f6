"""CPU half of the STARK input harness (tests/stark_input_cases.py): the case grids hold every pattern, width, column and both flag
outcomes they claim to hold; the oracle gives the proof of the residues whatever representative it is handed; the committed hashes
(tests/golden/stark_inputs.json) are regenerated -- the small entries whole, the large ones one unit each."""
import pytest

import stark_input_cases as sc
import stark_variants as sv

P, R = sc.P, sc.R

_expected = {}


def expected(case):
    """The oracle's proof of every unit's residues, once per case."""
    if case["name"] not in _expected:
        tr = sc.traces(case)
        _expected[case["name"]] = [sc.oracle_unit(tr[u], case["inputs"][u], case["sp"], case["steps"], case["ext"])
                                   for u in range(case["batch"])]
    return _expected[case["name"]]


def test_two_representatives_exist_exactly_below_r():
    assert R - 1 + P == 2**256 - 1 and R + P == 2**256
    assert sc.wire([2**256 - 1]) == b"\xff" * 32 and sc.limbs([1 + P])[:4] == ((1 + P) & 0xffffffff).to_bytes(4, "little")
    assert sc.limbs([5])[::-1] == sc.wire([5])


def test_representative_cases_hold_every_system_shape_and_pattern():
    cases = sc.repr_cases()
    full = [c for c in cases if c["patterns"] == sc.PATTERNS]
    assert {c["width"] for c in full} == {1, 2, 3}
    assert set(sc.PATTERNS) == {"canonical", "all", "row0_inputs", "last_row", "single_mid", "one_per_64", "random_half"}
    consts = set()
    top = False
    for c in cases:
        assert 16 <= c["steps"] <= 64 and c["ext"] in (4, 8) and 3 <= c["batch"] <= 5, c["name"]
        degree = max(sum(k) for d in c["sp"] for k in d)
        assert degree >= 1 and degree * (c["steps"] - 1) + 1 < c["steps"] * c["ext"]
        tr = sc.traces(c)
        assert all(not sc.violated(w, c["sp"]) for w in tr)
        assert all([col[0] for col in w] == [v % P for v in inp] for w, inp in zip(tr, c["inputs"]))
        if c["name"] != "w1_all_zero":
            assert len({tuple(i) for i in c["inputs"]}) == c["batch"], "units must differ"
        for j, poly in enumerate(c["sp"]):  # constant columns X_j' = X_j
            if poly == {tuple(1 if v == j else 0 for v in range(c["width"])): 1} and c["width"] > 1:
                consts |= {inp[j] for inp in c["inputs"]}
        for pattern in c["patterns"]:
            sel, sel_in = sc.selection(c, tr, pattern)
            wit, ins = sc.stored(c, tr, pattern)
            assert all(tr[u][col][k] < R for u, col, k in sel) and all(c["inputs"][u][col] % P < R for u, col in sel_in)
            assert all(0 <= v < 2**256 for v in sc.flat(wit)) and all(0 <= v < 2**256 for i in ins for v in i)
            assert [[[v % P for v in col] for col in w] for w in wit] == tr
            assert sum(v >= P for v in sc.flat(wit)) == len(sel)
            top = top or 2**256 - 1 in sc.flat(wit)
            if c["patterns"] == sc.PATTERNS and pattern != "canonical":
                assert sel, (c["name"], pattern)
            if pattern == "all":
                assert sel == set(sc.eligible(tr)) and len(sel) >= c["batch"] * c["steps"]  # at least one whole column per unit
            if pattern == "row0_inputs":
                assert {k for _, _, k in sel} == {0} and sel_in
            if pattern == "last_row":
                assert {k for _, _, k in sel} == {c["steps"] - 1} and not sel_in
            if pattern == "single_mid":
                assert len(sel) == 1 and 0 < list(sel)[0][2] < c["steps"] - 1
            if pattern == "one_per_64":
                blocks = [((u * c["width"] + col) * c["steps"] + k) // 64 for u, col, k in sel]
                assert len(blocks) == len(set(blocks)) == len({((u * c["width"] + col) * c["steps"] + k) // 64
                                                               for u, col, k in sc.eligible(tr)})
            if pattern == "random_half":
                assert len(sc.eligible(tr)) // 4 < len(sel) < 3 * len(sc.eligible(tr)) // 4 + 1
    assert {0, 1, R - 1} <= consts
    assert top, "no element is stored as 2^256 - 1"
    zero, = [c for c in cases if c["name"] == "w1_all_zero"]
    assert set(sc.flat(sc.traces(zero))) == {0}
    assert set(sc.flat(sc.stored(zero, sc.traces(zero), "all")[0])) == {P}
    assert set(sc.flat(sc.stored(zero, sc.traces(zero), "random_half")[0])) == {0, P}
    lin, = [c for c in cases if c["name"] == "w1_linear_b_zero"]
    g1 = pow(7, (P - 1) // lin["steps"], P)
    assert lin["sp"] == [{(1,): g1}] and pow(g1, lin["steps"], P) == 1 and pow(g1, lin["steps"] // 2, P) != 1
    assert all(w[0][k] == inp[0] * pow(g1, k, P) % P for w, inp in zip(sc.traces(lin), lin["inputs"]) for k in range(lin["steps"]))


@pytest.mark.parametrize("case", sc.repr_cases(), ids=lambda c: c["name"])
def test_oracle_proves_the_residues_whatever_the_representative(case):
    want = expected(case)
    tr = sc.traces(case)
    assert len({w for w in want}) == (1 if case["name"] == "w1_all_zero" else case["batch"])
    for pattern in case["patterns"]:
        wit, ins = sc.stored(case, tr, pattern)
        for u in range(case["batch"]):
            assert sc.oracle_unit(wit[u], ins[u], case["sp"], case["steps"], case["ext"]) == want[u], (case["name"], pattern, u)


def test_unreduced_coefficients_are_the_residues_system():
    c = sc.COEF_CASE
    raw = [dict(t) for t in c["raw"]]
    assert [{k: v % P for k, v in d.items()} for d in raw] == c["residues"]
    assert all(v >= P for d in raw for v in d.values())
    vals = [v for d in raw for v in d.values()]
    assert 1 + P in vals and P in vals and any(v % P > 1 for v in vals)
    assert [sorted(d) for d in raw] == [[k for k, _ in t] for t in c["raw"]], "terms are in sorted monomial order"
    coefs, exps, counts = sc.pack_terms_raw(c["raw"], c["width"])
    assert counts == [2, 3] and len(coefs) == 32 * 5 and exps == bytes([1, 0, 2, 0, 0, 3, 1, 0, 1, 1])
    assert int.from_bytes(coefs[:32], "big") == 1 + P
    assert any(v >= P for inp in c["inputs"] for v in inp)
    for inp in c["inputs"]:
        tr = sv.trace(inp, c["steps"], c["residues"])
        want = sc.oracle_unit(tr, inp, c["residues"], c["steps"], c["ext"])
        assert sv.trace(inp, c["steps"], raw) == tr == sv.trace(inp, c["steps"], c["without_zero_terms"])
        assert sc.oracle_unit(tr, inp, raw, c["steps"], c["ext"]) == want
        assert sc.oracle_unit(tr, inp, c["without_zero_terms"], c["steps"], c["ext"]) == want


def test_regime_cases_reach_each_regime_with_the_smallest_batch():
    th = sv.thresholds()
    cases = sc.regime_cases()
    assert sorted((c["width"], c["regime"]) for c in cases) == sorted((w, r) for w in (2, 3) for r in ("narrow", "middle", "wide"))
    for c in cases:
        (q, w), (lc, lw) = sv.regimes(c, th)
        assert q == lc == c["regime"] and w == c["width"] and lw == (2 if w == 2 else 0), c["name"]
        if c["regime"] != "narrow":  # one proof fewer is a smaller regime: the batch is just large enough
            (q1, _), (lc1, _) = sv.regimes(dict(c, batch=c["batch"] - 1), th)
            assert q1 != c["regime"] or lc1 != c["regime"], c["name"]
        degree = max(sum(k) for d in c["sp"] for k in d)
        assert degree * (c["steps"] - 1) + 1 < c["steps"] * c["ext"] and c["steps"] * c["ext"] < 2**24
        ins = [sc.regime_inputs(c, u) for u in range(c["batch"])]
        assert len({tuple(i) for i in ins}) == c["batch"]
        assert all(i[0] + c["steps"] < R for i in ins), "column 0, a counter, stays below 2^256 - p"
        assert c["sp"][0] == {tuple(1 if v == 0 else 0 for v in range(w)): 1, (0,) * w: 1}
    assert any(sv.rows(c) >= 1 << 19 for c in cases)


def test_fixture_matches_the_cases_and_its_small_entries_regenerate():
    fx = sc.load_fixture()
    cases = {c["name"]: c for c in sc.regime_cases()}
    assert [r["name"] for r in fx["regimes"]] == list(cases)
    for r in fx["regimes"]:
        c = cases[r["name"]]
        assert (r["width"], r["steps"], r["ext"], r["batch"], r["seed"]) == (c["width"], c["steps"], c["ext"], c["batch"], c["seed"])
        assert len(r["unit_sha256"]) == len(set(r["unit_sha256"])) == c["batch"]
        assert all(len(h) == 64 for h in r["unit_sha256"])
        if c["regime"] == "narrow":
            assert sc.regime_entry(c) == r["unit_sha256"], r["name"]
        elif c["regime"] == "middle":
            last = c["batch"] - 1
            assert sc.regime_entry(c, [last]) == r["unit_sha256"][last:], r["name"]
    s = fx["size_case"]
    assert (s["name"], s["width"], s["steps"], s["ext"]) == tuple(sc.SIZE_CASE[k] for k in ("name", "width", "steps", "ext"))
    assert sc.size_entry() == s["unit1_sha256"]


@pytest.mark.parametrize("width", list(range(1, 10)))
def test_witness_grid_is_complete_and_its_flags_are_the_predicate(width):
    g = sc.witness_grid(width)
    sp, steps, units = g["sp"], g["steps"], g["units"]
    vc = sc._first_variant_case(width)
    assert sp == sv.step_polys(vc) and g["ext"] == vc["ext"] and steps == 8 and len(units) <= 256
    degree = max(sum(k) for d in sp for k in d)
    assert degree * (steps - 1) + 1 < steps * g["ext"]
    assert all(any(k[v] for d in sp for k in d) for v in range(width)), "every column is read by some polynomial"
    assert len({tuple(u["inputs"]) for u in units}) == len(units)
    seen = {}
    for i, u in enumerate(units):
        base = sv.trace(u["inputs"], steps, sp)
        assert not sc.violated(base, sp)
        assert [[v % P for v in col] for col in u["witness"]] == u["residues"]
        assert all(0 <= v < 2**256 for col in u["witness"] for v in col)
        assert u["bad"] == sc.violated(u["residues"], sp) == sc.violated(u["witness"], sp)
        if u["kind"] == "untouched":
            assert u["witness"] == base and not u["bad"]
            continue
        c, k = u["c"], u["k"]
        diff = [(cc, kk) for cc in range(width) for kk in range(steps) if u["witness"][cc][kk] != base[cc][kk]]
        assert diff == [(c, k)], "exactly one element differs"
        seen.setdefault((c, k), set()).add(u["kind"])
        if u["kind"] == "plus_p":
            assert u["witness"][c][k] == base[c][k] + P and u["residues"] == base and not u["bad"]
        else:
            want = {"plus_1": (base[c][k] + 1) % P, "minus_1": (base[c][k] - 1) % P, "zero": 0}[u["kind"]]
            assert u["witness"][c][k] == want != base[c][k]
            if k >= 1:
                assert u["bad"], "a changed residue at k >= 1 breaks transition k - 1"
            else:  # k = 0: only transition 0 -> 1 reads it; the wrap last -> 0 is no constraint
                nxt = sc.step_row([col[0] for col in u["residues"]], sp)
                assert u["bad"] == any((base[cc][1] - nxt[cc]) % P for cc in range(width))
    # no case is left out: every column and step has +1 and -1, `zero` unless the value is 0, `plus_p` wherever the residue allows
    for c in range(width):
        for k in range(steps):
            assert {"plus_1", "minus_1"} <= seen[(c, k)]
        assert "plus_p" in seen[(c, 0)], "row 0 is small by construction"
        outcomes = {u["bad"] for u in units if u["c"] == c}
        assert outcomes == {True, False}, "both flag outcomes for column %d" % c
    n_zero = sum("zero" in s for s in seen.values())
    assert n_zero >= width * steps - 2
    # untouched units in front, at the end and spread between: no 20 consecutive units without a valid one
    assert units[0]["kind"] == units[-1]["kind"] == "untouched"
    valid = [i for i, u in enumerate(units) if not u["bad"]]
    assert max(b - a for a, b in zip(valid, valid[1:])) <= 20
    assert sum(u["kind"] == "untouched" for u in units) >= 3
    # a 256-thread workgroup of the check (one thread per step) holds 32 units
    assert 256 // steps < len(units) or width == 1


def test_wrap_and_size_cases_break_what_they_say():
    c = sc.WRAP_CASE
    tr = sc.traces(c)
    assert tr[0] == [[3] * c["steps"], [5] * c["steps"]], "periodic: the wrap transition holds too"
    assert tr[1][0] == [4] + [3] * (c["steps"] - 1) and tr[1][1] == tr[0][1]
    assert not any(sc.violated(w, c["sp"]) for w in tr)
    last = [col[-1] for col in tr[1]]
    assert sc.step_row(last, c["sp"])[0] != tr[1][0][0], "only the wrap transition of column 0 is broken"
    s = sc.SIZE_CASE
    ws = sc.size_case_units()
    base = sc.traces(s)
    assert [sc.violated(w, s["sp"]) for w in ws] == [True, False, True]
    steps = s["steps"]

    def broken(w):
        return [k for k in range(steps - 1) if any((w[cc][k + 1] - n) % P for cc, n in enumerate(sc.step_row([col[k] for col in w], s["sp"])))]
    assert broken(ws[0]) == [0] and broken(ws[2]) == [steps - 2] and ws[1] == base[1]
