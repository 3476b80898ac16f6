"""The write-footprint audit's CPU half (footprint_cases.py): the checker on synthetic images -- it flags a flipped first or last
guard byte, a changed read-only byte, one output byte left at its prefill, a pattern copied from one guard into another, and passes
a clean image --, and the table against include/starkhip.h: every sh_dev_* name has a row or a reasoned exemption, every pointer
argument of every prototype has a role, every output length is an expression of the shape."""
import ast
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint_cases as fc  # noqa: E402

BUFS = [("d_in", "in", 1000), ("d_out", "out", 777), ("d_q", "out", 0), ("d_io", "inout", 256)]
DATA = {"d_in": bytes(range(250)) * 4, "d_io": b"\x11" * 256}


def _run(layout, seed, result=b"\xc3"):
    """(before, after) of a well-behaved call: every output byte written with the same result whatever the prefill"""
    before = layout.image(seed, DATA)
    after = bytearray(before)
    for r in layout.regions:
        if r.role in ("out", "inout"):
            after[r.off:r.end] = result * r.nbytes
    return before, after


@pytest.fixture(scope="module")
def lay():
    return fc.Layout(BUFS)


def test_layout_and_pattern(lay):
    assert [r.off % fc.ALIGN for r in lay.regions] == [0] * 4
    gs = list(lay.guards())
    assert len(gs) == 5 and all(hi - lo >= fc.GUARD for lo, hi in gs) and gs[0][0] == 0 and gs[-1][1] == lay.total
    assert lay["d_q"].nbytes == 0 and lay["d_q"].off - lay["d_out"].end >= fc.GUARD  # an empty output still lies between two guards
    a, b = fc.pattern(1, 1 << 16), fc.pattern(2, 1 << 16)
    assert all(x != y for x, y in zip(a, b)), "the prefills of the two runs differ in every byte"
    assert fc.pattern(1, 1 << 16) == a and a[:4096] != a[4096:8192] and len(set(a)) == 256
    assert fc.pattern(3, 64) != a[:64]


def test_clean_image_passes(lay):
    (b1, a1), (b2, a2) = _run(lay, 1), _run(lay, 2)
    assert fc.check(lay, b1, bytes(a1)) == [] and fc.check(lay, b2, bytes(a2)) == []
    assert fc.compare_runs(lay, bytes(a1), bytes(a2)) == []
    assert lay.outputs(bytes(a1)) == {"d_out": b"\xc3" * 777, "d_q": b"", "d_io": b"\xc3" * 256}


@pytest.mark.parametrize("k", range(5))
@pytest.mark.parametrize("edge", ["first", "last"])
def test_guard_flip(lay, k, edge):
    lo, hi = list(lay.guards())[k]
    at = lo if edge == "first" else hi - 1
    before, after = _run(lay, 1)
    after[at] ^= 1
    found = fc.check(lay, before, bytes(after))
    assert len(found) == 1 and found[0][0] == "guard" and found[0][2] == at
    # named by the payload the byte touches
    assert found[0][1] == (lay.regions[k] if (edge == "last" and k < 4) or k == 0 else lay.regions[k - 1]).name


def test_read_only_byte(lay):
    r = lay["d_in"]
    for at in (r.off, r.off + 500, r.end - 1):
        before, after = _run(lay, 1)
        after[at] ^= 0x80
        assert fc.check(lay, before, bytes(after)) == [("input", "d_in", at)]
    # an in/out payload is an output: overwriting it is no finding
    before, after = _run(lay, 1)
    assert before[lay["d_io"].off] != after[lay["d_io"].off] and fc.check(lay, before, bytes(after)) == []


@pytest.mark.parametrize("name", ["d_out", "d_io"])
def test_output_byte_left_at_prefill(lay, name):
    r = lay[name]
    for at in (r.off, r.off + r.nbytes // 2, r.end - 1):
        runs = []
        for seed in (1, 2):
            before, after = _run(lay, seed)
            if r.role == "out":  # an in/out payload holds the same input in both runs: only a prefilled byte can betray itself
                after[at] = before[at]
            else:
                after[at] = fc.pattern(seed, lay.total)[at]
            assert fc.check(lay, before, bytes(after)) == []
            runs.append(bytes(after))
        assert fc.compare_runs(lay, *runs) == [("differs", name, at)]


def test_pattern_copied_between_guards(lay):
    gs = list(lay.guards())
    before, after = _run(lay, 1)
    (s_lo, _), (d_lo, _) = gs[0], gs[2]
    after[d_lo + 64:d_lo + 64 + 4096] = before[s_lo + 64:s_lo + 64 + 4096]  # the same offset inside another guard
    found = fc.check(lay, before, bytes(after))
    assert [f[0] for f in found] == ["guard"] and d_lo + 64 <= found[0][2] < d_lo + 64 + 8
    before, after = _run(lay, 1)
    after[d_lo:d_lo + 4096] = before[d_lo + 1:d_lo + 4097]  # the guard's own pattern shifted by one byte
    assert [f[0] for f in fc.check(lay, before, bytes(after))] == ["guard"]


def test_result_depending_on_prefill_or_stale_bytes(lay):
    (_, a1), (_, a2) = _run(lay, 1), _run(lay, 2, result=b"\xc4")
    assert [f[:2] for f in fc.compare_runs(lay, bytes(a1), bytes(a2))] == [("differs", "d_out"), ("differs", "d_io")]


# ---- the table against the header ------------------------------------------------------------------------------------------------------
PROTOS = fc.header_prototypes()


def test_every_entry_has_a_row_or_an_exemption():
    assert len(PROTOS) >= 56 and "sh_dev_mod64_poly_eval" in PROTOS and "sh_dev_alloc" in PROTOS
    rows = {r.entry for r in fc.ROWS}
    missing = sorted(set(PROTOS) - rows - set(fc.EXEMPT))
    assert not missing, "sh_dev_* entries without a footprint row: %s" % missing
    assert sorted(fc.EXEMPT) == ["sh_dev_alloc", "sh_dev_free"] and all(len(v) > 20 for v in fc.EXEMPT.values())
    assert not rows & set(fc.EXEMPT) and rows <= set(PROTOS), "a row names an entry the header does not declare"
    assert len({r.id for r in fc.ROWS}) == len(fc.ROWS)


def test_removing_a_row_is_noticed(monkeypatch):
    for victim in ("sh_dev_mod64_to_limbs", "sh_dev_ntt"):
        monkeypatch.setattr(fc, "ROWS", [r for r in fc.ROWS if r.entry != victim])
        with pytest.raises(AssertionError, match=victim):
            test_every_entry_has_a_row_or_an_exemption()
        monkeypatch.undo()


def test_aliasing_forms_have_rows():
    ids = {r.id for r in fc.ROWS}
    for fam in ("sh_dev_", "sh_dev_mod_", "sh_dev_mod64_"):
        assert {fam + "ntt-inplace", fam + "multi_inv-inplace", fam + "multi_interp_4-over-d_xs", fam + "multi_interp_4-over-d_ys"} <= ids
    by = fc.by_id()
    for fam in ("sh_dev_", "sh_dev_mod_", "sh_dev_mod64_"):  # the resumed witness dispatches and the forced tree run under their knobs
        assert by[fam + "stark_witness-slice64"].env == {"STARKHIP_WITNESS_SLICE": "64"} and by[fam + "poly_eval-tree"].env
        assert {65, 300} <= {s["steps"] for s in by[fam + "stark_witness-slice64"].shapes}
    lde = next(r for r in fc.ROWS if r.entry == "sh_dev_lde")
    assert lde.roles["d_trace"] == "inout:32 * cols * steps"  # the documented overwrite is declared, not exempted


@pytest.mark.parametrize("r", fc.ROWS, ids=lambda r: r.id)
def test_row_consistency(r):
    assert set(r.roles) == set(PROTOS[r.entry]), "every pointer argument of the prototype has a role, and only those"
    assert r.shapes and r.cite and r.polluter in fc.POLLUTERS
    assert r.anchor == "all" or 0 <= r.anchor < len(r.shapes)
    family = "mod" if r.entry.startswith("sh_dev_mod") or r.entry == "sh_dev_merkelize_plain" else "mimc"
    assert not r.polluter.startswith(family + "_"), "the polluter is an entry of another family"
    outputs = 0
    for arg, role in r.roles.items():
        kind, _, expr = role.partition(":")
        if kind.startswith("="):
            assert r.roles[kind[1:]].startswith("inout:"), "an aliased output makes the argument it aliases in/out"
            outputs += 1
            continue
        assert kind in ("const", "in", "hin", "out", "hout", "inout") and bool(expr) == (kind in ("out", "hout", "inout")), (arg, role)
        if expr:
            outputs += 1
            names = {n.id for n in ast.walk(ast.parse(expr, mode="eval")) if isinstance(n, ast.Name)} - {"max", "min"}
            assert names, "%s: the length of %s is a constant, not an expression of the shape" % (r.id, arg)
            for s in r.shapes:
                assert names <= set(s) | {"proof_len"}, (r.id, arg, names, s)
                if "proof_len" not in names:
                    assert fc.out_len(expr, s) >= 0
    assert outputs, "a row without an output checks nothing"
    for s in r.shapes:  # no shape above what the existing GPU tests already run
        assert s.get("n", 0) <= (1 << 24) + 5 and s.get("batch", 1) <= 65 and s.get("steps", 0) * s.get("ext", 1) <= 1 << 13


def test_formula_lengths():
    dm = next(r for r in fc.ROWS if r.id == "sh_dev_mod64_poly_divmod")
    lens = [(fc.out_len(dm.roles["d_q"].split(":")[1], s), fc.out_len(dm.roles["d_r"].split(":")[1], s)) for s in dm.shapes]
    assert lens == [(0, 40), (72, 0), (8 * 257, 8 * 256), (8 * 401, 8 * 299)]  # (5, 9): no quotient, the dividend is its own remainder
    z = next(r for r in fc.ROWS if r.id == "sh_dev_zpoly")
    assert [fc.out_len(z.roles["d_out"].split(":")[1], s) for s in z.shapes][:2] == [32, 64]  # no points: [1]
