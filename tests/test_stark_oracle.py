"""CPU tests of the O(n log n) STARK oracle (oracle/fastoracle.py:mk_stark_proof_fast), which writes the at-size STARK fixtures:
byte for byte equal to the reference's own proofs (stark.json), to the quadratic coefficient-form prover (pyoracle.mk_stark_proof)
on random shapes, and to the committed stark_large.json proofs.  Also: the kernel variant matrix (stark_variants.json) covers every
kernel instance stark.hip can launch, as the kernel source defines the thresholds today."""
import hashlib
import os
import random
import subprocess
import sys

import pytest

from conftest import load_golden, ROOT
import stark_variants as sv

P = 2**256 - 2**32 * 351 + 1


@pytest.fixture(scope="module")
def oc():
    from oracle import fastoracle, pyoracle

    class NS:
        pass

    ns = NS()
    ns.fast, ns.py = fastoracle, pyoracle
    return ns


@pytest.mark.parametrize("c", load_golden("stark.json"), ids=lambda c: c["name"])
def test_fast_oracle_equals_the_reference_proofs(oc, c):
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    w = [[int(x, 16) for x in col] for col in c["witness"]]
    proof = oc.fast.mk_stark_proof_fast(w, c["inputs"], sp, c["steps"], c["ext"])
    flat = oc.py.stark_flat(proof)
    assert proof[0].hex() == c["m_root"] and proof[1].hex() == c["l_root"]
    assert [b.hex() for b in proof[2][0]] == c["branch0"]
    assert len(flat) == c["flat_len"] and hashlib.sha256(flat).hexdigest() == c["flat_sha"]


@pytest.mark.parametrize("logsteps", [12, 14])
def test_fast_oracle_equals_the_committed_large_proofs(oc, logsteps):
    """stark_large.json's 2^12 / 2^14-step proofs, written by the quadratic prover."""
    c, = [c for c in load_golden("stark_large.json")["cases"] if c["logsteps"] == logsteps]
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    w = oc.py.get_computational_trace(c["inputs"], c["steps"], sp)
    proof = oc.fast.mk_stark_proof_fast(w, c["inputs"], sp, c["steps"], c["ext"])
    flat = oc.py.stark_flat(proof)
    assert proof[0].hex() == c["m_root"] and proof[1].hex() == c["l_root"]
    assert len(flat) == c["proof_bytes"] and hashlib.sha256(flat).hexdigest() == c["proof_sha256"]


def _random_polys(rng, width, maxdeg):
    sp = []
    for j in range(width):
        terms = {}
        for t in range(rng.randint(1, 4)):
            ex = [0] * width
            for _ in range(rng.randint(0 if t else 1, maxdeg)):
                ex[rng.randrange(width)] += 1
            terms[tuple(ex)] = rng.choice([1, 2, P - 1, rng.randrange(1, P)])
        sp.append(terms)
    sp[0][(0,) * width] = P - 1                        # a constant term
    if width <= maxdeg:
        sp[-1][(1,) * width] = rng.choice([1, P - 1])  # a term touching every variable
    return sp


# widths 1..9, ext 2..32, steps 2..256, and the tiny-trace shapes of test_gpu_parity.py::test_stark_extension_factors_and_tiny_traces
SHAPES = [(1, 2, 8), (2, 4, 8), (1, 2, 2), (2, 8, 2), (2, 16, 4), (3, 8, 16), (1, 4, 32), (1, 128, 8), (2, 256, 4),
          (4, 32, 4), (5, 16, 8), (6, 8, 16), (7, 4, 32), (8, 16, 16), (9, 8, 16), (3, 64, 4), (2, 256, 2), (9, 2, 32)]


@pytest.mark.parametrize("width,steps,ext", SHAPES, ids=lambda v: str(v))
def test_fast_oracle_equals_the_coefficient_form_prover(oc, width, steps, ext):
    rng = random.Random(width * 100003 + steps * 101 + ext)
    maxdeg = max(1, min(width + 1, (steps * ext - 2) // (steps - 1)))
    for _ in range(20):
        sp = _random_polys(rng, width, maxdeg)
        degree = max(oc.py.mv_degree(q) for q in sp)
        if degree >= 1 and degree * (steps - 1) + 1 < steps * ext:
            break
    else:
        pytest.fail("no admissible step polynomials drawn")
    inputs = [rng.choice([0, 1, P - 1, rng.randrange(P)]) for _ in range(width)]
    w = oc.py.get_computational_trace(inputs, steps, sp)
    want = oc.py.stark_flat(oc.py.mk_stark_proof(w, inputs, sp, steps, ext))
    assert oc.py.stark_flat(oc.fast.mk_stark_proof_fast(w, inputs, sp, steps, ext)) == want, (width, steps, ext, sp)


def test_fast_oracle_rejects_an_invalid_trace(oc):
    sp = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]
    w = oc.py.get_computational_trace([2, 5], 16, sp)
    w[1][7] = (w[1][7] + 1) % P
    with pytest.raises(AssertionError):
        oc.fast.mk_stark_proof_fast(w, [2, 5], sp, 16, 8)


def test_fast_oracle_imports_nothing_from_the_product():
    code = ("import sys; from oracle import fastoracle; "
            "bad = [m for m in sys.modules if m.split('.')[0] == 'starks_amd']; assert not bad, bad")
    subprocess.check_call([sys.executable, "-c", code], cwd=ROOT)


def test_variant_trace_helper_equals_pyoracle(oc):
    for c in load_golden("stark_variants.json")["cases"][::4]:
        sp = sv.step_polys(c)
        inp = sv.unit_inputs(c, c["batch"] - 1)
        assert sv.trace(inp, 16, sp) == oc.py.get_computational_trace(inp, 16, sp), c["name"]


def test_variant_matrix_covers_every_kernel_cell():
    """Every kernel instance stark.hip launches -- the quotient kernel for W = 1..9 and the lincomb kernel for W = 1, 2 and generic,
    each narrow, middle and WIDE, and the band where the quotients are narrow and the lincomb middle -- has a case, with the thresholds
    read from the kernel source: a retune of STARK_WIDE_THREADS or SHK_STARK_SPLIT_LOG fails here instead of dropping coverage."""
    th = sv.thresholds()
    cases = load_golden("stark_variants.json")["cases"]
    have = set()
    bounds = {}
    for c in cases:
        have |= sv.cells_of(c, th)
        for b in sv.boundary_rows(c, th):
            bounds.setdefault(c["width"], set()).add(b)
        assert len(c["unit_sha256"]) == c["batch"]
        degree = max(sum(k) for d in c["step_polys"] for k, _ in d)
        assert c["width"] <= 9 and sum(len(d) for d in c["step_polys"]) <= 256
        assert degree * (c["steps"] - 1) + 1 < c["steps"] * c["ext"]
    missing = sv.required_cells(th) - have
    assert not missing, "uncovered kernel cells: %s" % sorted(missing, key=str)
    need = {"split4", "split", "split+1p", "wide-1p", "wide"}
    assert any(need <= b for b in bounds.values()), bounds
    assert {4, 8, 16} <= {c["ext"] for c in cases}
    assert any(c["batch"] & (c["batch"] - 1) for c in cases)
    assert max(sum(len(d) for d in c["step_polys"]) for c in cases) == 256
