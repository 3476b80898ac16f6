"""Polynomial evaluation's two device decompositions (starks_amd/csrc/poly_items.cuh: pa_eval_direct and pa_eval_tree) run on the
host by tests/native/poly_eval_host.cpp (hipcc): the direct path's lanes, workgroup sums and second-pass sums over the same shapes
the GPU launches, and the chunked scaled remainder tree's batched root product and descent -- against exact Python-int Horner, and
against tests/golden/poly_eval.json (the live reference's Polynomial.__call__).  The host form of poly_utils.multi_eval over Z/5 and
Z/11 is checked against the reference's __call__ restated in Python ints.  CPU only."""
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_golden
from poly_arith_cases import P, horner, ints, operand, wire

G = load_golden("poly_eval.json")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pe") / "poly_eval_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "poly_eval_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _run(driver, d, path, coefs, xs, batch=1):
    (d / "coefs").write_bytes(wire(coefs))
    (d / "xs").write_bytes(wire(xs))
    out = subprocess.run([driver, path, str(d), str(batch)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return ints((d / "out").read_bytes()), [int(v) for v in out.stdout.split()]


def _want(coefs, xs, batch=1):
    n = len(coefs) // batch
    return [horner([c % P for c in coefs[b * n:(b + 1) * n]], x % P) for b in range(batch) for x in xs]


def _rand(rnd, n):
    return [rnd.randrange(P) for _ in range(n)]


SIZES = [0, 1, 2, 3, 7, 8, 9, 127, 128, 129, 1000, 1025]
PAIRS = sorted({(n, m) for n in SIZES for m in SIZES if n * m <= 1025 * 9 or n in (0, 1) or m in (0, 1)} |
               {(1000, 1000), (1025, 129), (129, 1025), (1025, 1025), (128, 128)})


@pytest.mark.parametrize("path", ["direct", "tree"])
@pytest.mark.parametrize("n,m", PAIRS)
def test_eval_host(driver, tmp_path, path, n, m):
    """n < m, n = m and n >> m (several chunks of the tree path); unreduced coefficients, the zero point, repeated points"""
    rnd = random.Random(n * 10007 + m)
    coefs, xs = _rand(rnd, n), _rand(rnd, m)
    if n > 2:
        coefs[1] = P + rnd.randrange(2**256 - P)  # >= p
    if m > 3:
        xs[0], xs[2] = 0, xs[1]
        xs[3] = P + rnd.randrange(2**256 - P)
    got, _ = _run(driver, tmp_path, path, coefs, xs)
    assert got == _want(coefs, xs)


@pytest.mark.parametrize("path", ["direct", "tree"])
@pytest.mark.parametrize("n,m,batch", [(0, 5, 3), (1, 4, 2), (9, 7, 3), (128, 3, 4), (300, 33, 2), (1025, 2, 3), (5, 1000, 2)])
def test_eval_host_batch(driver, tmp_path, path, n, m, batch):
    rnd = random.Random(n * 31 + m * 7 + batch)
    coefs, xs = _rand(rnd, batch * n), _rand(rnd, m)
    got, _ = _run(driver, tmp_path, path, coefs, xs, batch)
    assert got == _want(coefs, xs, batch)


@pytest.mark.parametrize("n,m", [(1 << 15, 1), (40000, 3), ((1 << 15) + 5, 5)])
def test_eval_host_direct_workgroups(driver, tmp_path, n, m):
    """long polynomials: the direct path's coefficients split over several workgroups, added by the second pass"""
    rnd = random.Random(n + m)
    coefs, xs = _rand(rnd, n), _rand(rnd, m)
    got, shape = _run(driver, tmp_path, "direct", coefs, xs)
    assert shape[0] > 1
    assert got == _want(coefs, xs)


def test_eval_host_tree_chunks(driver, tmp_path):
    """m = 3 points (N = 4) and 1000 coefficients: 250 chunks through one batched descent"""
    rnd = random.Random(5)
    coefs, xs = _rand(rnd, 1000), [0, 7, 7]
    got, shape = _run(driver, tmp_path, "tree", coefs, xs)
    assert shape == [4, 250]
    assert got == _want(coefs, xs)


def test_fixture_host(driver, tmp_path):
    """every case of the fixture through both host decompositions (inputs >= p and negative included)"""
    for c in G["eval"]:
        coefs, xs = operand(c["coefs"]), operand(c["xs"])
        for path in ("direct", "tree"):
            got, _ = _run(driver, tmp_path, path, coefs, xs)
            assert got == c["out"], (c["name"], path)


def test_fixture_restatements():
    """the Python-int Horner the GPU tests use agrees with the live reference's outputs"""
    for c in G["eval"]:
        assert _want(operand(c["coefs"]), operand(c["xs"])) == c["out"], c["name"]


@pytest.mark.parametrize("n,m,want", [(1 << 15, 1 << 13, 1), (1 << 16, 1 << 13, 0), (1 << 14, 1 << 10, 1), (1 << 16, 1 << 16, 0),
                                       (1 << 24, 1, 1), (1 << 24, 128, 1), (1 << 20, 1 << 20, 0), (1 << 18, 1 << 10, 1)])
def test_path_rule(driver, n, m, want):
    """the default path on both sides of the crossover stated in include/starkhip.h (poly_items.cuh: pe_direct_preferred)"""
    out = subprocess.run([driver, "rule", str(n), str(m), "1"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and int(out.stdout) == want


def test_fixture_degenerate_cases_present():
    names = {c["name"] for c in G["eval"]}
    assert {"zero_poly", "constant", "zero_and_repeated_x", "only_zero_point", "negative", "unreduced_all"} <= names
    assert any(x >= P for c in G["eval"] for x in operand(c["coefs"]))
    assert all(len(c["out"]) == len(operand(c["xs"])) for c in G["eval"])


@pytest.mark.parametrize("p", [5, 11])
def test_multi_eval_host_rings(p):
    """poly_utils.multi_eval over Z/5 and Z/11 is the reference's __call__ per point (polynomial.py:158-164: y += x^i a_i over
    the stripped coefficients, in the ring)"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    from starks_amd.poly_utils import multi_eval
    F = IntegersModP(p)
    Poly = polynomials_over(F)
    rnd = random.Random(p)
    for n in (0, 1, 2, 5, 13):
        coefs = [rnd.randrange(3 * p) - p for _ in range(n)]
        xs = [rnd.randrange(p) for _ in range(7)] + [0, p + 3, -2]
        want = [sum(c * pow(x, i, p) for i, c in enumerate(coefs)) % p for x in xs]
        ours = multi_eval(F, Poly(coefs), xs)
        assert all(isinstance(v, F) for v in ours)
        assert [int(v) for v in ours] == want
        assert [int(v) for v in multi_eval(F, coefs, [F(x) for x in xs])] == want
        assert [Poly(coefs)(x) for x in xs] == ours
