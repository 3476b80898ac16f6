"""The device polynomial arithmetic's decomposition (starks_amd/csrc/poly_items.cuh) run on the host by
tests/native/poly_tree_host.cpp (hipcc): the same padded product tree, Newton inverses, scaled remainder tree and numerator tree as
api_poly.hip drives on the GPU, every level a batch of size-2d transforms, at n ~ 10^3 -- against exact Python-int schoolbook products,
long division, zpoly and O(n^2) Lagrange, and against tests/golden/poly_arith.json (the live reference's outputs).  CPU only."""
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_golden
from poly_arith_cases import P, divmod_, ints, lagrange, matches, mul, resolved, strip, wire, zpoly

G = resolved(load_golden("poly_arith.json"))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pa") / "poly_tree_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "poly_tree_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _run(driver, d, op, **files):
    for k, v in files.items():
        (d / k).write_bytes(wire(v))
    out = subprocess.run([driver, op, str(d)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return int(out.stdout)


def _rand(rnd, n):
    return [rnd.randrange(P) for _ in range(n)]


SIZES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 127, 128, 129, 255, 300, 511, 512, 513, 1000, 1023, 1024, 1025]


@pytest.mark.parametrize("n", SIZES)
def test_zpoly_host(driver, tmp_path, n):
    xs = _rand(random.Random(n), n)
    _run(driver, tmp_path, "zpoly", xs=xs)
    assert ints((tmp_path / "out").read_bytes()) == zpoly(xs)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 9, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 383, 700])
def test_lagrange_host(driver, tmp_path, n):
    rnd = random.Random(1000 + n)
    xs, ys = _rand(rnd, n), _rand(rnd, n)
    if n > 4:  # repeated and zero x's
        xs[1] = xs[0]
        xs[n // 2] = 0
    _run(driver, tmp_path, "lagrange", xs=xs, ys=ys)
    assert ints((tmp_path / "out").read_bytes()) == lagrange(xs, ys)


@pytest.mark.parametrize("na,nb", [(1, 1), (1, 9), (2, 2), (31, 33), (64, 64), (65, 64), (200, 57), (511, 514), (1000, 1025)])
def test_mul_host(driver, tmp_path, na, nb):
    rnd = random.Random(na * 7 + nb)
    a, b = _rand(rnd, na), _rand(rnd, nb)
    _run(driver, tmp_path, "mul", a=a, b=b)
    assert ints((tmp_path / "out").read_bytes()) == mul(a, b)


@pytest.mark.parametrize("na,nb", [(1, 1), (9, 1), (9, 2), (33, 33), (5, 9), (64, 33), (129, 64), (1000, 3), (1025, 512), (1024, 1023)])
def test_divmod_host(driver, tmp_path, na, nb):
    rnd = random.Random(na * 11 + nb)
    a, b = _rand(rnd, na), _rand(rnd, nb)
    b[-1] = b[-1] or 1
    _run(driver, tmp_path, "divmod", a=a, b=b)
    assert (ints((tmp_path / "q").read_bytes()), ints((tmp_path / "r").read_bytes())) == divmod_(a, b)


def test_fixture_host(driver, tmp_path):
    """every case of the fixture through the host decomposition (inputs >= p and negative included)"""
    for c in G["mul"]:
        _run(driver, tmp_path, "mul", a=c["a"], b=c["b"])
        assert matches(c["out"], strip(ints((tmp_path / "out").read_bytes())))
    for c in G["divmod"]:
        _run(driver, tmp_path, "divmod", a=c["a"], b=c["b"])
        assert matches(c["q"], strip(ints((tmp_path / "q").read_bytes()))), c["name"]
        assert matches(c["r"], strip(ints((tmp_path / "r").read_bytes()))), c["name"]
    for c in G["zpoly"]:
        _run(driver, tmp_path, "zpoly", xs=c["xs"])
        assert matches(c["out"], ints((tmp_path / "out").read_bytes()))
    for c in G["lagrange"]:
        _run(driver, tmp_path, "lagrange", xs=c["xs"], ys=c["ys"])
        assert matches(c["out"], strip(ints((tmp_path / "out").read_bytes()))), c["name"]


def test_fixture_restatements():
    """the Python-int statements the GPU tests use agree with the live reference's outputs"""
    for c in G["mul"]:
        assert matches(c["out"], strip(mul([x % P for x in c["a"]], [x % P for x in c["b"]])))
    for c in G["divmod"]:
        q, r = divmod_(c["a"], c["b"])
        assert matches(c["q"], strip(q)) and matches(c["r"], strip(r)), c["name"]
    for c in G["zpoly"]:
        assert matches(c["out"], zpoly([x % P for x in c["xs"]]))
    for c in G["lagrange"]:
        assert matches(c["out"], strip(lagrange(c["xs"], c["ys"]))), c["name"]


def test_fixture_degenerate_cases_present():
    names = {c["name"] for c in G["lagrange"]}
    assert {"repeated", "all_repeated", "zero_ys", "negative", "random_0", "random_1"} <= names
    assert {c["name"] for c in G["divmod"]} >= {"deg0", "deg1", "nonmonic", "short", "exact"}
    assert any(x >= P for c in G["mul"] for x in c["a"])
