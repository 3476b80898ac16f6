"""sh_mod_poly_eval's CPU half: tests/native/modeval_host.cpp (hipcc) runs the templated drivers of starks_amd/csrc/poly_items.cuh
(pa_eval, pa_eval_direct, pa_eval_tree) over fpm with the element steps of modeval_items.cuh -- the code api_modpoly.hip runs -- on a
host Ops: the direct path's lanes, workgroup sums and second pass, the tree path's chunks, root product, descent and combine, against
exact Python-int Horner over seven moduli and against tests/golden/mod_poly_eval.json (the live reference's Polynomial.__call__ over
IntegersModP(p)).  Over the MiMC prime the bytes equal poly_eval_host's.  Also: the largest transform the Ops saw against
sh_mod_poly_max_transform(4, n, m), the path rules against their stated formula, the library's symbols, header and prototypes, and
the Python routing predicates without a context.  One more build of the same driver under ASan + UBSan runs three cases as its own
program.  CPU only."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT, load_golden
import modeval_cases as me
import modpoly_cases as mp
from modeval_cases import IDS, MODULI, evaluate, ints, matches, wire

CSRC = os.path.join(ROOT, "starks_amd", "csrc")
G = mp.resolved(load_golden("mod_poly_eval.json"))
HIPCC = ["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("me") / "modeval_host")
    subprocess.check_call(HIPCC + [os.path.join(ROOT, "tests", "native", "modeval_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module")
def mimc_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pe") / "poly_eval_host")
    subprocess.check_call(HIPCC + [os.path.join(ROOT, "tests", "native", "poly_eval_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _run(driver, d, p, path, coefs, xs, batch=1, root=None, check=True):
    w, k = root or mp.two_adic_root(p)
    (d / "mod").write_bytes(p.to_bytes(32, "big"))
    (d / "root").write_bytes(w.to_bytes(32, "big"))
    (d / "coefs").write_bytes(wire(p, coefs))
    (d / "xs").write_bytes(wire(p, xs))
    out = subprocess.run([driver, path, str(d), str(batch), str(k)], capture_output=True, text=True, timeout=600)
    if not check:
        return out
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    seen, formula, transforms, a, b, c = (int(v) for v in out.stdout.split())
    n, m = len(coefs) // batch, len(xs)
    assert formula == me.max_transform(n, m), (n, m, formula)
    if path == "direct":
        assert seen == 0 and transforms == 0, "the direct path runs no transform"
        assert (a, b, c) == me.direct_shape(n, m, batch) or not (n and m)
    elif n and m:
        assert seen == formula, (n, m, seen, formula)
    return (d / "out").read_bytes(), (a, b, c)


def _admits(p, n, m):
    return me.max_transform(n, m) <= 1 << mp.two_adic_root(p)[1]


def _paths(p, n, m):
    return ["direct"] + (["tree"] if _admits(p, n, m) else [])


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_eval_host(driver, tmp_path, p):
    """n < m, n = m and n >> m over the grid; unreduced coefficients and points, the point 0, a repeated point; m = 1, 2, 3, 7, 9, 129:
    no multiple of the group size"""
    trees = 0
    for n, m in me.PAIRS:
        coefs, xs = me.inputs(p, n, m)
        want = evaluate(p, coefs, xs)
        for path in _paths(p, n, m):
            got, _ = _run(driver, tmp_path, p, path, coefs, xs)
            assert ints(got) == want, (n, m, path)
            trees += path == "tree"
    assert trees >= (len(me.PAIRS) if mp.two_adic_root(p)[1] >= 12 else 0)


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_eval_host_batch(driver, tmp_path, p):
    for n, m, batch in me.BATCHES:
        coefs, xs = me.inputs(p, n, m, batch)
        for path in _paths(p, n, m):
            got, _ = _run(driver, tmp_path, p, path, coefs, xs, batch)
            assert ints(got) == evaluate(p, coefs, xs, batch), (n, m, batch, path)


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
@pytest.mark.parametrize("n,m", me.WIDE)
def test_eval_host_direct_workgroups(driver, tmp_path, p, n, m):
    """long polynomials: W > 1 workgroups per point group, added by the second pass (W = 1 against W > 1 on one polynomial needs 2^26
    products and runs on the GPU: tests/test_gpu_modeval.py)"""
    coefs, xs = me.inputs(p, n, m)
    got, shape = _run(driver, tmp_path, p, "direct", coefs, xs)
    assert shape[0] > 1 and shape[2] == (me.ME_GROUP if m >= me.ME_GROUP else 1)
    assert ints(got) == evaluate(p, coefs, xs)


@pytest.mark.parametrize("p", [97, mp.GOLDILOCKS, mp.BN254], ids=IDS.get)
def test_eval_host_tree_chunks(driver, tmp_path, p):
    """m = 3 points (N = 4) and 1000 coefficients: 250 chunks through one batched descent"""
    coefs, _ = me.inputs(p, 1000, 3)
    xs = [0, 7, 7 + p]
    got, shape = _run(driver, tmp_path, p, "tree", coefs, xs)
    assert shape == (4, 250, 0)
    assert ints(got) == evaluate(p, coefs, xs)


def test_mimc_prime_equals_poly_eval_host(driver, mimc_driver, tmp_path):
    """over the MiMC prime (p > 2^255: the ninth word) both paths give poly_eval_host's bytes"""
    p = mp.MIMC_P
    for n, m, batch in [(257, 5, 1), (1000, 64, 1), (129, 129, 1), (9, 7, 3), ((1 << 15) + 5, 5, 1)]:
        coefs, xs = me.inputs(p, n, m, batch)
        for path in ("direct", "tree"):
            got, _ = _run(driver, tmp_path, p, path, coefs, xs, batch)
            d = tmp_path / "mimc"
            d.mkdir(exist_ok=True)
            (d / "coefs").write_bytes(wire(p, coefs))
            (d / "xs").write_bytes(wire(p, xs))
            assert subprocess.run([mimc_driver, path, str(d), str(batch)], capture_output=True, timeout=600).returncode == 0
            assert got == (d / "out").read_bytes(), (n, m, batch, path)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_restatements():
    assert {c["p"] for c in G} == set(mp.FIXTURE_MODULI)
    for c in G:
        assert matches(c["out"], evaluate(c["p"], c["a"], c["xs"])), (c["p"], c["name"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mod_poly_eval.json")) < 1 << 17


def test_fixture_cases_present():
    for p in mp.FIXTURE_MODULI:
        mine = {c["name"]: c for c in G if c["p"] == p}
        assert {"zero_poly", "constant", "zero_and_repeated_x", "all_points_equal", "only_zero_point", "trailing_zeros", "negative",
                "unreduced_all", "random_1000_64"} <= set(mine)
        assert any(x >= p for x in mine["random_1000_64"]["a"]) and mine["zero_poly"]["out"]["vals"] == [0] * 4
        assert all(c["out"]["len"] == len(c["xs"]) for c in mine.values())


@pytest.mark.parametrize("p", mp.FIXTURE_MODULI, ids=IDS.get)
def test_fixture_host(driver, tmp_path, p):
    for c in (c for c in G if c["p"] == p):
        for path in _paths(p, len(c["a"]), len(c["xs"])):
            got, _ = _run(driver, tmp_path, p, path, c["a"], c["xs"])
            assert matches(c["out"], ints(got)), (c["name"], path)


# ---- transforms, roots and the path rules --------------------------------------------------------------------------------------------
def test_max_transform_formula():
    assert me.max_transform(0, 5) == 0 and me.max_transform(5, 0) == 0 and me.max_transform(1, 1) == 4
    assert me.max_transform(1 << 24, 3) == 8 and me.max_transform(7, 1024) == 2048 and me.max_transform(7, 1025) == 4096
    assert me.max_transform(1 << 20, 1 << 20) == 1 << 21


def test_direct_path_needs_no_root(driver, tmp_path):
    """root_log = 0 with root = 1 is valid on the direct path, over fields of any 2-adicity; a tree there is refused by the Ops"""
    for p in (3, 97, mp.BN254):
        coefs, xs = me.inputs(p, 300, 9)
        got, _ = _run(driver, tmp_path, p, "direct", coefs, xs, root=(1, 0))
        assert ints(got) == evaluate(p, coefs, xs)
        assert _run(driver, tmp_path, p, "tree", coefs, xs, root=(1, 0), check=False).returncode == 7


def test_small_two_adicity(driver, tmp_path):
    """over 97 (transforms up to 32) the rule chooses direct for m > 16 whatever the cost rule says, a forced tree there is refused,
    and m = 16 still runs the tree"""
    p = 97
    w, k = mp.two_adic_root(p)
    assert k == 5
    shapes = [(1 << 20, 17), (1 << 24, 64), (1 << 22, 1 << 12), (1 << 20, 1 << 20), (1 << 22, 16), (1 << 16, 8)]
    f = tmp_path / "shapes"
    f.write_text("".join("%d %d 1\n" % s for s in shapes))
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([driver, "rules", str(f), str(k)], text=True).splitlines()]
    for (n, m), (_, generic, chosen) in zip(shapes, rows):
        assert chosen == (1 if m > 16 else generic), (n, m)
    assert any(generic == 0 for (n, m), (_, generic, _c) in zip(shapes, rows) if m > 16)  # the cost rule alone would take the tree
    coefs, xs = me.inputs(p, 100, 17)
    assert _run(driver, tmp_path, p, "tree", coefs, xs, check=False).returncode == 7
    coefs, xs = me.inputs(p, 100, 16)
    got, _ = _run(driver, tmp_path, p, "tree", coefs, xs)
    assert ints(got) == evaluate(p, coefs, xs)


def test_path_rules(driver, tmp_path):
    """the MiMC rule decides as the parent commit's constants do over a grid; the generic rule is its stated formula over its own
    constants, with both decisions present on either side of a crossover"""
    lines = subprocess.check_output([driver, "consts"], text=True).splitlines()
    mimc, generic = (tuple(float(v) for v in line.split()) for line in lines)
    assert mimc == me.MIMC_COST
    shapes = [(1 << a, 1 << b, batch) for a in range(0, 26, 2) for b in range(0, 21, 2) for batch in (1, 4)]
    shapes += [(1 << 15, 1 << 13, 1), (1 << 16, 1 << 13, 1), (1000, 1000, 1), (1 << 24, 1, 1), (1 << 20, 1 << 20, 1), (12345, 678, 3)]
    f = tmp_path / "shapes"
    f.write_text("".join("%d %d %d\n" % s for s in shapes))
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([driver, "rules", str(f), "26"], text=True).splitlines()]
    assert len(rows) == len(shapes)
    for s, (got_mimc, got_generic, chosen) in zip(shapes, rows):
        assert got_mimc == me.direct_preferred(me.MIMC_COST, *s), s
        assert got_generic == chosen == me.direct_preferred(generic, *s), s
    assert dict(zip(shapes, rows))[(1 << 15, 1 << 13, 1)][0] == 1 and dict(zip(shapes, rows))[(1 << 16, 1 << 13, 1)][0] == 0
    col = [r[1] for r in rows]
    assert 0 in col and 1 in col
    # a crossover of the generic rule along n at m = 2^12: direct below, tree above, one switch
    along = [me.direct_preferred(generic, 1 << a, 1 << 12, 1) for a in range(8, 25)]
    assert along[0] and not along[-1] and sum(x != y for x, y in zip(along, along[1:])) == 1


# ---- under ASan + UBSan, as its own program -------------------------------------------------------------------------------------------
def test_driver_sanitized(tmp_path):
    exe = str(tmp_path / "modeval_host_san")
    subprocess.check_call(HIPCC + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                                   os.path.join(ROOT, "tests", "native", "modeval_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    env.pop("LD_PRELOAD", None)
    for p, path, (n, m, batch) in [(97, "tree", (1000, 3, 1)), (mp.MIMC_P, "direct", ((1 << 15) + 5, 5, 1)), (mp.BN254, "tree", (300, 33, 2))]:
        coefs, xs = me.inputs(p, n, m, batch)
        w, k = mp.two_adic_root(p)
        for name, data in (("mod", p.to_bytes(32, "big")), ("root", w.to_bytes(32, "big")), ("coefs", wire(p, coefs)), ("xs", wire(p, xs))):
            (tmp_path / name).write_bytes(data)
        out = subprocess.run([exe, path, str(tmp_path), str(batch), str(k)], capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
        assert ints((tmp_path / "out").read_bytes()) == evaluate(p, coefs, xs, batch)


# ---- the library and the Python call sites -------------------------------------------------------------------------------------------
def test_library_exports_and_header():
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, "modeval.hip"),
                           "-o", os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("sh_mod_poly_eval", "sh_dev_mod_poly_eval"):
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header
        assert len(L._sig[name][1]) == 10
    assert "SH_MOD_POLY_EVAL = 4" in header and _lib.MOD_POLY_EVAL == 4
    still_open = [line for line in header.splitlines() if "STILL OPEN" in line]
    assert still_open and all("sh_mod_poly_eval" not in line and "evaluation" not in line for line in still_open)
    for n, m in ((0, 5), (5, 0), (1, 1), (1000, 3), (7, 1025), (1 << 20, 1 << 20)):
        assert L.sh_mod_poly_max_transform(4, n, m) == me.max_transform(n, m), (n, m)
    assert L.sh_mod_poly_max_transform(3, 700, 0) == 2048 and L.sh_mod_poly_max_transform(5, 9, 9) == 0  # ops 0-3 unchanged, no op 5


def test_routing_without_a_context(monkeypatch):
    """no context held: __call__ and multi_eval over BN254 stay on the host at any size, never ask for a context and return what the
    host loop returns; with one held the predicates open from the thresholds on, and never for a composite modulus, Z/11 or the MiMC prime"""
    from starks_amd import IntegersModP, _lib, poly_utils, polynomial
    from starks_amd.polynomial import polynomials_over
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("routing must not ask for a context"))
    monkeypatch.setattr(polynomial, "mod_eval_wire", lambda *a, **k: pytest.fail("device entry called"))
    for held in (None, object()):
        monkeypatch.setattr(_lib, "_ctx", held)
        # (modulus, coefficients): without a context any size stays; with one, the reference's small rings at the sizes of its own
        # tests (below the thresholds) and a composite modulus at any size
        for p, n in (((mp.BN254, 300), (11, 300)) if held is None else ()) + ((11, 8), (7, 5), (5, 3), (mp.BN254 * 3, 300), (mp.BN254, 8)):
            F = IntegersModP(p)
            coefs = [(5 * i + 2) % p for i in range(n)]
            poly = polynomials_over(F)(coefs)
            for x in (0, 3, p - 1):
                y = poly(F(x))
                assert isinstance(y, F) and int(y) == mp.horner(p, coefs, x)
            vals = poly_utils.multi_eval(F, poly, [F(1), F(2), F(0)])
            assert isinstance(vals, list) and [int(v) for v in vals] == evaluate(p, coefs, [1, 2, 0])
    monkeypatch.setattr(polynomial, "MOD_EVAL_DEVICE_MIN_COEFS", 4)
    monkeypatch.setattr(poly_utils, "MOD_EVAL_DEVICE_MIN_WORK", 16)
    monkeypatch.setattr(_lib, "_ctx", object())
    F = IntegersModP(mp.BN254)
    assert polynomial._mod_eval_on_device(F, [F(1)] * 4, F(3)) and polynomial._mod_eval_on_device(F, [F(1)] * 4, 3)
    assert not polynomial._mod_eval_on_device(F, [F(1)] * 3, F(3))
    assert not polynomial._mod_eval_on_device(F, [F(1)] * 4, polynomials_over(F)([1, 2]))  # composition keeps the host loop
    assert not polynomial._mod_eval_on_device(F, [F(1)] * 4, True)
    assert polynomial._mod_eval_on_device(IntegersModP(97), [1] * 4, 3)  # no transform requirement: the direct path is always there
    for bad in (mp.BN254 * 3, 11 * 13, mp.MIMC_P, 1 << 64, 2**256 + 297):
        assert not polynomial._mod_eval_on_device(IntegersModP(bad), [1] * 64, 3)
        assert not poly_utils._mod_eval_on_device(IntegersModP(bad), 64, 64)
    assert poly_utils._mod_eval_on_device(F, 4, 4) and not poly_utils._mod_eval_on_device(F, 5, 3)
    assert not poly_utils._mod_eval_on_device(F, 0, 100) and not poly_utils._mod_eval_on_device(F, 100, 0)
    monkeypatch.setattr(_lib, "_ctx", None)
    assert not polynomial._mod_eval_on_device(F, [F(1)] * 64, F(3)) and not poly_utils._mod_eval_on_device(F, 64, 64)
