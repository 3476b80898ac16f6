"""The generic-modulus polynomial arithmetic and batch inversion's CPU half: tests/native/modpoly_host.cpp (hipcc) runs the very drivers
of starks_amd/csrc/poly_items.cuh and the element steps of modpoly_items.cuh -- the code api_modpoly.hip runs -- on a host Ops (a
textbook NTT over fpm, loops over the item bodies, the batch inversion tile by tile with tiny tiles and with the production tile),
against the exact Python-int statements of tests/modpoly_cases.py over ten moduli and against tests/golden/mod_poly.json (the live
reference's outputs over IntegersModP(p)).  Also: the largest transform the host Ops saw equals sh_mod_poly_max_transform's formula,
two roots of one order give the same bytes, the driver's restatement of the root checks, the library cross-compiles and exports the
entries, two_adic_root and the prime test, and the Python routing rule.  CPU only.
What this half does NOT run: the host checks of api_modpoly.hip (they need a context, hence a device): tests/test_gpu_modpoly.py."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_golden
import modpoly_cases as mp
from modpoly_cases import FIELDS, ints, matches, strip, wire

CSRC = os.path.join(ROOT, "starks_amd", "csrc")
G = mp.resolved(load_golden("mod_poly.json"))
MODULI = list(FIELDS)
IDS = {mp.BN254: "bn254", mp.BLS12_381: "bls12_381", mp.GOLDILOCKS: "goldilocks", mp.BABYBEAR: "babybear", mp.KOALABEAR: "koalabear",
       65537: "f65537", 12289: "f12289", 193: "f193", 97: "f97", mp.MIMC_P: "mimc"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mp") / "modpoly_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "modpoly_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, p, op, args, root=None, **files):
    (d / "mod").write_bytes(p.to_bytes(32, "big"))
    if root is not None:
        (d / "root").write_bytes(root.to_bytes(32, "big"))
    for k, v in files.items():
        (d / k).write_bytes(wire(p, v))
    return subprocess.run([driver, op, str(d)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def _poly(driver, d, p, op, opcode, sizes, root=None, **files):
    """one driver run of a polynomial operation; checks the largest transform against the formula in both languages"""
    w, k = root or mp.two_adic_root(p)
    out = _call(driver, d, p, op, [k], root=w, **files)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    seen, formula, _ = (int(x) for x in out.stdout.split())
    assert seen == formula == mp.max_transform(opcode, *sizes), (op, sizes, seen, formula)


def _admits(p, opcode, *sizes):
    return mp.max_transform(opcode, *sizes) <= 1 << mp.two_adic_root(p)[1]


def _rand(rnd, p, n):
    return [rnd.randrange(p) for _ in range(n)]


# ---- the size grids of tests/test_poly_arith_host.py, cut to what each field's 2-adicity admits -------------------------------------
ZPOLY_SIZES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 127, 128, 129, 255, 300, 511, 512, 513, 1000, 1023, 1024, 1025]
LAGRANGE_SIZES = [1, 2, 3, 5, 8, 9, 15, 16, 17, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 383, 700]
MUL_SIZES = [(1, 1), (1, 9), (2, 2), (31, 33), (64, 64), (65, 64), (200, 57), (511, 514), (1000, 1025)]
DIVMOD_SIZES = [(1, 1), (9, 1), (9, 2), (33, 33), (5, 9), (64, 33), (129, 64), (1000, 3), (1025, 512), (1024, 1023)]


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_zpoly_host(driver, tmp_path, p):
    ran = 0
    for n in ZPOLY_SIZES:
        if _admits(p, mp.OP_ZPOLY, n):
            xs = _rand(random.Random(n), p, n)
            _poly(driver, tmp_path, p, "zpoly", mp.OP_ZPOLY, (n,), xs=xs)
            assert ints((tmp_path / "out").read_bytes()) == mp.zpoly(p, xs), n
            ran += 1
    assert ran >= 8


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_lagrange_host(driver, tmp_path, p):
    ran = 0
    for n in LAGRANGE_SIZES:
        if _admits(p, mp.OP_LAGRANGE, n):
            rnd = random.Random(1000 + n)
            xs, ys = _rand(rnd, p, n), _rand(rnd, p, n)
            if n > 4:  # repeated and zero x's
                xs[1] = xs[0]
                xs[n // 2] = 0
            _poly(driver, tmp_path, p, "lagrange", mp.OP_LAGRANGE, (n,), xs=xs, ys=ys)
            assert ints((tmp_path / "out").read_bytes()) == mp.lagrange(p, xs, ys), n
            ran += 1
    assert ran >= 8


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_mul_host(driver, tmp_path, p):
    ran = 0
    for na, nb in MUL_SIZES:
        if _admits(p, mp.OP_MUL, na, nb):
            rnd = random.Random(na * 7 + nb)
            a, b = _rand(rnd, p, na), _rand(rnd, p, nb)
            a[0] += p * ((2**256 - 1 - a[0]) // p)  # an unreduced wire value
            _poly(driver, tmp_path, p, "mul", mp.OP_MUL, (na, nb), a=a, b=b)
            assert ints((tmp_path / "out").read_bytes()) == mp.mul(p, a, b), (na, nb)
            ran += 1
    assert ran >= 3


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_divmod_host(driver, tmp_path, p):
    ran = 0
    for na, nb in DIVMOD_SIZES:
        if _admits(p, mp.OP_DIVMOD, na, nb):
            rnd = random.Random(na * 11 + nb)
            a, b = _rand(rnd, p, na), _rand(rnd, p, nb)
            b[-1] = b[-1] or 1
            a[-1] += p * ((2**256 - 1 - a[-1]) // p)
            _poly(driver, tmp_path, p, "divmod", mp.OP_DIVMOD, (na, nb), a=a, b=b)
            assert (ints((tmp_path / "q").read_bytes()), ints((tmp_path / "r").read_bytes())) == mp.divmod_(p, a, b), (na, nb)
            ran += 1
    assert ran >= 4


# ---- the batch inversion: tiny tiles (three or more levels at n ~ 10^3) and the production tile --------------------------------------
@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
@pytest.mark.parametrize("L,C,n,levels", [(4, 2, 1000, 4), (2, 2, 700, 5), (8, 3, 1000, 3), (256, 2, 1000, 2), (256, 2, 512, 1), (4, 2, 1, 1)])
def test_multi_inv_host(driver, tmp_path, p, L, C, n, levels):
    rnd = random.Random(n * L + C)
    vals = [rnd.randrange(2**256) for _ in range(n)]  # any 256-bit value
    for i in (0, n // 3, n - 1):
        vals[i] = 0
    if n > 8:
        vals[5] = p  # == 0 mod p, stored unreduced
        vals[6] = p - 1
    out = _call(driver, tmp_path, p, "inv", [L, C], **{"in": vals})
    assert out.returncode == 0, out.stderr
    depth, powers, launches = (int(x) for x in out.stdout.split())
    assert (depth, powers, launches) == (levels, 1, 2 * levels - 1)
    got = ints((tmp_path / "out").read_bytes())
    assert got == mp.multi_inv(p, vals)
    assert all((v * w) % p == (1 if v % p else 0) for v, w in zip(vals, got))


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
@pytest.mark.parametrize("L,C,rows,levels", [(4, 1, 100, 4), (2, 2, 65, 4), (256, 1, 300, 2), (256, 1, 7, 1)])
def test_multi_interp_4_host(driver, tmp_path, p, L, C, rows, levels):
    rnd = random.Random(rows * L + C)
    xs, ys = [rnd.randrange(2**256) for _ in range(4 * rows)], [rnd.randrange(2**256) for _ in range(4 * rows)]
    for r in range(1, rows, 5):  # a pair, a triple, all four equal
        for k in range(1, 1 + (r % 3) + 1):
            xs[4 * r + k] = xs[4 * r]
    out = _call(driver, tmp_path, p, "interp", [L, C], xs=xs, ys=ys)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.split()] == [levels, 1, 2 * levels - 1]
    assert ints((tmp_path / "out").read_bytes()) == mp.multi_interp_4(p, xs, ys)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def _fixture_inputs(c):
    if c["op"] == "multi_inv":
        v = list(c["in"])
        for i in c["zeros"]:
            v[i] = 0
        return v
    return None


def test_fixture_restatements():
    """the Python-int statements the host and GPU tests use agree with the live reference's outputs"""
    assert {c["p"] for c in G} == set(mp.FIXTURE_MODULI)
    for c in G:
        p, op, key = c["p"], c["op"], (c["p"], c["op"], c["name"])
        if op == "mul":
            assert matches(c["out"], strip(mp.mul(p, c["a"], c["b"]))), key
        elif op == "divmod":
            q, r = mp.divmod_(p, c["a"], c["b"])
            assert matches(c["q"], strip(q)) and matches(c["r"], strip(r)), key
        elif op == "zpoly":
            assert matches(c["out"], mp.zpoly(p, c["xs"])), key
        elif op == "lagrange":
            assert matches(c["out"], strip(mp.lagrange(p, c["xs"], c["ys"]))), key
        elif op == "multi_inv":
            assert matches(c["out"], mp.multi_inv(p, _fixture_inputs(c))), key
        else:
            assert matches(c["out"], mp.multi_interp_4(p, c["xs"], c["ys"])), key
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mod_poly.json")) < 1 << 18


def test_fixture_degenerate_cases_present():
    for p in mp.FIXTURE_MODULI:
        mine = [c for c in G if c["p"] == p]
        assert {"repeated", "all_repeated", "zero_ys", "negative", "zero_x", "random_0", "random_1", "one"} <= \
            {c["name"] for c in mine if c["op"] == "lagrange"}
        assert {c["name"] for c in mine if c["op"] == "divmod"} >= {"short", "one_coeff", "small_monic", "small_exact"}
        assert any(x >= p for c in mine if c["op"] == "mul" for x in c["a"])
        assert any(c["name"] == "n0" for c in mine if c["op"] == "zpoly")
    big = [c for c in G if c["p"] == mp.BN254]
    assert {c["name"] for c in big if c["op"] == "divmod"} >= {"deg0", "deg1", "monic", "nonmonic", "exact", "short"}


@pytest.mark.parametrize("p", mp.FIXTURE_MODULI, ids=IDS.get)
def test_fixture_host(driver, tmp_path, p):
    """every case of the fixture through the host decomposition (inputs >= p and negative included)"""
    for c in (c for c in G if c["p"] == p):
        op, key = c["op"], (c["op"], c["name"])
        if op == "mul":
            _poly(driver, tmp_path, p, "mul", mp.OP_MUL, (len(c["a"]), len(c["b"])), a=c["a"], b=c["b"])
            assert matches(c["out"], strip(ints((tmp_path / "out").read_bytes()))), key
        elif op == "divmod":
            _poly(driver, tmp_path, p, "divmod", mp.OP_DIVMOD, (len(c["a"]), len(c["b"])), a=c["a"], b=c["b"])
            assert matches(c["q"], strip(ints((tmp_path / "q").read_bytes()))), key
            assert matches(c["r"], strip(ints((tmp_path / "r").read_bytes()))), key
        elif op == "zpoly":
            _poly(driver, tmp_path, p, "zpoly", mp.OP_ZPOLY, (len(c["xs"]),), xs=c["xs"])
            assert matches(c["out"], ints((tmp_path / "out").read_bytes())), key
        elif op == "lagrange":
            _poly(driver, tmp_path, p, "lagrange", mp.OP_LAGRANGE, (len(c["xs"]),), xs=c["xs"], ys=c["ys"])
            assert matches(c["out"], strip(ints((tmp_path / "out").read_bytes()))), key
        elif op == "multi_inv":
            assert _call(driver, tmp_path, p, "inv", [4, 2], **{"in": _fixture_inputs(c)}).returncode == 0
            assert matches(c["out"], ints((tmp_path / "out").read_bytes())), key
        else:
            assert _call(driver, tmp_path, p, "interp", [4, 1], xs=c["xs"], ys=c["ys"]).returncode == 0
            assert matches(c["out"], ints((tmp_path / "out").read_bytes())), key


# ---- roots ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [mp.BN254, mp.GOLDILOCKS, 12289, 97], ids=IDS.get)
def test_any_root_of_the_order_gives_the_same_bytes(driver, tmp_path, p):
    """every result is an exact polynomial identity: root^3 (another root of the same order), and a root of a smaller order that
    still admits the call, give identical bytes"""
    w, k = mp.two_adic_root(p)
    n = 13 if k >= 6 else 7
    rnd = random.Random(p % 1000)
    xs, ys, a, b = _rand(rnd, p, n), _rand(rnd, p, n), _rand(rnd, p, 2 * n), _rand(rnd, p, n - 2)
    need = max(mp.max_transform(mp.OP_LAGRANGE, n), mp.max_transform(mp.OP_DIVMOD, 2 * n, n - 2)).bit_length() - 1
    roots = [(w, k), (pow(w, 3, p), k), (pow(w, 1 << (k - need), p), need)]
    assert len({r for r, _ in roots}) == 3 or k == need
    res = []
    for root in roots:
        got = []
        _poly(driver, tmp_path, p, "lagrange", mp.OP_LAGRANGE, (n,), root=root, xs=xs, ys=ys)
        got.append((tmp_path / "out").read_bytes())
        _poly(driver, tmp_path, p, "zpoly", mp.OP_ZPOLY, (n,), root=root, xs=xs)
        got.append((tmp_path / "out").read_bytes())
        _poly(driver, tmp_path, p, "divmod", mp.OP_DIVMOD, (2 * n, n - 2), root=root, a=a, b=b[:-1] + [b[-1] or 1])
        got.append((tmp_path / "q").read_bytes() + (tmp_path / "r").read_bytes())
        res.append(got)
    assert res[0] == res[1] == res[2]
    assert ints(res[0][0]) == mp.lagrange(p, xs, ys)


def test_driver_root_checks(driver, tmp_path):
    """the driver's restatement of the host checks: an even modulus, a root of the wrong order, a call above the root's order"""
    p = 97
    w, k = mp.two_adic_root(p)
    xs = list(range(1, 21))
    assert _call(driver, tmp_path, 96, "zpoly", [k], root=w, xs=xs).returncode == 4
    assert _call(driver, tmp_path, p, "zpoly", [k - 1], root=w, xs=xs).returncode == 5       # order 32 given as 16
    assert _call(driver, tmp_path, p, "zpoly", [k], root=pow(w, 2, p), xs=xs).returncode == 5  # order 16 given as 32
    # 20 x 20 coefficients need a transform of 64 against a root of order 32
    assert mp.max_transform(mp.OP_MUL, 20, 20) == 64
    assert _call(driver, tmp_path, p, "mul", [k], root=w, a=xs, b=xs).returncode == 7
    assert _call(driver, tmp_path, p, "mul", [k], root=w, a=xs[:16], b=xs).returncode == 7
    assert _call(driver, tmp_path, p, "mul", [k], root=w, a=xs[:13], b=xs).returncode == 0


def test_max_transform_formula():
    """the contract of include/starkhip.h in closed form at the sizes the issue names"""
    assert mp.max_transform(mp.OP_MUL, 0, 5) == 0 and mp.max_transform(mp.OP_MUL, 1, 1) == 2
    assert mp.max_transform(mp.OP_MUL, 1 << 20, 1 << 20) == 1 << 21
    assert mp.max_transform(mp.OP_DIVMOD, 5, 9) == 0 and mp.max_transform(mp.OP_DIVMOD, 1, 1) == 2
    assert mp.max_transform(mp.OP_DIVMOD, (1 << 16) + 5, (1 << 15) - 3) == 1 << 17
    assert mp.max_transform(mp.OP_ZPOLY, 0) == 0 and mp.max_transform(mp.OP_ZPOLY, 1) == 2 and mp.max_transform(mp.OP_ZPOLY, 1025) == 2048
    assert mp.max_transform(mp.OP_LAGRANGE, 700) == 2048 and mp.max_transform(mp.OP_LAGRANGE, 1) == 4


# ---- the library and the Python call sites -------------------------------------------------------------------------------------------
NAMES = ["sh_mod_multi_inv", "sh_mod_multi_interp_4", "sh_mod_poly_mul", "sh_mod_poly_divmod", "sh_mod_zpoly", "sh_mod_lagrange_interp"]


def test_library_cross_compiles():
    """the two new translation units for gfx950, and the symbols the header declares in the built library"""
    for src in ("modpoly.hip", "api_modpoly.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in NAMES + [n.replace("sh_", "sh_dev_", 1) for n in NAMES]:
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header
    assert "uint64_t sh_mod_poly_max_transform(" in header
    for op, sizes in ((mp.OP_MUL, (20, 20)), (mp.OP_MUL, (0, 3)), (mp.OP_DIVMOD, (1025, 512)), (mp.OP_DIVMOD, (3, 9)), (mp.OP_DIVMOD, (9, 1)),
                      (mp.OP_ZPOLY, (0, 0)), (mp.OP_ZPOLY, (513, 0)), (mp.OP_LAGRANGE, (700, 0)), (mp.OP_LAGRANGE, (1, 0))):
        assert L.sh_mod_poly_max_transform(op, *sizes) == mp.max_transform(op, *sizes), (op, sizes)


def test_two_adic_root_and_prime_test():
    from starks_amd import _lib
    for p, (s, g) in FIELDS.items():
        w, k = _lib.two_adic_root(p)
        assert k == min(s, 26) and (w, k) == mp.two_adic_root(p, g)
        assert pow(w, 1 << (k - 1), p) == p - 1
        assert _lib.is_probable_prime(p)
    for c in (1, 9, 91, 561, 65535, 2**64 - 1, mp.BN254 * 3, mp.BN254 - 2, 3215031751, 2**256 - 1):
        assert not _lib.is_probable_prime(c), c
    with pytest.raises(ValueError):
        _lib.two_adic_root(64)


def test_routing_rule(monkeypatch):
    """never asks for a context; Z/7, Z/31, a composite modulus, a size below the threshold and a field of too little 2-adicity stay
    on the host path; with a context held, a size at the threshold over BN254 goes to the device entry"""
    from starks_amd import IntegersModP, _lib, poly_utils, polynomial
    from starks_amd.polynomial import polynomials_over
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("routing must not ask for a context"))
    calls = []
    for mod, name in ((polynomial, "mod_mul_wire"), (polynomial, "mod_divmod_wire"), (poly_utils, "mod_zpoly_wire"),
                      (poly_utils, "mod_lagrange_interp_wire"), (poly_utils, "mod_multi_inv_wire"), (poly_utils, "mod_multi_interp_4_wire")):
        monkeypatch.setattr(mod, name, lambda *a, _n=name, **k: calls.append(_n) or pytest.fail("device entry called: " + _n))
    monkeypatch.setattr(polynomial, "MOD_DEVICE_MIN", {"mul": 4, "divmod": 4})
    monkeypatch.setattr(poly_utils, "MOD_DEVICE_MIN", {"multi_inv": 16, "multi_interp_4": 4, "zpoly": 4, "lagrange_interp": 4})

    def run_all(p, n, prime=True):
        F = IntegersModP(p)
        P = polynomials_over(F)
        vals = [(3 * i + 1) % p for i in range(n)]
        a, b = P(vals), P(vals[: max(n // 2, 1)] + [1])
        prod = a * b
        q, r = divmod(prod, b)
        assert q == a and r.is_zero()
        assert (prod % b).is_zero() and prod / b == a
        pts = list(range(1, n + 1)) if n < p else vals
        z = poly_utils.zpoly(F, pts)
        assert all(int(z(F(x))) == 0 for x in pts[:3])
        poly_utils.lagrange_interp(F, [F(x) for x in pts], [F(v) for v in vals])
        # the inversions run no transform: any prime field reaches the device at the threshold, so these stay below it (8 < 16, 3 < 4)
        inv = [int(x) for x in poly_utils.multi_inv(F, vals[:8])]  # over a composite modulus the host path's values are today's
        assert not prime or inv == mp.multi_inv(p, vals[:8])
        poly_utils.multi_interp_4(F, [[F(1), F(2), F(3), F(4)]] * 3, [[F(5), F(6), F(0), F(1)]] * 3)

    for held in (None, object()):
        monkeypatch.setattr(_lib, "_ctx", held)
        run_all(7, 6)                  # the reference's Z/7
        run_all(31, 8)                 # Z/31
        run_all(mp.BN254 * 3, 8, False)  # odd and composite: the prime test keeps it off the device
        run_all(mp.BN254, 2)           # below every threshold (the product has 3 coefficients)
        run_all(97, 40)                # 97 admits transforms of 32 only
        assert calls == []
    monkeypatch.setattr(_lib, "_ctx", None)
    run_all(mp.BN254, 16)              # no context: the host path at any size
    assert calls == []
    # the rule itself, with a context held and the real library's sh_mod_poly_max_transform
    monkeypatch.setattr(_lib, "_ctx", object())
    F = IntegersModP(mp.BN254)
    assert polynomial._mod_on_device(F, "mul", mp.OP_MUL, 4, 4) and not polynomial._mod_on_device(F, "mul", mp.OP_MUL, 100, 3)  # the shorter operand
    assert polynomial._mod_on_device(F, "divmod", mp.OP_DIVMOD, 7, 4) and not polynomial._mod_on_device(F, "divmod", mp.OP_DIVMOD, 100, 98)
    assert poly_utils._mod_on_device(F, "zpoly", 4, mp.OP_ZPOLY) and poly_utils._mod_on_device(F, "multi_inv", 16)
    assert not poly_utils._mod_on_device(F, "multi_inv", 15) and poly_utils._mod_on_device(IntegersModP(7), "multi_inv", 16)
    assert not poly_utils._mod_on_device(IntegersModP(mp.BN254 * 3), "multi_inv", 16)
    assert not poly_utils._mod_on_device(IntegersModP(7), "zpoly", 4, mp.OP_ZPOLY)  # Z/7 admits transforms of 2 only
    F97 = IntegersModP(97)
    assert polynomial._mod_on_device(F97, "mul", mp.OP_MUL, 16, 17) and not polynomial._mod_on_device(F97, "mul", mp.OP_MUL, 20, 20)
    assert poly_utils._mod_on_device(F97, "lagrange_interp", 16, mp.OP_LAGRANGE)
    assert not poly_utils._mod_on_device(F97, "lagrange_interp", 17, mp.OP_LAGRANGE)
    assert not polynomial._mod_on_device(IntegersModP(mp.MIMC_P), "mul", mp.OP_MUL, 64, 64)   # the MiMC prime keeps its own path
    assert not polynomial._mod_on_device(IntegersModP(1 << 64), "mul", mp.OP_MUL, 64, 64)     # even
    assert not polynomial._mod_on_device(IntegersModP(2**256 + 297), "mul", mp.OP_MUL, 64, 64)  # 257 bits
    with pytest.raises(pytest.fail.Exception):
        polynomials_over(F)(list(range(1, 9))) * polynomials_over(F)([1, 2, 3, 4])  # at the threshold: the device entry is called
    assert calls == ["mod_mul_wire"]
