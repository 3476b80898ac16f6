"""The packed-word polynomial arithmetic and batch inversion's CPU half: tests/native/mod64poly_host.cpp (hipcc) runs the very drivers
of starks_amd/csrc/poly_items.cuh and the element steps of mod64poly_items.cuh -- the code api_mod64poly.hip runs -- on a host Ops (a
textbook NTT over f64_*, loops over the item bodies, the batch inversion tile by tile with tiny tiles and with the production tile),
against the exact Python-int statements of tests/modpoly_cases.py over ten moduli below 2^64 and against the outputs recorded in
tests/golden/mod_poly.json.  Also: the largest transform the host Ops saw equals sh_mod_poly_max_transform's formula, two roots of one
order give the same words, unreduced input words give the outputs of their residues, the inversion's level boundaries, the library
cross-compiles and exports the twelve entries, and the Python argument helper.  CPU only.
What this half does NOT run: the host checks of api_mod64poly.hip (they need a context, hence a device): tests/test_gpu_mod64poly.py."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_golden
import mod64poly_cases as mc
from mod64poly_cases import FIELDS, IDS, unwords, words

CSRC = os.path.join(ROOT, "starks_amd", "csrc")
G = mc.resolved(load_golden("mod_poly.json"))
MODULI = list(FIELDS)
IV_T, ROW_T = 2048, 1024  # the production tiles: M6P_IV_LANES x M6P_IV_CHUNK, x M6P_IV_ROW_CHUNK (mod64poly_items.cuh)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("m6p") / "mod64poly_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "mod64poly_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, p, op, args, **files):
    for k, v in files.items():
        (d / k).write_bytes(words(p, v))
    return subprocess.run([driver, op, str(d), str(p)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def _poly(driver, d, p, op, opcode, sizes, root=None, **files):
    """one driver run of a polynomial operation; checks the largest transform against the formula in both languages"""
    w, k = root or mc.two_adic_root(p)
    out = _call(driver, d, p, op, [w, k], **files)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    seen, formula, _ = (int(x) for x in out.stdout.split())
    assert seen == formula == mc.max_transform(opcode, *sizes), (op, sizes, seen, formula)


def _read(d, name):
    return unwords((d / name).read_bytes())


def _rand(rnd, p, n):
    return [rnd.randrange(p) for _ in range(n)]


def test_modulus_table():
    """the table's own claims: every modulus is prime (Miller-Rabin), below 2^64, with the 2-adicity stated; two of them exceed 2^63"""
    for p, s in FIELDS.items():
        assert mc.is_prime(p) and 3 <= p < 2**64 and ((p - 1) & -(p - 1)).bit_length() - 1 == s, p
        w, k = mc.two_adic_root(p)
        assert k == min(s, 26) and pow(w, 1 << (k - 1), p) == p - 1
    assert mc.P63 == 9223372036904058881 and 2**63 < mc.P63 < mc.GOLDILOCKS < mc.BIG and not mc.is_prime(mc.BIG + 2)
    assert all(not mc.is_prime(q) for q in range(mc.BIG + 1, 2**64))


# ---- every op against exact ints over the ten moduli ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_zpoly_host(driver, tmp_path, p):
    ran = 0
    for n in mc.ZPOLY_SIZES:
        if mc.admits(p, mc.OP_ZPOLY, n):
            xs = _rand(random.Random(n), p, n)
            _poly(driver, tmp_path, p, "zpoly", mc.OP_ZPOLY, (n,), xs=xs)
            assert _read(tmp_path, "out") == mc.zpoly(p, xs), n
            ran += 1
    assert ran >= mc.floor(p, "zpoly")


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_lagrange_host(driver, tmp_path, p):
    ran = 0
    for n in mc.LAGRANGE_SIZES:
        if mc.admits(p, mc.OP_LAGRANGE, n):
            rnd = random.Random(1000 + n)
            xs, ys = _rand(rnd, p, n), _rand(rnd, p, n)
            if n > 4:  # repeated and zero x's
                xs[1] = xs[0]
                xs[n // 2] = 0
            _poly(driver, tmp_path, p, "lagrange", mc.OP_LAGRANGE, (n,), xs=xs, ys=ys)
            assert _read(tmp_path, "out") == mc.lagrange(p, xs, ys), n
            ran += 1
    assert ran >= mc.floor(p, "lagrange")


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_mul_host(driver, tmp_path, p):
    ran = 0
    for na, nb in mc.MUL_SIZES:
        if mc.admits(p, mc.OP_MUL, na, nb):
            rnd = random.Random(na * 7 + nb)
            a, b = _rand(rnd, p, na), _rand(rnd, p, nb)
            a[0] += p * ((2**64 - 1 - a[0]) // p)  # an unreduced word
            _poly(driver, tmp_path, p, "mul", mc.OP_MUL, (na, nb), a=a, b=b)
            assert _read(tmp_path, "out") == mc.mul(p, a, b), (na, nb)
            ran += 1
    assert ran >= mc.floor(p, "mul")


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_divmod_host(driver, tmp_path, p):
    ran = 0
    for na, nb in mc.DIVMOD_SIZES:
        if mc.admits(p, mc.OP_DIVMOD, na, nb):
            rnd = random.Random(na * 11 + nb)
            a, b = _rand(rnd, p, na), _rand(rnd, p, nb)
            b[-1] = b[-1] or 1
            a[-1] += p * ((2**64 - 1 - a[-1]) // p)
            _poly(driver, tmp_path, p, "divmod", mc.OP_DIVMOD, (na, nb), a=a, b=b)
            assert (_read(tmp_path, "q"), _read(tmp_path, "r")) == mc.divmod_(p, a, b), (na, nb)
            ran += 1
    assert ran >= mc.floor(p, "divmod")


# ---- the batch inversion: tiny tiles (three or more levels at n ~ 10^3) and the production tiles -------------------------------------
def _inv_values(rnd, p, n):
    vals = [rnd.randrange(2**64) for _ in range(n)]  # any 64-bit value
    for i in (0, n // 3, n - 1):
        vals[i] = 0
    if n > 8:
        vals[5] = p  # == 0 mod p, stored unreduced
        vals[6] = p - 1
        vals[7] = p * ((2**64 - 1) // p)  # the largest multiple of p in a word
    return vals


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
@pytest.mark.parametrize("L,C,n,levels", [(4, 2, 1000, 4), (2, 2, 700, 5), (8, 3, 1000, 3), (256, 8, 3000, 2), (256, 8, 2048, 1), (4, 2, 1, 1)])
def test_multi_inv_host(driver, tmp_path, p, L, C, n, levels):
    vals = _inv_values(random.Random(n * L + C), p, n)
    out = _call(driver, tmp_path, p, "inv", [L, C], **{"in": vals})
    assert out.returncode == 0, out.stderr
    depth, powers, launches = (int(x) for x in out.stdout.split())
    assert (depth, powers, launches) == (levels, 1, 2 * levels - 1)
    got = _read(tmp_path, "out")
    assert got == mc.multi_inv(p, vals)
    assert all((v * w) % p == (1 if v % p else 0) for v, w in zip(vals, got))


def _interp_rows(rnd, rows):
    xs, ys = [rnd.randrange(2**64) for _ in range(4 * rows)], [rnd.randrange(2**64) for _ in range(4 * rows)]
    for r in range(1, rows, 5):  # a pair, a triple, all four equal
        for k in range(1, 1 + (r % 3) + 1):
            xs[4 * r + k] = xs[4 * r]
    return xs, ys


@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
@pytest.mark.parametrize("L,C,rows,levels", [(4, 1, 100, 4), (2, 2, 65, 4), (256, 4, 1100, 2), (256, 4, 7, 1)])
def test_multi_interp_4_host(driver, tmp_path, p, L, C, rows, levels):
    xs, ys = _interp_rows(random.Random(rows * L + C), rows)
    out = _call(driver, tmp_path, p, "interp", [L, C], xs=xs, ys=ys)
    assert out.returncode == 0, out.stderr
    assert [int(x) for x in out.stdout.split()] == [levels, 1, 2 * levels - 1]
    assert _read(tmp_path, "out") == mc.multi_interp_4(p, xs, ys)


def _depth(n, T):
    d = 1
    while n > T:
        n, d = -(-n // T), d + 1
    return d


@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.BIG, 3], ids=IDS.get)
def test_inversion_level_boundaries(driver, tmp_path, p):
    """one below, at and one above each level boundary: a 4-item tile up to three levels, the production tiles up to T + 1 (T^2 items
    take the serial host walk too long; tests/test_gpu_mod64poly.py runs them)"""
    for L, C, T in ((2, 2, 4), (4, 1, 4)):
        for n in (1, T - 1, T, T + 1, T * T - 1, T * T, T * T + 1):
            rnd = random.Random(n + T)
            if C == 2:
                vals = [rnd.randrange(2**64) for _ in range(n)]
                vals[n - 1] = p if n % 2 else 0
                out = _call(driver, tmp_path, p, "inv", [L, C], **{"in": vals})
                want = mc.multi_inv(p, vals)
            else:
                xs, ys = _interp_rows(rnd, n)
                out = _call(driver, tmp_path, p, "interp", [L, C], xs=xs, ys=ys)
                want = mc.multi_interp_4(p, xs, ys)
            assert out.returncode == 0 and int(out.stdout.split()[0]) == _depth(n, T), (n, out.stdout)
            assert _read(tmp_path, "out") == want, (L, C, n)
    for n in (1, IV_T - 1, IV_T, IV_T + 1):
        vals = _inv_values(random.Random(n), p, n) if n > 3 else [5]
        out = _call(driver, tmp_path, p, "inv", [256, 8], **{"in": vals})
        assert out.returncode == 0 and int(out.stdout.split()[0]) == _depth(n, IV_T)
        assert _read(tmp_path, "out") == mc.multi_inv(p, vals), n
    for rows in (1, ROW_T - 1, ROW_T, ROW_T + 1):
        xs, ys = _interp_rows(random.Random(rows), rows)
        out = _call(driver, tmp_path, p, "interp", [256, 4], xs=xs, ys=ys)
        assert out.returncode == 0 and int(out.stdout.split()[0]) == _depth(rows, ROW_T)
        assert _read(tmp_path, "out") == mc.multi_interp_4(p, xs, ys), rows


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", mc.FIXTURE_MODULI, ids=IDS.get)
def test_fixture_host(driver, tmp_path, p):
    """every recorded case below 2^64 through the host decomposition: the word operands are the recorded ones reduced mod p"""
    mine = [c for c in G if c["p"] == p]
    assert len(mine) == (38 if p == 97 else 57) and {c["op"] for c in mine} == {"mul", "divmod", "zpoly", "lagrange", "multi_inv", "multi_interp_4"}
    for c in mine:
        op, key, f = c["op"], (c["op"], c["name"]), mc.fixture_words(p, c)
        if op == "mul":
            if not f["a"] or not f["b"]:
                continue  # the driver takes no empty operand: tests/test_gpu_mod64poly.py runs the entries' empty cases
            _poly(driver, tmp_path, p, "mul", mc.OP_MUL, (len(f["a"]), len(f["b"])), **f)
            got = [_read(tmp_path, "out")]
        elif op == "divmod":
            if not f["a"]:
                continue
            _poly(driver, tmp_path, p, "divmod", mc.OP_DIVMOD, (len(f["a"]), len(f["b"])), **f)
            got = [_read(tmp_path, "q"), _read(tmp_path, "r")]
        elif op == "zpoly":
            _poly(driver, tmp_path, p, "zpoly", mc.OP_ZPOLY, (len(f["xs"]),), **f)
            got = [_read(tmp_path, "out")]
        elif op == "lagrange":
            _poly(driver, tmp_path, p, "lagrange", mc.OP_LAGRANGE, (len(f["xs"]),), **f)
            got = [_read(tmp_path, "out")]
        elif op == "multi_inv":
            assert _call(driver, tmp_path, p, "inv", [4, 2], **f).returncode == 0
            got = [_read(tmp_path, "out")]
        else:
            assert _call(driver, tmp_path, p, "interp", [4, 1], **f).returncode == 0
            got = [_read(tmp_path, "out")]
        for rec, g in zip(mc.recorded(c), mc.normal(c, got)):
            assert mc.matches(rec, g), key


# ---- roots and unreduced inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.P63, 12289, 97], ids=IDS.get)
def test_any_root_of_the_order_gives_the_same_words(driver, tmp_path, p):
    """every result is an exact polynomial identity: root^3 (another root of the same order), and a root of a smaller order that
    still admits the call, give identical words"""
    w, k = mc.two_adic_root(p)
    n = 13 if k >= 6 else 7
    rnd = random.Random(p % 1000)
    xs, ys, a, b = _rand(rnd, p, n), _rand(rnd, p, n), _rand(rnd, p, 2 * n), _rand(rnd, p, n - 2)
    need = max(mc.max_transform(mc.OP_LAGRANGE, n), mc.max_transform(mc.OP_DIVMOD, 2 * n, n - 2)).bit_length() - 1
    roots = [(w, k), (pow(w, 3, p), k), (pow(w, 1 << (k - need), p), need)]
    assert len({r for r, _ in roots}) == 3 or k == need
    res = []
    for root in roots:
        got = []
        _poly(driver, tmp_path, p, "lagrange", mc.OP_LAGRANGE, (n,), root=root, xs=xs, ys=ys)
        got.append((tmp_path / "out").read_bytes())
        _poly(driver, tmp_path, p, "zpoly", mc.OP_ZPOLY, (n,), root=root, xs=xs)
        got.append((tmp_path / "out").read_bytes())
        _poly(driver, tmp_path, p, "divmod", mc.OP_DIVMOD, (2 * n, n - 2), root=root, a=a, b=b[:-1] + [b[-1] or 1])
        got.append((tmp_path / "q").read_bytes() + (tmp_path / "r").read_bytes())
        res.append(got)
    assert res[0] == res[1] == res[2]
    assert unwords(res[0][0]) == mc.lagrange(p, xs, ys)


@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.P63, mc.BABYBEAR, 65537, 97], ids=IDS.get)
def test_unreduced_words(driver, tmp_path, p):
    """words in [p, 2^64) -- p itself, 2^64 - 1 and multiples of p among them -- give the outputs of their residues, in every op"""
    rnd = random.Random(p % 997)
    n = 9
    xs, ys, a, b = _rand(rnd, p, n), _rand(rnd, p, n), _rand(rnd, p, 2 * n), _rand(rnd, p, n - 2)
    for v in (xs, ys, a, b):  # every other residue below 2^64 - p, so that an unreduced word of it exists above 2^63 too
        v[::2] = [x % (2**64 - p) for x in v[::2]]
    xs[2], ys[3], a[4], b[1] = 0, 0, 0, 0
    b[-1] = b[-1] or 1
    a[0] = (2**64 - 1) % p  # lifts to 2^64 - 1
    up = {k: mc.lifted(p, v, rnd) for k, v in (("xs", xs), ("ys", ys), ("a", a), ("b", b))}
    up["xs"][2], up["ys"][3], up["a"][4], up["b"][1] = p, p, p * ((2**64 - 1) // p), p  # zeros as p and as the largest multiple of p
    assert up["a"][0] == 2**64 - 1 and sum(v >= p for k in up for v in up[k]) >= 8
    assert all(u % p == v for k, vals in (("xs", xs), ("ys", ys), ("a", a), ("b", b)) for u, v in zip(up[k], vals))
    for vals in (dict(xs=xs, ys=ys, a=a, b=b), up):
        _poly(driver, tmp_path, p, "mul", mc.OP_MUL, (2 * n, n - 2), a=vals["a"], b=vals["b"])
        assert _read(tmp_path, "out") == mc.mul(p, a, b)
        _poly(driver, tmp_path, p, "divmod", mc.OP_DIVMOD, (2 * n, n - 2), a=vals["a"], b=vals["b"])
        assert (_read(tmp_path, "q"), _read(tmp_path, "r")) == mc.divmod_(p, a, b)
        _poly(driver, tmp_path, p, "zpoly", mc.OP_ZPOLY, (n,), xs=vals["xs"])
        assert _read(tmp_path, "out") == mc.zpoly(p, xs)
        _poly(driver, tmp_path, p, "lagrange", mc.OP_LAGRANGE, (n,), xs=vals["xs"], ys=vals["ys"])
        assert _read(tmp_path, "out") == mc.lagrange(p, xs, ys)
        assert _call(driver, tmp_path, p, "inv", [4, 2], **{"in": vals["a"]}).returncode == 0
        assert _read(tmp_path, "out") == mc.multi_inv(p, a)
        assert _call(driver, tmp_path, p, "interp", [4, 1], xs=vals["xs"][:8], ys=vals["ys"][:8]).returncode == 0
        assert _read(tmp_path, "out") == mc.multi_interp_4(p, xs[:8], ys[:8])


def test_driver_root_checks(driver, tmp_path):
    """the driver's restatement of the host checks: an even modulus, 0 and 1, a root of the wrong order, a root at or above p, a call
    above the root's order"""
    p = 97
    w, k = mc.two_adic_root(p)
    xs = list(range(1, 21))
    for bad in (96, 0, 1):
        assert _call(driver, tmp_path, bad, "zpoly", [w, k], xs=xs).returncode == 4
    assert _call(driver, tmp_path, p, "zpoly", [w, k - 1], xs=xs).returncode == 5            # order 32 given as 16
    assert _call(driver, tmp_path, p, "zpoly", [pow(w, 2, p), k], xs=xs).returncode == 5     # order 16 given as 32
    assert _call(driver, tmp_path, p, "zpoly", [w + p, k], xs=xs).returncode == 5            # at or above p
    assert mc.max_transform(mc.OP_MUL, 20, 20) == 64
    assert _call(driver, tmp_path, p, "mul", [w, k], a=xs, b=xs).returncode == 7
    assert _call(driver, tmp_path, p, "mul", [w, k], a=xs[:13], b=xs).returncode == 0


# ---- the library and the Python call sites -------------------------------------------------------------------------------------------
NAMES = ["sh_mod64_multi_inv", "sh_mod64_multi_interp_4", "sh_mod64_poly_mul", "sh_mod64_poly_divmod", "sh_mod64_zpoly",
         "sh_mod64_lagrange_interp"]


def test_library_cross_compiles():
    """the two new translation units for gfx950, and the twelve symbols the header declares in the built library"""
    for src in ("mod64poly.hip", "api_mod64poly.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in NAMES + [n.replace("sh_", "sh_dev_", 1) for n in NAMES]:
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header
        assert L._sig[name][1][1] is ctypes.c_uint64  # the modulus is a word
    assert "mod64poly.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_python_forms_without_a_device(monkeypatch):
    """the argument helper, and what the six word forms decide before they ask for a context"""
    from starks_amd import _lib, poly_utils, polynomial
    assert _lib.mod64_poly_args(mc.GOLDILOCKS) == (mc.GOLDILOCKS,) + mc.two_adic_root(mc.GOLDILOCKS)
    assert _lib.mod64_poly_args(97, (pow(28, 3, 97) + 97, 5)) == (97, pow(28, 3, 97), 5)
    for bad in (2**64 + 13, 1, 0):
        with pytest.raises(ValueError):
            _lib.mod64_poly_args(bad)
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("an empty call must not ask for a context"))
    assert len(polynomial.mod64_mul_words(97, [], [1, 2])) == 0 and len(poly_utils.mod64_multi_inv_words(97, b"")) == 0
    assert len(poly_utils.mod64_lagrange_interp_words(97, [], [])) == 0 and len(poly_utils.mod64_multi_interp_4_words(97, [], [])) == 0
    with pytest.raises(ZeroDivisionError):
        polynomial.mod64_divmod_words(97, [1, 2], [])
    with pytest.raises(ValueError):
        poly_utils.mod64_multi_interp_4_words(97, [1, 2, 3], [1, 2, 3])
    with pytest.raises(ValueError):
        poly_utils.mod64_lagrange_interp_words(97, [1, 2], b"\0" * 8)
    with pytest.raises(ValueError):
        polynomial.mod64_mul_words(97, b"\0" * 7, [1])
