"""Polynomial evaluation at arbitrary points over any prime modulus below 2^256 on the MI355X (sh_mod_poly_eval / sh_dev_mod_poly_eval
of include/starkhip.h; csrc/modeval.hip, modeval_items.cuh, api_modpoly.hip; polynomial.mod_eval_wire, Polynomial.__call__ and
poly_utils.multi_eval): byte-identical to tests/golden/mod_poly_eval.json (the live reference over IntegersModP(p)); exact against
Python-int Horner around the group size, the transform's tile and the workgroup split; both forced paths byte-identical in fresh child
processes on both sides of the default crossover; over the MiMC prime byte-identical to sh_dev_poly_eval; consistent with the transform,
lagrange_interp, zpoly and the product at size; every refusal with its code and the entry's name.  All comparisons are exact."""
import ctypes
import hashlib
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import modeval_cases as me  # noqa: E402
import modpoly_cases as mp  # noqa: E402
from modeval_cases import evaluate, ints, matches, wire  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, ROOT_ORDER, UNSUPPORTED = -1, -2, -6
IDS = {mp.BN254: "bn254", mp.BLS12_381: "bls12_381", mp.GOLDILOCKS: "goldilocks", 65537: "f65537", 97: "f97", mp.MIMC_P: "mimc"}
# both sides of the default crossover of the generic rule at 2^16 points (modeval_items.cuh: ME_COST puts it between 2^12 and 2^13
# coefficients), and a batched shape
CROSSOVER = [(1 << 12, 1 << 16, 1), (1 << 13, 1 << 16, 1), (5000, 300, 2)]


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


@pytest.fixture(scope="module")
def ctx(L):
    from starks_amd import _lib
    return _lib.ctx()


def _args(p, root=None):
    from starks_amd import _lib
    return _lib.mod_poly_args(p, root)


def _err(L):
    from starks_amd import _lib
    return L.sh_last_error(_lib.ctx()).decode()


def _host(L, ctx, p, coefs, xs, batch=1, root=None):
    """sh_mod_poly_eval on ints -> ints"""
    from starks_amd import _lib
    m, w, k = _args(p, root)
    n = len(coefs) // batch
    out = ctypes.create_string_buffer(32 * max(batch * len(xs), 1))
    rc = L.sh_mod_poly_eval(ctx, m, w, k, wire(p, coefs) if n else None, n, batch, wire(p, xs) if xs else None, len(xs), out)
    _lib.check(rc, "sh_mod_poly_eval")
    return ints(out.raw[:32 * batch * len(xs)])


class Dev(object):
    """device buffers of plain limbs: ints up as 8 x u32 little-endian limbs, unreduced, and down the same way"""

    def __init__(self, L, c, elems):
        from starks_amd import _lib
        self.L, self.c, self.d, self._lib = L, c, ctypes.c_void_p(), _lib
        _lib.check(L.sh_dev_alloc(c, 32 * max(elems, 1), ctypes.byref(self.d)), "sh_dev_alloc")

    def at(self, k):
        return ctypes.c_void_p(self.d.value + 32 * k)

    def put(self, k, vals):
        raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
        if raw:
            self._lib.check(self.L.sh_dev_upload(self.c, raw, self.at(k), len(raw)), "sh_dev_upload")

    def get(self, k, n):
        buf = ctypes.create_string_buffer(32 * max(n, 1))
        if n:
            self._lib.check(self.L.sh_dev_download(self.c, self.at(k), buf, 32 * n), "sh_dev_download")
        return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]

    def free(self):
        self.L.sh_dev_free(self.c, self.d)


def _dev(L, ctx, p, coefs, xs, batch=1, root=None):
    """sh_dev_mod_poly_eval on ints (any value below 2^256) -> ints; the output area is poisoned first"""
    from starks_amd import _lib
    m, w, k = _args(p, root)
    nc, nx = len(coefs), len(xs)
    d = Dev(L, ctx, nc + nx + batch * nx + 4)
    try:
        d.put(0, [int(v) if 0 <= int(v) < 2**256 else int(v) % p for v in coefs])
        d.put(nc, [int(v) if 0 <= int(v) < 2**256 else int(v) % p for v in xs])
        d.put(nc + nx, [2**256 - 1] * (batch * nx))
        rc = L.sh_dev_mod_poly_eval(ctx, m, w, k, d.at(0) if nc else None, nc // batch, batch, d.at(nc) if nx else None, nx,
                                    d.at(nc + nx) if nx else None)
        _lib.check(rc, "sh_dev_mod_poly_eval")
        return d.get(nc + nx, batch * nx)
    finally:
        d.free()


# ---- the fixture and exact Horner -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", mp.FIXTURE_MODULI, ids=IDS.get)
def test_fixture_bytes(L, ctx, p):
    for c in (c for c in mp.resolved(load_golden("mod_poly_eval.json")) if c["p"] == p):
        assert matches(c["out"], _host(L, ctx, p, c["a"], c["xs"])), ("host", c["name"])
        assert matches(c["out"], _dev(L, ctx, p, c["a"], c["xs"])), ("dev", c["name"])


SHAPES = [(1, 1, 1), (255, 3, 1), (256, 4, 1), (257, 5, 1), (1025, 9, 1), (1000, 1000, 1), (1025, 1025, 1), ((1 << 15) + 5, 5, 1),
          (1 << 16, 1, 1), (300, 33, 2), (0, 5, 3)]
_WANT = {}


def _case(p, n, m, batch):
    key = (p, n, m, batch)
    if key not in _WANT:
        coefs, xs = me.inputs(p, n, m, batch)
        _WANT[key] = (coefs, xs, evaluate(p, coefs, xs, batch))
    return _WANT[key]


@pytest.mark.parametrize("n,m,batch", SHAPES)
def test_exact_bn254(L, ctx, n, m, batch):
    """the group size (m = 3, 4, 5, 9), the transform's 2^10 tile (1000 and 1025 points), W > 1 (2^15 + 5 and 2^16 coefficients),
    batches and n = 0; inputs stored unreduced, the point 0 and a repeated point"""
    coefs, xs, want = _case(mp.BN254, n, m, batch)
    if n and m:
        assert me.direct_shape(n, m, batch)[0] > 1 or n < 1 << 15
    assert _dev(L, ctx, mp.BN254, coefs, xs, batch) == want
    assert _host(L, ctx, mp.BN254, coefs, xs, batch) == want


@pytest.mark.parametrize("p", [mp.GOLDILOCKS, mp.BLS12_381, 65537, 97, 3], ids=lambda p: IDS.get(p, "f%d" % p))
def test_exact_other_fields(L, ctx, p):
    for n, m, batch in [(257, 5, 1), (1025, 9, 1), (300, 33, 2), ((1 << 15) + 5, 5, 1)]:
        coefs, xs, want = _case(p, n, m, batch)
        assert _dev(L, ctx, p, coefs, xs, batch) == want, (n, m, batch)
    coefs, xs, want = _case(p, 100, 7, 1)
    assert _dev(L, ctx, p, coefs, xs, root=(1, 0)) == want  # no root at all: the direct path


def test_grid_shape_never_changes_a_bit(L, ctx):
    """W = 1 against W > 1 on one polynomial: 2^13 points fill the grid (2048 point groups, W = 1), the first four alone split the
    2^15 coefficients over two workgroups; and a lone point (G = 1, W = 2)"""
    p, n = mp.BN254, 1 << 15
    coefs = mp.vec(p, 4242, n, 7)
    xs = mp.vec(p, 4343, 1 << 13, 5)
    assert me.direct_shape(n, 1 << 13, 1)[0] == 1 and me.direct_shape(n, 4, 1)[0] == 2 and me.direct_shape(n, 1, 1) == (2, 64, 1)
    full = _dev(L, ctx, p, coefs, xs, root=(1, 0))  # root_log = 0 keeps every call on the direct path
    assert _dev(L, ctx, p, coefs, xs[:4], root=(1, 0)) == full[:4]
    assert _dev(L, ctx, p, coefs, xs[:1], root=(1, 0)) == full[:1] == [mp.horner(p, coefs, xs[0] % p)]
    assert full[4095] == mp.horner(p, coefs, xs[4095] % p)


# ---- forced paths, each in a fresh child process ------------------------------------------------------------------------------------
def _path_digests():
    """what a child prints: one sha256 per CROSSOVER shape over BN254 (host-buffer form), then the code and message of m = 64 over 97"""
    from starks_amd import _lib
    L, c = _lib.lib(), _lib.ctx()
    lines = []
    for n, m, batch in CROSSOVER:
        coefs, xs = me.inputs(mp.BN254, n, m, batch)
        lines.append(hashlib.sha256(wire(mp.BN254, _host(L, c, mp.BN254, coefs, xs, batch))).hexdigest())
    coefs, xs = me.inputs(97, 50, 64)
    mod, w, k = _lib.mod_poly_args(97)
    out = ctypes.create_string_buffer(32 * 64)
    rc = L.sh_mod_poly_eval(c, mod, w, k, wire(97, coefs), 50, 1, wire(97, xs), 64, out)
    lines.append("%d %s" % (rc, L.sh_last_error(c).decode() if rc else hashlib.sha256(out.raw).hexdigest()))
    return lines


def test_forced_paths_are_byte_identical(L, ctx):
    """STARKHIP_EVAL_PATH=direct and =tree in child processes started fresh: the same bytes as each other and as this process's
    default choice on both sides of the crossover; a forced tree over 97 at 64 points is refused ("needs"), the default and the forced
    direct path run it"""
    got = {}
    for path in ("direct", "tree"):
        env = dict(os.environ, STARKHIP_EVAL_PATH=path)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "path-child"], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        got[path] = out.stdout.strip().splitlines()[-len(CROSSOVER) - 1:]
    mine = _path_digests()
    assert got["direct"][:-1] == got["tree"][:-1] == mine[:-1]
    assert got["direct"][-1] == mine[-1] and mine[-1].startswith("0 ")
    code, text = got["tree"][-1].split(" ", 1)
    assert int(code) == ROOT_ORDER and text.startswith("sh_mod_poly_eval") and "needs" in text
    for (n, m, batch), digest in zip(CROSSOVER[:2], mine):  # three points of each against Python ints
        coefs, xs = me.inputs(mp.BN254, n, m, batch)
        sub = [xs[0], xs[1], xs[m - 1]]
        assert _host(L, ctx, mp.BN254, coefs, sub) == evaluate(mp.BN254, coefs, sub)


def test_small_two_adicity_runs_direct(L, ctx):
    """over 97 with root_log = 5 the tree admits 16 points: m = 64 takes the direct path and is correct, m = 16 is correct either way"""
    for n, m in ((1000, 64), (1000, 16), (40, 97)):
        coefs, xs, want = _case(97, n, m, 1)
        assert _dev(L, ctx, 97, coefs, xs) == want
        assert _host(L, ctx, 97, coefs, xs) == want


# ---- the MiMC prime and results pinned elsewhere ------------------------------------------------------------------------------------
def test_mimc_prime_equals_sh_dev_poly_eval(L, ctx):
    from starks_amd import _lib
    p = mp.MIMC_P
    for n, m, batch in [(257, 5, 1), (1025, 9, 1), (300, 33, 2), ((1 << 15) + 5, 5, 1), (1000, 1000, 1)]:
        coefs, xs = me.inputs(p, n, m, batch)
        d = Dev(L, ctx, len(coefs) + m + batch * m)
        try:
            d.put(0, coefs)
            d.put(len(coefs), xs)
            _lib.check(L.sh_dev_poly_eval(ctx, d.at(0), n, batch, d.at(len(coefs)), m, d.at(len(coefs) + m)), "sh_dev_poly_eval")
            want = d.get(len(coefs) + m, batch * m)
        finally:
            d.free()
        assert _dev(L, ctx, p, coefs, xs, batch) == want, (n, m, batch)


@pytest.mark.parametrize("p", [mp.BN254, mp.GOLDILOCKS], ids=IDS.get)
def test_consistent_with_the_transform(L, ctx, p):
    """n = m = 2^12 at the roots of unity: sh_dev_mod_ntt's forward transform"""
    from starks_amd import _lib
    n = 1 << 12
    w, k = mp.two_adic_root(p)
    w = pow(w, 1 << (k - 12), p)
    coefs = mp.vec(p, 99, n, 9)
    xs, x = [], 1
    for _ in range(n):
        xs.append(x)
        x = x * w % p
    d = Dev(L, ctx, 2 * n)
    try:
        d.put(0, coefs)
        _lib.check(L.sh_dev_mod_ntt(ctx, p.to_bytes(32, "big"), d.at(0), d.at(n), n, 1, w.to_bytes(32, "big"), 0), "sh_dev_mod_ntt")
        want = d.get(n, n)
    finally:
        d.free()
    assert _dev(L, ctx, p, coefs, xs) == want
    assert want[0] == sum(coefs) % p


def test_consistent_with_lagrange_zpoly_and_mul(L, ctx):
    """the interpolant through (x_i, y_i) takes the y_i at the x_i; zpoly vanishes at its roots and nowhere else sampled; the values
    of a product are the products of the values -- sh_dev_mod_lagrange_interp, sh_dev_mod_zpoly and sh_dev_mod_poly_mul at size"""
    from starks_amd import _lib
    p, n = mp.BN254, 1500
    m, w, k = _args(p)
    xs, ys = mp.vec(p, 11, n, 4), mp.vec(p, 12, n, 6)
    assert len({x % p for x in xs}) == n
    na, nb = 900, 700
    a, b = mp.vec(p, 13, na, 5), mp.vec(p, 14, nb, 3)
    d = Dev(L, ctx, 6 * n + 2 * (na + nb) + 8)
    try:
        o_x, o_y, o_l, o_z, o_a, o_b, o_c = 0, n, 2 * n, 3 * n, 4 * n + 1, 4 * n + 1 + na, 4 * n + 1 + na + nb
        d.put(o_x, xs)
        d.put(o_y, ys)
        d.put(o_a, a)
        d.put(o_b, b)
        _lib.check(L.sh_dev_mod_lagrange_interp(ctx, m, w, k, d.at(o_x), d.at(o_y), n, d.at(o_l)), "sh_dev_mod_lagrange_interp")
        _lib.check(L.sh_dev_mod_zpoly(ctx, m, w, k, d.at(o_x), n, d.at(o_z)), "sh_dev_mod_zpoly")
        _lib.check(L.sh_dev_mod_poly_mul(ctx, m, w, k, d.at(o_a), na, d.at(o_b), nb, d.at(o_c)), "sh_dev_mod_poly_mul")
        lag, z, c = d.get(o_l, n), d.get(o_z, n + 1), d.get(o_c, na + nb - 1)
    finally:
        d.free()
    assert _dev(L, ctx, p, lag, xs) == [y % p for y in ys]
    pts = xs[:700] + [x + 1 for x in xs[:5]]
    vz = _dev(L, ctx, p, z, pts)
    assert vz[:700] == [0] * 700 and all(vz[700:])
    va, vb, vc = _dev(L, ctx, p, a, pts), _dev(L, ctx, p, b, pts), _dev(L, ctx, p, c, pts)
    assert vc == [x * y % p for x, y in zip(va, vb)]


# ---- context behaviour -----------------------------------------------------------------------------------------------------------------
def test_moduli_and_mimc_calls_interleave(L, ctx):
    from starks_amd.polynomial import eval_wire
    p1, p2 = mp.BN254, mp.GOLDILOCKS
    c1, x1, w1 = _case(p1, 1025, 9, 1)
    c2, x2, w2 = _case(p2, 300, 33, 2)
    cm, xm = me.inputs(mp.MIMC_P, 257, 5)
    wm = evaluate(mp.MIMC_P, cm, xm)
    for _ in range(2):
        assert _dev(L, ctx, p1, c1, x1) == w1
        assert ints(eval_wire(wire(mp.MIMC_P, cm), wire(mp.MIMC_P, xm))) == wm
        assert _host(L, ctx, p2, c2, x2, 2) == w2
        assert _host(L, ctx, p1, c1, x1) == w1


def test_refusals(L, ctx):
    """every refusal of the contract, before any launch, with the entry's name opening sh_last_error"""
    p = mp.BN254
    m, w, k = _args(p)
    d = Dev(L, ctx, 64)
    try:
        d.put(0, list(range(64)))
        A, X, O = d.at(0), d.at(16), d.at(32)

        def dev(code, word, mod=m, root=w, rl=k, coefs=A, n=8, batch=1, xs=X, mm=4, out=O):
            assert L.sh_dev_mod_poly_eval(ctx, mod, root, rl, coefs, n, batch, xs, mm, out) == code, word
            assert _err(L).startswith("sh_dev_mod_poly_eval: ") and word in _err(L), _err(L)

        dev(INVALID, "batch", batch=0)
        dev(INVALID, "null", coefs=None)
        dev(INVALID, "null", xs=None)
        dev(INVALID, "null", out=None)
        dev(INVALID, "null", mod=None)
        dev(INVALID, "null", root=None)
        dev(UNSUPPORTED, "2^25", n=(1 << 25) + 1)
        dev(UNSUPPORTED, "2^26", n=1 << 25, batch=3)
        dev(UNSUPPORTED, "2^20", mm=(1 << 20) + 1)
        dev(INVALID, "overlaps", out=d.at(7))    # the last coefficient
        dev(INVALID, "overlaps", out=d.at(13))   # [13, 17) reaches the first point
        dev(INVALID, "overlaps", out=A, n=0, coefs=None, xs=d.at(3))
        dev(INVALID, "modulus", mod=(p + 1).to_bytes(32, "big"))
        dev(INVALID, "modulus", mod=(1).to_bytes(32, "big"))
        dev(ROOT_ORDER, "below", root=(p + 5).to_bytes(32, "big"))
        dev(ROOT_ORDER, "order", rl=k - 1)
        dev(ROOT_ORDER, "order", root=(1).to_bytes(32, "big"))
        dev(UNSUPPORTED, "26", rl=27)
        assert d.get(32, 4) == [32, 33, 34, 35]  # nothing was launched
        # valid degenerate calls: m = 0 with null xs and out writes nothing; n = 0 with null coefs writes zeros; out directly behind xs
        assert L.sh_dev_mod_poly_eval(ctx, m, w, k, A, 8, 1, None, 0, None) == 0
        assert L.sh_dev_mod_poly_eval(ctx, m, w, k, None, 0, 2, X, 4, d.at(20)) == 0
        assert d.get(20, 8) == [0] * 8 and d.get(28, 1) == [28]
        assert L.sh_dev_mod_poly_eval(ctx, m, (1).to_bytes(32, "big"), 0, A, 8, 1, X, 4, O) == 0
        assert d.get(32, 4) == evaluate(p, list(range(8)), [16, 17, 18, 19])
    finally:
        d.free()
    buf = ctypes.create_string_buffer(32 * 8)
    co, xs = wire(p, range(8)), wire(p, range(4))

    def host(code, word, mod=m, root=w, rl=k, coefs=co, n=8, batch=1, pts=xs, mm=4, out=buf):
        assert L.sh_mod_poly_eval(ctx, mod, root, rl, coefs, n, batch, pts, mm, out) == code, word
        assert _err(L).startswith("sh_mod_poly_eval: ") and word in _err(L), _err(L)

    host(INVALID, "batch", batch=0)
    host(INVALID, "null", coefs=None)
    host(INVALID, "null", pts=None)
    host(INVALID, "null", out=None)
    host(UNSUPPORTED, "2^25", n=(1 << 25) + 1)
    host(UNSUPPORTED, "2^20", mm=(1 << 20) + 1)
    host(INVALID, "modulus", mod=(2**200).to_bytes(32, "big"))
    host(ROOT_ORDER, "order", rl=k - 2)
    assert L.sh_mod_poly_eval(ctx, m, w, k, None, 0, 1, None, 0, None) == 0


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [mp.BN254, mp.GOLDILOCKS], ids=IDS.get)
def test_python_forms(L, ctx, p, monkeypatch):
    from starks_amd import IntegersModP, poly_utils, polynomial
    from starks_amd.polynomial import mod_eval_wire, polynomials_over
    from starks_amd.wireseq import WireList
    coefs, xs, want = _case(p, 300, 33, 2)
    assert ints(mod_eval_wire(p, wire(p, coefs), wire(p, xs), batch=2)) == want
    assert ints(mod_eval_wire(p, wire(p, coefs), wire(p, xs), batch=2, root=(1, 0))) == want
    assert mod_eval_wire(p, wire(p, coefs), b"") == b"" and ints(mod_eval_wire(p, b"", wire(p, xs[:3]))) == [0, 0, 0]
    with pytest.raises(ValueError):
        mod_eval_wire(p, wire(p, coefs[:5]), wire(p, xs), batch=2)
    F = IntegersModP(p)
    Poly = polynomials_over(F)
    calls = []
    real = polynomial.mod_eval_wire
    monkeypatch.setattr(polynomial, "mod_eval_wire", lambda *a, **k: calls.append(a[0]) or real(*a, **k))
    n = polynomial.MOD_EVAL_DEVICE_MIN_COEFS
    for size, routed in ((n - 1, 0), (n, 1), (4 * n + 3, 1)):
        c = [v % p for v in mp.vec(p, size, size)]
        c[-1] = c[-1] or 1
        poly = Poly(c)
        del calls[:]
        for x in (F(xs[0]), xs[3] % p, 0):
            y = poly(x)
            assert isinstance(y, F) and int(y) == mp.horner(p, c, int(x) % p)
        assert len(calls) == 3 * routed, size
    # a device-backed polynomial (WireList coefficients) routes the same way
    prod = Poly(c) * Poly(c[:40])
    assert isinstance(prod.coefficients, WireList)
    del calls[:]
    assert int(prod(F(5))) == mp.horner(p, c, 5) * mp.horner(p, c[:40], 5) % p and len(calls) == 1
    # multi_eval: a WireList from the threshold on n m, a list below it
    work = poly_utils.MOD_EVAL_DEVICE_MIN_WORK
    big = poly_utils.multi_eval(F, Poly(c), [F(x) for x in xs])
    assert len(c) * len(xs) >= work and isinstance(big, WireList) and big.field is F
    assert [int(v) for v in big] == evaluate(p, c, xs) and all(isinstance(v, F) for v in big[:2])
    assert [int(v) for v in poly_utils.multi_eval(F, c, xs[:5])] == evaluate(p, c, xs[:5])
    small = poly_utils.multi_eval(F, Poly(c[:3]), [F(1), F(2)])
    assert 6 < work and isinstance(small, list) and [int(v) for v in small] == evaluate(p, c[:3], [1, 2])


def test_other_rings_stay_on_the_host(L, ctx, monkeypatch):
    """a composite modulus at any size and the reference's Z/11 at its own sizes never reach the device entry"""
    from starks_amd import IntegersModP, poly_utils, polynomial
    from starks_amd.polynomial import polynomials_over
    monkeypatch.setattr(polynomial, "mod_eval_wire", lambda *a, **k: pytest.fail("device entry called"))
    for p, n in ((mp.BN254 * 3, 400), (11, 10), (7, 6)):
        F = IntegersModP(p)
        c = [(7 * i + 3) % p for i in range(n)]
        poly = polynomials_over(F)(c)
        assert int(poly(F(2))) == mp.horner(p, c, 2) and isinstance(poly(2), F)
        vals = poly_utils.multi_eval(F, poly, [F(0), F(1), F(2), F(3)])
        assert isinstance(vals, list) and [int(v) for v in vals] == evaluate(p, c, [0, 1, 2, 3])


if __name__ == "__main__" and sys.argv[1:] == ["path-child"]:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    print("\n".join(_path_digests()))
