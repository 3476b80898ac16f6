"""Polynomial products, division, zpoly and lagrange_interp on the MI355X (sh_poly_mul, sh_poly_divmod, sh_zpoly, sh_lagrange_interp
and their sh_dev_* forms; starks_amd.polynomial / poly_utils; csrc/poly_arith.hip): byte-identical to tests/golden/poly_arith.json,
exact against Python ints up to 2^12, O(n) identities at a random point up to the size limits, and lagrange_interp over roots of
unity and a coset equal to the (already pinned) inverse NTT at 2^16 - 2^20 points."""
import ctypes
import os
import random

import pytest

from conftest import load_golden
from poly_arith_cases import P, divmod_, horner, ints, lagrange, matches, mul, resolved, strip, wire, zpoly

pytestmark = pytest.mark.gpu

G = resolved(load_golden("poly_arith.json"))


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def _rand_wire(rnd, n):
    """n values mod p as wire bytes, fast: random 256-bit values with the top bit cleared are < p"""
    import numpy as np
    raw = np.random.default_rng(rnd.getrandbits(64)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x7f
    return raw.tobytes()


def _horner_wire(raw, x):
    y = 0
    mv = memoryview(raw)
    for i in range(len(raw) - 32, -32, -32):
        y = (y * x + int.from_bytes(mv[i:i + 32], "big")) % P
    return y


def _prod_at(raw, r):
    v = 1
    mv = memoryview(raw)
    for i in range(0, len(raw), 32):
        v = v * (r - int.from_bytes(mv[i:i + 32], "big")) % P
    return v


def test_fixture_bytes(L):
    from starks_amd.polynomial import divmod_wire, mul_wire
    from starks_amd.poly_utils import lagrange_interp_wire, zpoly_wire
    for c in G["mul"]:
        assert matches(c["out"], strip(ints(mul_wire(wire(c["a"]), wire(c["b"])))))
    for c in G["divmod"]:
        q, r = divmod_wire(wire(c["a"]), wire(c["b"]))
        assert matches(c["q"], strip(ints(q))) and matches(c["r"], strip(ints(r))), c["name"]
    for c in G["zpoly"]:
        assert matches(c["out"], ints(zpoly_wire(wire(c["xs"]))))
    for c in G["lagrange"]:
        assert matches(c["out"], strip(ints(lagrange_interp_wire(wire(c["xs"]), wire(c["ys"]))))), c["name"]


def test_fixture_python_api(L):
    """the reference's names over IntegersModP(p): the same outputs, ints >= p and negative ints reduced as the reference does"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    from starks_amd.poly_utils import lagrange_interp
    from starks_amd.poly_utils import zpoly as zp
    F = IntegersModP(P)
    Poly = polynomials_over(F)
    for c in G["mul"]:
        assert matches(c["out"], [int(v) for v in (Poly(c["a"]) * Poly(c["b"]))])
    for c in G["divmod"]:
        q, r = divmod(Poly(c["a"]), Poly(c["b"]))
        assert matches(c["q"], q) and matches(c["r"], r), c["name"]
        assert matches(c["q"], Poly(c["a"]) / Poly(c["b"])) and matches(c["r"], Poly(c["a"]) % Poly(c["b"]))
    for c in G["zpoly"]:
        assert matches(c["out"], [int(v) for v in zp(F, c["xs"])])
        assert matches(c["out"], [int(v) for v in zp(F, [F(x) for x in c["xs"]])])
    for c in G["lagrange"]:
        assert matches(c["out"], [int(v) for v in lagrange_interp(F, c["xs"], c["ys"])]), c["name"]


@pytest.mark.parametrize("n", [1, 2, 3, 31, 32, 33, 255, 256, 257, 1000, 1023, 1024, 1025, 4095, 4096])
def test_exact_zpoly_and_products(L, n):
    from starks_amd.polynomial import mul_wire
    from starks_amd.poly_utils import zpoly_wire
    rnd = random.Random(n)
    xs = [rnd.randrange(P) for _ in range(n)]
    want = zpoly(xs) if n <= 1025 else None
    got = ints(zpoly_wire(wire(xs)))
    if want is not None:
        assert got == want
    a = [rnd.randrange(P) for _ in range(n)]
    b = [rnd.randrange(P) for _ in range(n // 3 + 1)]
    assert ints(mul_wire(wire(a), wire(b))) == mul(a, b)
    if n > 1025:  # zpoly above the schoolbook's reach: the tree's result at three points
        assert len(got) == n + 1 and got[-1] == 1
        for r in (rnd.randrange(P) for _ in range(3)):
            assert horner(got, r) == _prod_at(wire(xs), r)


@pytest.mark.parametrize("na,nb", [(1, 1), (4096, 1), (4096, 2), (4096, 4096), (4095, 2049), (3000, 4000), (4097, 17), (2048, 1025)])
def test_exact_divmod(L, na, nb):
    from starks_amd.polynomial import divmod_wire
    rnd = random.Random(na + 31 * nb)
    a = [rnd.randrange(P) for _ in range(na)]
    b = [rnd.randrange(P) for _ in range(nb)]
    q, r = divmod_wire(wire(a), wire(b))
    assert (ints(q), ints(r)) == divmod_(a, b)


@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 257, 700])
def test_exact_lagrange(L, n):
    from starks_amd.poly_utils import lagrange_interp_wire
    rnd = random.Random(7 * n)
    xs = [rnd.randrange(P) for _ in range(n)]
    ys = [rnd.randrange(P) for _ in range(n)]
    if n > 4:
        xs[2] = xs[1]
        xs[-1] = 0
    assert ints(lagrange_interp_wire(wire(xs), wire(ys))) == lagrange(xs, ys)


@pytest.mark.parametrize("na,nb", [(1 << 16, (1 << 16) + 1), ((1 << 20) + 3, 1 << 19), (1 << 24, 1 << 24)])
def test_product_identity(L, na, nb):
    """a b at r equals a(r) b(r), up to 2^25 - 1 result coefficients"""
    from starks_amd.polynomial import mul_wire
    rnd = random.Random(na ^ nb)
    a, b = _rand_wire(rnd, na), _rand_wire(rnd, nb)
    c = mul_wire(a, b)
    assert len(c) == 32 * (na + nb - 1)
    r = rnd.randrange(P)
    assert _horner_wire(c, r) == _horner_wire(a, r) * _horner_wire(b, r) % P


@pytest.mark.parametrize("na,nb", [(1 << 24, 1 << 23), (1 << 24, 1 << 4), ((1 << 20) + 5, (1 << 19) - 3), (1 << 16, 1 << 17)])
def test_divmod_identity(L, na, nb):
    """a(r) = q(r) b(r) + rem(r), the remainder shorter than the divisor, up to 2^24-coefficient dividends"""
    from starks_amd.polynomial import divmod_wire
    rnd = random.Random(na + nb)
    a, b = _rand_wire(rnd, na), _rand_wire(rnd, nb)
    q, rem = divmod_wire(a, b)
    assert len(q) == 32 * max(na - nb + 1, 0) and len(rem) == 32 * min(na, nb - 1)
    x = rnd.randrange(P)
    assert _horner_wire(a, x) == (_horner_wire(q, x) * _horner_wire(b, x) + _horner_wire(rem, x)) % P


@pytest.mark.parametrize("n", [(1 << 16) - 1, 1 << 16, (1 << 16) + 1, 0b10110110101101011011, 1 << 20])
def test_zpoly_identity(L, n):
    """zpoly's value at r equals prod (r - x_i), n + 1 coefficients, leading 1, up to 2^20 points"""
    from starks_amd.poly_utils import zpoly_wire
    rnd = random.Random(n)
    xs = _rand_wire(rnd, n)
    z = zpoly_wire(xs)
    assert len(z) == 32 * (n + 1) and int.from_bytes(z[-32:], "big") == 1
    r = rnd.randrange(P)
    assert _horner_wire(z, r) == _prod_at(xs, r)


def _powers(g, n, h=1):
    out, v = [], h % P
    for _ in range(n):
        out.append(v)
        v = v * g % P
    return out


@pytest.mark.parametrize("lg", [16, 18, 20])
def test_lagrange_roots_of_unity(L, lg):
    """over the 2^lg-th roots of unity the interpolant is the inverse NTT of ys; over the coset h w^i it is that rescaled by h^-j"""
    from starks_amd import fft
    from starks_amd.poly_utils import lagrange_interp_wire
    n = 1 << lg
    w = pow(7, (P - 1) // n, P)
    rnd = random.Random(lg)
    ys = _rand_wire(rnd, n)
    want = fft.ntt_bytes(ys, n, w, inverse=True)
    assert lagrange_interp_wire(wire(_powers(w, n)), ys) == want
    if lg == 20:
        return
    h = rnd.randrange(2, P)
    got = ints(lagrange_interp_wire(wire(_powers(w, n, h)), ys))
    hinv = pow(h, P - 2, P)
    assert got == [c * s % P for c, s in zip(ints(want), _powers(hinv, n))]


def test_lagrange_arbitrary_points_2_20(L):
    """2^20 arbitrary x's: P(x_i) = y_i at 256 sampled i (the remainder of P by the samples' zpoly, evaluated on the host) plus four
    direct Horner evaluations, and degree < n"""
    from starks_amd.polynomial import divmod_wire
    from starks_amd.poly_utils import lagrange_interp_wire, zpoly_wire
    n = 1 << 20
    rnd = random.Random(20)
    xs, ys = _rand_wire(rnd, n), _rand_wire(rnd, n)
    p = lagrange_interp_wire(xs, ys)
    assert len(p) == 32 * n
    idx = rnd.sample(range(n), 256)
    x_of = lambda i: int.from_bytes(xs[32 * i:32 * i + 32], "big")  # noqa: E731
    y_of = lambda i: int.from_bytes(ys[32 * i:32 * i + 32], "big")  # noqa: E731
    sample_x = b"".join(xs[32 * i:32 * i + 32] for i in idx)
    _, rem = divmod_wire(p, zpoly_wire(sample_x))
    rem = ints(rem)
    for i in idx:
        assert horner(rem, x_of(i)) == y_of(i)
    for i in idx[:4]:
        assert _horner_wire(p, x_of(i)) == y_of(i)


def test_lazily_reduced_inputs(L):
    """wire values >= p give the results of their residues"""
    from starks_amd.polynomial import divmod_wire, mul_wire
    from starks_amd.poly_utils import lagrange_interp_wire, zpoly_wire
    rnd = random.Random(5)
    small = [rnd.randrange(2**256 - P) for _ in range(300)]
    lazy = wire([v + P for v in small])
    assert zpoly_wire(lazy) == zpoly_wire(wire(small))
    assert mul_wire(lazy, lazy[:3200]) == mul_wire(wire(small), wire(small[:100]))
    assert divmod_wire(lazy, lazy[:1600]) == divmod_wire(wire(small), wire(small[:50]))
    assert lagrange_interp_wire(lazy, wire([v + P for v in small[::-1]])) == lagrange_interp_wire(wire(small), wire(small[::-1]))


def test_errors_before_launch_and_empty(L):
    from starks_amd import _lib
    c = _lib.ctx()
    one = wire([1])
    buf = ctypes.create_string_buffer(64)
    INVALID = -1
    assert L.sh_poly_mul(c, one, (1 << 25) + 1, one, 1, buf) == INVALID
    assert L.sh_poly_mul(c, one, 1 << 24, one, (1 << 24) + 2, buf) == INVALID
    assert L.sh_poly_mul(c, one, 0, one, 1, buf) == 0  # empty operand: nothing to write
    assert L.sh_poly_divmod(c, one, 1, one, 0, buf, buf) == INVALID                  # divisor with no coefficients
    assert L.sh_poly_divmod(c, one, 1, wire([1, 0]), 2, buf, buf) == INVALID         # zero leading coefficient
    assert L.sh_poly_divmod(c, one, 1, wire([1, P]), 2, buf, buf) == INVALID         # ... lazily reduced
    assert L.sh_poly_divmod(c, one, (1 << 24) + 1, one, 1, buf, buf) == INVALID
    assert L.sh_zpoly(c, one, (1 << 20) + 1, buf) == INVALID
    assert L.sh_lagrange_interp(c, one, one, (1 << 20) + 1, buf) == INVALID
    assert L.sh_lagrange_interp(c, one, one, 0, buf) == 0
    assert L.sh_zpoly(c, b"", 0, buf) == 0 and ints(buf.raw[:32]) == [1]
    # device forms: an output overlapping an input is refused before any launch
    d = ctypes.c_void_p()
    _lib.check(L.sh_dev_alloc(c, 32 * 64, ctypes.byref(d)), "sh_dev_alloc")
    try:
        base = d.value
        assert L.sh_dev_poly_mul(c, ctypes.c_void_p(base), 8, ctypes.c_void_p(base + 32 * 8), 8, ctypes.c_void_p(base + 32 * 4)) == INVALID
        assert L.sh_dev_zpoly(c, ctypes.c_void_p(base), 8, ctypes.c_void_p(base + 32 * 7)) == INVALID
        assert L.sh_dev_lagrange_interp(c, ctypes.c_void_p(base), ctypes.c_void_p(base + 32 * 8), 8, ctypes.c_void_p(base + 32 * 15)) == INVALID
        assert L.sh_dev_poly_divmod(c, ctypes.c_void_p(base), 8, ctypes.c_void_p(base + 32 * 8), 4, ctypes.c_void_p(base + 32 * 9),
                                    ctypes.c_void_p(base + 32 * 40)) == INVALID
        _lib.check(L.sh_sync(c), "sh_sync")
    finally:
        L.sh_dev_free(c, d)


def test_device_forms_match_host_forms(L):
    """sh_dev_* in limb form on the ctx stream = the host-buffer forms"""
    from starks_amd import _lib
    from starks_amd.polynomial import divmod_wire
    from starks_amd.poly_utils import lagrange_interp_wire
    c = _lib.ctx()
    rnd = random.Random(9)
    n = 777
    xs, ys = _rand_wire(rnd, n), _rand_wire(rnd, n)
    d = ctypes.c_void_p()
    _lib.check(L.sh_dev_alloc(c, 32 * 4 * n, ctypes.byref(d)), "sh_dev_alloc")
    try:
        at = lambda k: ctypes.c_void_p(d.value + 32 * k * n)  # noqa: E731
        _lib.check(L.sh_dev_from_wire(c, xs, at(0), n), "from_wire")
        _lib.check(L.sh_dev_from_wire(c, ys, at(1), n), "from_wire")
        _lib.check(L.sh_dev_lagrange_interp(c, at(0), at(1), n, at(2)), "sh_dev_lagrange_interp")
        out = ctypes.create_string_buffer(32 * n)
        _lib.check(L.sh_dev_to_wire(c, at(2), out, n), "to_wire")
        assert out.raw == lagrange_interp_wire(xs, ys)
        _lib.check(L.sh_dev_poly_divmod(c, at(0), n, at(1), 100, at(2), at(3)), "sh_dev_poly_divmod")
        q = ctypes.create_string_buffer(32 * (n - 99))
        r = ctypes.create_string_buffer(32 * 99)
        _lib.check(L.sh_dev_to_wire(c, at(2), q, n - 99), "to_wire")
        _lib.check(L.sh_dev_to_wire(c, at(3), r, 99), "to_wire")
        assert (q.raw, r.raw) == divmod_wire(xs, ys[:3200])
    finally:
        L.sh_dev_free(c, d)


def test_two_contexts_same_bytes(L):
    """a second context (its own stream, plans and workspaces) computes the same bytes, once"""
    from starks_amd import _lib
    from starks_amd.poly_utils import lagrange_interp_wire
    rnd = random.Random(11)
    n = (1 << 14) + 3
    xs, ys = _rand_wire(rnd, n), _rand_wire(rnd, n)
    out = ctypes.create_string_buffer(32 * n)
    _lib.check(L.sh_lagrange_interp(_lib.second_ctx(), xs, ys, n, out), "sh_lagrange_interp (second context)")
    assert out.raw == lagrange_interp_wire(xs, ys)
