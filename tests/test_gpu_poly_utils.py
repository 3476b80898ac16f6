"""Batch inversion and four-point interpolation on the MI355X (sh_dev_multi_inv / sh_multi_inv, sh_dev_multi_interp_4 /
sh_multi_interp_4, starks_amd.poly_utils; csrc/multi_inv.hip): byte-identical to tests/golden/poly_utils.json, exact at every tile and
level boundary from one element to 2^26, and invariant under in-place calls, lazily reduced inputs, concatenation and stream order."""
import ctypes
import hashlib
import random

import pytest

from conftest import load_golden
from poly_utils_cases import interp_restated, mimc_inputs, wire

pytestmark = pytest.mark.gpu

P = 2**256 - 2**32 * 351 + 1
T = 1024          # IV_LANES * IV_CHUNK
G = load_golden("poly_utils.json")


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def _ctx():
    from starks_amd import _lib
    return _lib.ctx()


def _ok(rc, where):
    from starks_amd import _lib
    _lib.check(rc, where)


class Dev(object):
    """a device buffer of n limb-form elements"""

    def __init__(self, L, n):
        self.L, self.n, self.p = L, n, ctypes.c_void_p()
        _ok(L.sh_dev_alloc(_ctx(), 32 * max(n, 1), ctypes.byref(self.p)), "sh_dev_alloc")

    def at(self, i):
        return ctypes.c_void_p(self.p.value + 32 * i)

    def get(self, i):
        b = ctypes.create_string_buffer(32)
        _ok(self.L.sh_dev_download(_ctx(), self.at(i), b, 32), "sh_dev_download")
        return int.from_bytes(b.raw, "little")

    def put(self, i, v):
        _ok(self.L.sh_dev_upload(_ctx(), int(v).to_bytes(32, "little"), self.at(i), 32), "sh_dev_upload")

    def chunks(self, step=1 << 22):
        buf = ctypes.create_string_buffer(32 * min(step, max(self.n, 1)))
        for a in range(0, self.n, step):
            k = min(step, self.n - a)
            _ok(self.L.sh_dev_download(_ctx(), self.at(a), buf, 32 * k), "sh_dev_download")
            yield buf.raw[:32 * k]

    def free(self):
        self.L.sh_dev_free(_ctx(), self.p)


def _inv(L, src, dst, n=None):
    _ok(L.sh_dev_multi_inv(_ctx(), src.p, dst.p, src.n if n is None else n), "sh_dev_multi_inv")


def _host_inv(v):
    return pow(v % P, P - 2, P)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
def test_golden_multi_inv(L):
    from starks_amd import IntegersModP
    from starks_amd.poly_utils import multi_inv, multi_inv_wire
    F = IntegersModP(P)
    for c in G["mimc"]:
        vals = mimc_inputs(c)
        out = ctypes.create_string_buffer(32 * len(vals))
        _ok(L.sh_multi_inv(_ctx(), wire(vals), len(vals), out), "sh_multi_inv")
        assert hashlib.sha256(out.raw).hexdigest() == c["out_ints_sha"], c["name"]
        assert multi_inv_wire(wire(vals)) == out.raw
        # the Python API keeps the reference's semantics per input type: a zero int -> 0, a zero field element -> 1
        got_ints = multi_inv(F, vals)
        got_elems = multi_inv(F, [F(v) for v in vals])
        assert hashlib.sha256(got_ints.wire_bytes()).hexdigest() == c["out_ints_sha"], c["name"]
        assert hashlib.sha256(got_elems.wire_bytes()).hexdigest() == c["out_elems_sha"], c["name"]
        if "out_elems" in c:
            assert [int(v) for v in got_elems] == [int(v, 16) for v in c["out_elems"]]
            assert [int(v) for v in got_ints] == [int(v, 16) for v in c["out_ints"]]


def test_golden_multi_interp_4(L):
    from starks_amd import IntegersModP
    from starks_amd.poly_utils import multi_interp_4, multi_interp_4_wire
    F = IntegersModP(P)
    for c in [x for x in G["interp"] if x["p"] == P]:
        xs = [[int(v, 16) for v in r] for r in c["xs"]]
        ys = [[int(v, 16) for v in r] for r in c["ys"]]
        rows = len(xs)
        out = ctypes.create_string_buffer(128 * rows)
        _ok(L.sh_multi_interp_4(_ctx(), wire(sum(xs, [])), wire(sum(ys, [])), rows, out), "sh_multi_interp_4")
        want = interp_restated(xs, ys, P)
        assert out.raw == wire(sum(want, []))
        assert multi_interp_4_wire(wire(sum(xs, [])), wire(sum(ys, [])), rows) == out.raw
        polys = multi_interp_4(F, [[F(v) for v in r] for r in xs], [[F(v) for v in r] for r in ys])
        assert [[int(v) for v in p.coefficients] for p in polys] == [[int(v, 16) for v in r] for r in c["coeffs"]], c["name"]


def test_arguments(L):
    a, b = Dev(L, 8), Dev(L, 8)
    try:
        assert L.sh_dev_multi_inv(None, a.p, b.p, 8) == -1
        assert L.sh_dev_multi_inv(_ctx(), None, b.p, 8) == -1
        assert L.sh_dev_multi_inv(_ctx(), a.p, None, 8) == -1
        assert L.sh_dev_multi_inv(_ctx(), a.p, a.at(1), 4) == -1          # partial overlap
        assert L.sh_dev_multi_inv(_ctx(), a.p, b.p, 0) == 0              # nothing to do
        assert L.sh_dev_multi_interp_4(_ctx(), a.p, b.p, 2, a.at(1)) == -1
        assert L.sh_dev_multi_interp_4(_ctx(), a.p, b.p, 0, b.p) == 0
        assert L.sh_multi_inv(_ctx(), None, 1, ctypes.create_string_buffer(32)) == -1
        assert L.sh_multi_interp_4(_ctx(), b"\0" * 128, None, 1, ctypes.create_string_buffer(128)) == -1
    finally:
        a.free()
        b.free()


# ---- sizes: boundaries, random indices, the round trip, planted zeros ------------------------------------------------------------
def _boundaries(n):
    idx = set()
    t = T
    while t < T * n:  # both sides of the edge of every tile of every level
        for k in range(0, n + t, t):
            idx.update(i for i in (k - 1, k, k + 1) if 0 <= i < n)
        t *= T
    return idx


@pytest.mark.parametrize("n", [1, 3, T - 1, T, T + 1, T * T + 1, 3 * 2**22 + 5, 2**26])
def test_sizes(L, n):
    rnd = random.Random(n)
    x, y, z = Dev(L, n), Dev(L, n), Dev(L, n)
    try:
        _ok(L.sh_dev_fill_seeded(_ctx(), x.p, n, 77), "sh_dev_fill_seeded")
        zeros = sorted({0, n - 1, n // 2, rnd.randrange(n)} if n > 3 else {n - 1})
        for i in zeros:
            x.put(i, 0)
        _inv(L, x, y)
        _inv(L, y, z)
        idx = sorted(_boundaries(n) | {rnd.randrange(n) for _ in range(4096)})
        k, a, checked = 0, 0, 0
        for xc, yc, zc in zip(x.chunks(), y.chunks(), z.chunks()):
            assert xc == zc  # multi_inv(multi_inv(x)) == x (x is canonical), byte for byte
            end = a + len(xc) // 32
            while k < len(idx) and idx[k] < end:
                i = idx[k] - a
                xi, yi = int.from_bytes(xc[32 * i:32 * i + 32], "little"), int.from_bytes(yc[32 * i:32 * i + 32], "little")
                assert yi == (pow(xi, P - 2, P) if xi else 0), idx[k]
                k, checked = k + 1, checked + 1
            a = end
        assert checked == len(idx)
        for i in zeros:
            assert y.get(i) == 0
    finally:
        for d in (x, y, z):
            d.free()


# ---- invariances ------------------------------------------------------------------------------------------------------------------
def test_in_place_equals_out_of_place(L):
    n = T * T + 17
    x, y = Dev(L, n), Dev(L, n)
    try:
        _ok(L.sh_dev_fill_seeded(_ctx(), x.p, n, 5), "sh_dev_fill_seeded")
        x.put(3, 0)
        _inv(L, x, y)
        _inv(L, x, x)
        assert list(x.chunks()) == list(y.chunks())
    finally:
        x.free()
        y.free()


def test_lazily_reduced_inputs(L):
    """x + p (< 2^256) in the limbs gives the bytes of x"""
    rnd = random.Random(3)
    n = 5 * T + 3
    vals = [rnd.randrange(2**256 - P) for _ in range(n)]
    vals[7] = 0
    x, xr, y, yr = Dev(L, n), Dev(L, n), Dev(L, n), Dev(L, n)
    try:
        _ok(L.sh_dev_upload(_ctx(), b"".join(v.to_bytes(32, "little") for v in vals), x.p, 32 * n), "sh_dev_upload")
        _ok(L.sh_dev_upload(_ctx(), b"".join((v + P).to_bytes(32, "little") for v in vals), xr.p, 32 * n), "sh_dev_upload")
        _inv(L, x, y)
        _inv(L, xr, yr)
        assert list(y.chunks()) == list(yr.chunks())
        assert y.get(7) == 0 and y.get(8) == _host_inv(vals[8])
    finally:
        for d in (x, xr, y, yr):
            d.free()


def test_concatenation(L):
    from starks_amd.poly_utils import multi_inv_wire
    rnd = random.Random(4)
    a = [rnd.randrange(P) for _ in range(3 * T + 1)] + [0]
    b = [0, P] + [rnd.randrange(P) for _ in range(T * 2 - 7)]
    assert multi_inv_wire(wire(a + b)) == multi_inv_wire(wire(a)) + multi_inv_wire(wire(b))


def test_queued_behind_an_ntt(L):
    """sh_dev_ntt then sh_dev_multi_inv on its output with no synchronisation in between"""
    from starks_amd.poly_utils import multi_inv_wire
    n = 1 << 20
    x, y, z = Dev(L, n), Dev(L, n), Dev(L, n)
    try:
        _ok(L.sh_dev_fill_seeded(_ctx(), x.p, n, 9), "sh_dev_fill_seeded")
        root = pow(7, (P - 1) // n, P).to_bytes(32, "big")
        _ok(L.sh_dev_ntt(_ctx(), x.p, y.p, n, 1, root, 0), "sh_dev_ntt")
        _inv(L, y, z)
        got = b"".join(z.chunks())
        ys = b"".join(y.chunks())
        want = multi_inv_wire(b"".join(ys[i:i + 32][::-1] for i in range(0, len(ys), 32)))
        assert b"".join(got[i:i + 32][::-1] for i in range(0, len(got), 32)) == want
    finally:
        for d in (x, y, z):
            d.free()


# ---- multi_interp_4 at 2^18 rows --------------------------------------------------------------------------------------------------
def test_multi_interp_4_2_18_rows(L):
    from starks_amd.poly_utils import multi_interp_4_wire
    rows = 1 << 18
    rnd = random.Random(18)
    xs = [[rnd.randrange(P) for _ in range(4)] for _ in range(rows)]
    ys = [[rnd.randrange(P) for _ in range(4)] for _ in range(rows)]
    degenerate = set(range(0, rows, 97))
    for r in degenerate:
        xs[r][(r // 97) % 3 + 1] = xs[r][0]
    raw = multi_interp_4_wire(wire(v for r in xs for v in r), wire(v for r in ys for v in r), rows)
    c = [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]
    for r in range(rows):
        cr = c[4 * r:4 * r + 4]
        if r in degenerate:
            assert cr == interp_restated([xs[r]], [ys[r]], P)[0], r
            continue
        for x, y in zip(xs[r], ys[r]):
            assert ((cr[3] * x + cr[2]) * x + cr[1]) * x % P == (y - cr[0]) % P, r
