"""Polynomial evaluation at arbitrary points on the MI355X (sh_poly_eval, sh_dev_poly_eval; starks_amd.polynomial.eval_wire,
poly_utils.multi_eval, Polynomial.__call__; csrc/poly_eval.hip): byte-identical to tests/golden/poly_eval.json, exact against
Python-int Horner up to n m = 2^22, both forced paths (STARKHIP_EVAL_PATH) byte-identical on both sides of the default crossover,
and at size against results pinned elsewhere: the NTT at the roots of unity and on a coset, lagrange_interp's values, zpoly's
roots, and eval(a b) = eval(a) eval(b), up to every limit."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden
from poly_arith_cases import P, horner, ints, operand, seeded, wire

pytestmark = pytest.mark.gpu

G = load_golden("poly_eval.json")


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def _ctx():
    from starks_amd import _lib
    return _lib.ctx()


def _ck(rc, where):
    from starks_amd import _lib
    _lib.check(rc, where)


class Dev(object):
    """device buffers of fp elements, freed together"""

    def __init__(self, L):
        self.L, self.bufs = L, []

    def alloc(self, n):
        p = ctypes.c_void_p()
        _ck(self.L.sh_dev_alloc(_ctx(), 32 * max(n, 1), ctypes.byref(p)), "sh_dev_alloc")
        self.bufs.append(p)
        return p

    def seeded(self, n, seed):
        p = self.alloc(n)
        _ck(self.L.sh_dev_fill_seeded(_ctx(), p, n, seed), "fill")
        return p

    def upload(self, raw):
        p = self.alloc(len(raw) // 32)
        _ck(self.L.sh_dev_from_wire(_ctx(), raw, p, len(raw) // 32), "from_wire")
        return p

    def download(self, p, n, k=0):
        out = ctypes.create_string_buffer(32 * max(n, 1))
        _ck(self.L.sh_dev_to_wire(_ctx(), at(p, k), out, n), "to_wire")
        return out.raw[:32 * n]

    def free(self):
        for p in self.bufs:
            self.L.sh_dev_free(_ctx(), p)
        self.bufs = []


def at(p, k):
    return ctypes.c_void_p(p.value + 32 * k)


@pytest.fixture
def dev(L):
    d = Dev(L)
    yield d
    d.free()


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


def _root(n):
    return pow(7, (P - 1) // n, P)


def _eval_dev(L, dev, d_coefs, n, batch, xs_raw):
    m = len(xs_raw) // 32
    d_xs, d_out = dev.upload(xs_raw), dev.alloc(batch * m)
    _ck(L.sh_dev_poly_eval(_ctx(), d_coefs, n, batch, d_xs, m, d_out), "sh_dev_poly_eval")
    return dev.download(d_out, batch * m)


def _ntt_dev(L, dev, d_coefs, n, batch=1):
    d_out = dev.alloc(batch * n)
    _ck(L.sh_dev_ntt(_ctx(), d_coefs, d_out, n, batch, _root(n).to_bytes(32, "big"), 0), "sh_dev_ntt")
    return d_out


def _powers(x, count, start=1):
    out, v = [], start % P
    for _ in range(count):
        out.append(v)
        v = v * x % P
    return out


def _words(raw, idx):
    mv = memoryview(raw)
    return b"".join(bytes(mv[32 * i:32 * i + 32]) for i in idx)


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------------
def test_fixture_bytes(L):
    from starks_amd.polynomial import eval_wire
    for c in G["eval"]:
        assert eval_wire(wire(operand(c["coefs"])), wire(operand(c["xs"]))) == wire(c["out"]), c["name"]


def test_fixture_python_api(L):
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    from starks_amd.poly_utils import multi_eval
    F = IntegersModP(P)
    Poly = polynomials_over(F)
    for c in G["eval"]:
        got = multi_eval(F, Poly(operand(c["coefs"])), operand(c["xs"]))
        assert [int(v) for v in got] == c["out"], c["name"]
        assert all(isinstance(v, F) for v in got)


# ---- 2. exact against Python ints; both paths ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,batch", [(1, 1, 1), (3, 5, 2), (257, 3, 1), (4096, 1024, 1), (1 << 16, 64, 1), (1000, 4096, 1),
                                       (1 << 14, 16, 4), (65, 1 << 10, 3)])
def test_exact_vs_horner(L, n, m, batch):
    from starks_amd.polynomial import eval_wire
    rnd = random.Random(n * 131 + m + batch)
    coefs, xs = _rand_wire(rnd, batch * n), bytearray(_rand_wire(rnd, m))
    if m > 3:
        xs[32:64] = bytes(32)  # x = 0
        xs[64:96] = xs[96:128]  # a repeated x
    xs = bytes(xs)
    got = ints(eval_wire(coefs, xs, batch))
    want = [_horner_wire(coefs[32 * n * b:32 * n * (b + 1)], x) for b in range(batch) for x in ints(xs)]
    assert got == want


PARITY_CASES = [(1 << 16, 1 << 16, 1), (1 << 14, 1 << 10, 1), (1 << 15, 1 << 13, 1), (1 << 16, 1 << 13, 1), (1 << 12, 1 << 12, 2),
                (5000, 300, 3), (1 << 16, 16, 1), (100, 1 << 16, 1)]


def _parity_digests():
    """sha256 of sh_poly_eval's output for every PARITY_CASES entry (run in a child process with the path forced)"""
    from starks_amd.polynomial import eval_wire
    res = []
    for n, m, batch in PARITY_CASES:
        rnd = random.Random(n + 3 * m + batch)
        res.append(hashlib.sha256(eval_wire(_rand_wire(rnd, batch * n), _rand_wire(rnd, m), batch)).hexdigest())
    return res


def test_forced_paths_same_bytes(L):
    """STARKHIP_EVAL_PATH=direct and =tree give the same bytes as the default choice, up to n = m = 2^16 and on both sides of the
    default crossover ((2^15, 2^13) goes direct and (2^16, 2^13) to the tree by include/starkhip.h's rule), each in a child
    process"""
    code = "import sys, json; sys.path[:0] = [%r, %r]; import test_gpu_poly_eval as t; print(json.dumps(t._parity_digests()))" % (
        ROOT, os.path.join(ROOT, "tests"))
    outs = {}
    for path in ("direct", "tree"):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, STARKHIP_EVAL_PATH=path), cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[path] = json.loads(r.stdout.strip().splitlines()[-1])
    assert outs["direct"] == outs["tree"] == _parity_digests()


def test_forced_paths_fixture(L):
    """the fixture and the exact cases with each path forced"""
    for path in ("direct", "tree"):
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_poly_eval.py"), "-q", "-x", "-m", "gpu",
                            "-k", "test_fixture_bytes or test_exact_vs_horner", "-p", "no:cacheprovider"], capture_output=True, text=True,
                           timeout=600, env=dict(os.environ, STARKHIP_EVAL_PATH=path), cwd=ROOT)
        assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


# ---- 3. at size, against results pinned elsewhere --------------------------------------------------------------------------------
@pytest.mark.parametrize("lg", [16, 20, 24])
def test_roots_of_unity_equal_ntt(L, dev, lg):
    """P at w^k equals the NTT of P's coefficients at k: every point up to 2^20, 2^10 of them at 2^24"""
    n = 1 << lg
    d_c = dev.seeded(n, 40 + lg)
    ntt = dev.download(_ntt_dev(L, dev, d_c, n), n)
    w = _root(n)
    idx = list(range(n)) if n <= 1 << 20 else sorted(random.Random(lg).sample(range(n), 1 << 10))
    xs = wire(_powers(w, n) if len(idx) == n else [pow(w, k, P) for k in idx])
    assert _eval_dev(L, dev, d_c, n, 1, xs) == (ntt if len(idx) == n else _words(ntt, idx))


@pytest.mark.parametrize("lg", [16, 20])
def test_coset_equals_scaled_ntt(L, dev, lg):
    """P at g w^k equals the NTT of c_k g^k"""
    n, g = 1 << lg, 7
    coefs = [seeded(60 + lg, i) % P for i in range(n)]
    scaled, gk = [], 1
    for c in coefs:
        scaled.append(c * gk % P)
        gk = gk * g % P
    ntt = dev.download(_ntt_dev(L, dev, dev.upload(wire(scaled)), n), n)
    w = _root(n)
    xs = _powers(w, min(n, 1 << 16), g)
    assert _eval_dev(L, dev, dev.upload(wire(coefs)), n, 1, wire(xs)) == ntt[:32 * len(xs)]


def test_max_coefs_subset_of_roots(L, dev):
    """n = 2^25 (the limit) at 2^8 of the 2^25-th roots of unity"""
    n = 1 << 25
    d_c = dev.seeded(n, 71)
    ntt_d = _ntt_dev(L, dev, d_c, n)
    idx = sorted(random.Random(25).sample(range(n), 256))
    want = b"".join(dev.download(ntt_d, 1, k) for k in idx)
    w = _root(n)
    assert _eval_dev(L, dev, d_c, n, 1, wire([pow(w, k, P) for k in idx])) == want


@pytest.mark.parametrize("lg", [16, 18, 20])
def test_lagrange_interp_values(L, dev, lg):
    """lagrange_interp(xs, ys) at xs gives ys"""
    n = 1 << lg
    d_x, d_y, d_p = dev.seeded(n, 80 + lg), dev.seeded(n, 90 + lg), dev.alloc(n)
    _ck(L.sh_dev_lagrange_interp(_ctx(), d_x, d_y, n, d_p), "lagrange")
    d_v = dev.alloc(n)
    _ck(L.sh_dev_poly_eval(_ctx(), d_p, n, 1, d_x, n, d_v), "eval")
    assert dev.download(d_v, n) == dev.download(d_y, n)


@pytest.mark.parametrize("n", [1 << 10, 1 << 16, 1 << 20])
def test_zpoly_roots(L, dev, n):
    """zpoly(xs) (n + 1 coefficients: two chunks of the tree path) is 0 at every x_i"""
    d_x, d_z = dev.seeded(n, 100 + n.bit_length()), dev.alloc(n + 1)
    _ck(L.sh_dev_zpoly(_ctx(), d_x, n, d_z), "zpoly")
    d_v = dev.alloc(n)
    _ck(L.sh_dev_poly_eval(_ctx(), d_z, n + 1, 1, d_x, n, d_v), "eval")
    assert dev.download(d_v, n) == bytes(32 * n)


@pytest.mark.parametrize("na,nb", [(1000, 17), (1 << 20, (1 << 20) + 1), (1 << 24, (1 << 24) + 1)])
def test_eval_of_product(L, dev, na, nb):
    """eval(a b) = eval(a) eval(b) at 64 random points, up to n_a + n_b - 1 = 2^25"""
    d_a, d_b, d_ab = dev.seeded(na, 110), dev.seeded(nb, 111), dev.alloc(na + nb - 1)
    _ck(L.sh_dev_poly_mul(_ctx(), d_a, na, d_b, nb, d_ab), "mul")
    xs = _rand_wire(random.Random(na), 64)
    va, vb = ints(_eval_dev(L, dev, d_a, na, 1, xs)), ints(_eval_dev(L, dev, d_b, nb, 1, xs))
    assert ints(_eval_dev(L, dev, d_ab, na + nb - 1, 1, xs)) == [a * b % P for a, b in zip(va, vb)]


# ---- 4, 5. limits, batches and forms ------------------------------------------------------------------------------------------------
def test_max_batch_total(L, dev):
    """batch n = 2^26 (4 x 2^24) at 2^7 of the 2^24-th roots equals the batched NTT; batch = 4 equals four single calls"""
    n, batch = 1 << 24, 4
    d_c = dev.seeded(batch * n, 120)
    ntt_d = _ntt_dev(L, dev, d_c, n, batch)
    idx = sorted(random.Random(7).sample(range(n), 128))
    w = _root(n)
    xs = wire([pow(w, k, P) for k in idx])
    got = _eval_dev(L, dev, d_c, n, batch, xs)
    assert got == b"".join(dev.download(ntt_d, 1, b * n + k) for b in range(batch) for k in idx)
    assert got == b"".join(_eval_dev(L, dev, at(d_c, b * n), n, 1, xs) for b in range(batch))


def test_max_points_four_chunks(L, dev):
    """m = 2^20 points with n = 2^22 (C = 4 chunks): the odd 2^22-th roots w^(4k + 1) against the size-2^22 NTT"""
    n, m = 1 << 22, 1 << 20
    d_c = dev.seeded(n, 130)
    ntt = dev.download(_ntt_dev(L, dev, d_c, n), n)
    w = _root(n)
    xs = _powers(pow(w, 4, P), m, w)
    assert _eval_dev(L, dev, d_c, n, 1, wire(xs)) == _words(ntt, range(1, n, 4))


def test_dev_equals_host_form(L, dev):
    from starks_amd.polynomial import eval_wire
    rnd = random.Random(9)
    for n, m, batch in [(300, 70, 3), (1 << 15, 5, 2), (7, 1 << 12, 1)]:
        coefs, xs = _rand_wire(rnd, batch * n), _rand_wire(rnd, m)
        assert _eval_dev(L, dev, dev.upload(coefs), n, batch, xs) == eval_wire(coefs, xs, batch)


def test_zero_and_empty(L, dev):
    from starks_amd.polynomial import eval_wire
    assert eval_wire(b"", wire([0, 1, 5]), 1) == bytes(96)
    assert eval_wire(b"", wire([3]), 4) == bytes(128)
    assert eval_wire(wire([1, 2]), b"") == b""
    sentinel = b"\x5a" * 64
    out = ctypes.create_string_buffer(sentinel, 64)
    _ck(L.sh_poly_eval(_ctx(), wire([1, 2, 3]), 3, 1, b"", 0, out), "m = 0")
    assert out.raw[:64] == sentinel


# ---- 6. errors, before anything is launched ---------------------------------------------------------------------------------------
def test_errors_before_launch(L, dev):
    c = _ctx()
    SH_ERR_INVALID, SH_ERR_UNSUPPORTED = _codes()
    coefs, xs = wire([1, 2, 3, 4]), wire([5, 6])
    sentinel = b"\xa5" * 64
    out = ctypes.create_string_buffer(sentinel, 64)
    assert L.sh_poly_eval(None, coefs, 4, 1, xs, 2, out) == SH_ERR_INVALID
    assert L.sh_poly_eval(c, None, 4, 1, xs, 2, out) == SH_ERR_INVALID
    assert L.sh_poly_eval(c, coefs, 4, 1, None, 2, out) == SH_ERR_INVALID
    assert L.sh_poly_eval(c, coefs, 4, 1, xs, 2, None) == SH_ERR_INVALID
    assert L.sh_poly_eval(c, coefs, 4, 0, xs, 2, out) == SH_ERR_INVALID
    assert L.sh_poly_eval(c, coefs, (1 << 25) + 1, 1, xs, 2, out) == SH_ERR_UNSUPPORTED
    assert L.sh_poly_eval(c, coefs, 1 << 24, 5, xs, 2, out) == SH_ERR_UNSUPPORTED
    assert L.sh_poly_eval(c, coefs, 4, 1, xs, (1 << 20) + 1, out) == SH_ERR_UNSUPPORTED
    assert out.raw[:64] == sentinel
    d_c, d_x, d_o = dev.seeded(64, 1), dev.seeded(8, 2), dev.alloc(64)
    _ck(L.sh_dev_fill_seeded(c, d_o, 64, 3), "fill")
    before = dev.download(d_o, 64)
    assert L.sh_dev_poly_eval(c, d_c, 64, 1, d_x, 8, at(d_c, 60)) == SH_ERR_INVALID  # out overlaps the coefficients
    assert L.sh_dev_poly_eval(c, d_c, 8, 1, d_o, 8, at(d_o, 4)) == SH_ERR_INVALID  # out overlaps the points
    assert L.sh_dev_poly_eval(c, d_c, 8, 0, d_x, 8, d_o) == SH_ERR_INVALID
    assert L.sh_dev_poly_eval(c, d_c, 1 << 26, 1, d_x, 8, d_o) == SH_ERR_UNSUPPORTED
    assert L.sh_dev_poly_eval(c, None, 8, 1, d_x, 8, d_o) == SH_ERR_INVALID
    _ck(L.sh_sync(c), "sync")
    assert dev.download(d_o, 64) == before


def _codes():
    src = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    import re
    get = lambda name: int(re.search(r"%s\s*=\s*(-?\d+)" % name, src).group(1))  # noqa: E731
    return get("SH_ERR_INVALID"), get("SH_ERR_UNSUPPORTED")


# ---- 7. Polynomial.__call__ ------------------------------------------------------------------------------------------------------------
def test_call_on_device_backed_polynomial(L, monkeypatch):
    """__call__ on a WireList-backed 2^20-coefficient polynomial runs on the device and equals the NTT at that root; host-built
    polynomials and short ones keep the host loop"""
    from starks_amd import IntegersModP, fft, polynomial
    from starks_amd.wireseq import WireList
    F = IntegersModP(P)
    Poly = polynomial.polynomials_over(F)
    n = 1 << 20
    raw = _rand_wire(random.Random(20), n)
    p = Poly(WireList(raw, F))
    w = _root(n)
    ntt = fft.ntt_bytes(raw, n, w)
    calls = []
    real = polynomial.eval_wire
    monkeypatch.setattr(polynomial, "eval_wire", lambda *a, **k: calls.append(1) or real(*a, **k))
    for k in (0, 1, 5, n - 1):
        v = p(pow(w, k, P))
        assert isinstance(v, F) and int(v) == int.from_bytes(ntt[32 * k:32 * k + 32], "big")
    assert int(p(F(pow(w, 3, P)))) == int.from_bytes(ntt[96:128], "big")
    assert len(calls) == 5
    small = Poly(WireList(raw[:32 * 8], F))
    assert int(small(3)) == horner(ints(raw[:256]), 3) and len(calls) == 5
    q = Poly([1, 2, 3])
    assert int(q(2)) == 17 and len(calls) == 5
