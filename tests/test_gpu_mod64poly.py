"""Polynomial products, division, zpoly, lagrange_interp, multi_inv and multi_interp_4 over any prime modulus below 2^64 on packed 64-bit
words on the MI355X (the sh_mod64_* / sh_dev_mod64_* entries of include/starkhip.h; csrc/mod64poly.hip, api_mod64poly.hip; the
mod64_*_words forms of starks_amd.polynomial and poly_utils): word for word the outputs recorded in tests/golden/mod_poly.json, the
same from a child process whose transforms all run several passes, equal to the 32-byte sh_mod_* entries on the same values, exact
against Python ints at the small sizes, the batch inversion at the level boundaries of its tiles, every refusal with its status and
the entry's name, two contexts interleaved with 32-byte and MiMC calls, and the Python forms.  All comparisons are exact."""
import ctypes
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import mod64poly_cases as mc  # noqa: E402
from mod64poly_cases import IDS, unwords, words  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, ROOT_ORDER, UNSUPPORTED = -1, -2, -6
FIELDS3 = [mc.GOLDILOCKS, mc.P63, mc.BABYBEAR]
IV_T, ROW_T = 2048, 1024  # the tiles the implementation kept (mod64poly_items.cuh: M6P_IV_LANES x M6P_IV_CHUNK, x M6P_IV_ROW_CHUNK)
FULL = 2**64 - 1


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


@pytest.fixture(scope="module")
def G():
    return mc.resolved(load_golden("mod_poly.json"))


def _args(p, root=None):
    from starks_amd import _lib
    return _lib.mod64_poly_args(p, root)


def _err(L, c=None):
    from starks_amd import _lib
    return L.sh_last_error(c or _lib.ctx()).decode()


def _rand_words(rnd, n):
    """n random 64-bit words as bytes, fast (any 64-bit word is an input: the entries take it mod p)"""
    import numpy as np
    return np.random.default_rng(rnd.getrandbits(64)).integers(0, 2**64, size=n, dtype=np.uint64).tobytes()


def _to_wire(raw):
    """native words -> the 32-byte big-endian values of the same integers"""
    import numpy as np
    a = np.frombuffer(bytes(raw), dtype="=u8")
    out = np.zeros((len(a), 32), dtype=np.uint8)
    out[:, 24:] = a.astype(">u8").view(np.uint8).reshape(len(a), 8)
    return out.tobytes()


def _from_wire(raw):
    """32-byte big-endian values below 2^64 -> native words"""
    import numpy as np
    a = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 32)
    assert not a[:, :24].any()
    return np.ascontiguousarray(a[:, 24:]).view(">u8").astype("=u8").tobytes()


def _horner(p, raw, x):
    y = 0
    for c in reversed(unwords(raw)):
        y = (y * x + c) % p
    return y


# ---- the fixture through the Python word forms (host forms) --------------------------------------------------------------------------
def _fixture_outputs(c, as_bytes=False):
    """every output of a fixture case through the Python word forms, as lists of ints"""
    from starks_amd.polynomial import mod64_divmod_words, mod64_mul_words
    from starks_amd.poly_utils import (mod64_lagrange_interp_words, mod64_multi_interp_4_words, mod64_multi_inv_words,
                                       mod64_zpoly_words)
    p, op = c["p"], c["op"]
    f = {k: (words(p, v) if as_bytes else v) for k, v in mc.fixture_words(p, c).items()}
    if op == "mul":
        return [list(mod64_mul_words(p, f["a"], f["b"]))]
    if op == "divmod":
        return [list(x) for x in mod64_divmod_words(p, f["a"], f["b"])]
    if op == "zpoly":
        return [list(mod64_zpoly_words(p, f["xs"]))]
    if op == "lagrange":
        return [list(mod64_lagrange_interp_words(p, f["xs"], f["ys"]))]
    if op == "multi_inv":
        return [list(mod64_multi_inv_words(p, f["in"]))]
    return [list(mod64_multi_interp_4_words(p, f["xs"], f["ys"]))]


@pytest.mark.parametrize("p", mc.FIXTURE_MODULI, ids=IDS.get)
def test_fixture_host_forms(L, G, p):
    """the recorded outputs over IntegersModP(p) through the host-buffer forms, operands given as lists and as bytes"""
    mine = [c for c in G if c["p"] == p]
    assert len(mine) == (38 if p == 97 else 57)
    for i, c in enumerate(mine):
        for rec, got in zip(mc.recorded(c), mc.normal(c, _fixture_outputs(c, as_bytes=i % 2 == 1))):
            assert mc.matches(rec, got), (c["op"], c["name"])


def _digest(cases):
    h = hashlib.sha256()
    for c in cases:
        for got in _fixture_outputs(c):
            h.update(words(c["p"], got) + b"|")
    return h.hexdigest()


def test_fixture_with_multi_pass_plans(L, G):
    """STARKHIP_MOD64_TILE_LOG=4 in a fresh child process: every transform above 4 points runs several passes, so every tree level
    does; the child's digest of the fixture equals this process's"""
    cases = [c for c in G if c["p"] in mc.FIXTURE_MODULI]
    env = dict(os.environ, STARKHIP_MOD64_TILE_LOG="4")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "tile-child"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == _digest(cases)


# ---- device forms --------------------------------------------------------------------------------------------------------------------
class Dev(object):
    """a device buffer of native words"""

    def __init__(self, L, c, elems):
        from starks_amd import _lib
        self.L, self.c, self.d, self._lib = L, c, ctypes.c_void_p(), _lib
        _lib.check(L.sh_dev_alloc(c, 8 * max(elems, 1), ctypes.byref(self.d)), "sh_dev_alloc")

    def at(self, k):
        return ctypes.c_void_p(self.d.value + 8 * k)

    def put(self, k, vals):
        raw = vals if isinstance(vals, (bytes, bytearray)) else words(3, vals)
        if raw:
            self._lib.check(self.L.sh_dev_upload(self.c, bytes(raw), self.at(k), len(raw)), "sh_dev_upload")

    def get(self, k, n):
        buf = ctypes.create_string_buffer(8 * max(n, 1))
        if n:
            self._lib.check(self.L.sh_dev_download(self.c, self.at(k), buf, 8 * n), "sh_dev_download")
        return unwords(buf.raw[:8 * n])

    def free(self):
        self.L.sh_dev_free(self.c, self.d)


def _dev_case(L, ctx, p, op, shift=0, **f):
    """one call of a device form on words (any 64-bit values), the outputs as ints; the output area is poisoned first.  shift = 1
    puts the first operand and the outputs on addresses that are 8 but not 16 bytes aligned (the kernels' one-word accesses)"""
    from starks_amd import _lib
    m, w, k = _args(p) if op not in ("multi_inv", "multi_interp_4") else (p, 1, 0)
    a, b = f.get("a", f.get("xs", f.get("in", []))), f.get("b", f.get("ys", []))
    na, nb = len(a), len(b)
    pad = (na + nb) % 2  # keeps the parity of the outputs' offsets equal to shift's
    d = Dev(L, ctx, shift + pad + na + nb + 2 * (na + nb) + 12)
    try:
        ia, ib = shift, shift + na
        o1 = shift + pad + na + nb
        o2 = o1 + na + nb + 4
        d.put(ia, a)
        d.put(ib, b)
        d.put(o1, [FULL] * (2 * (na + nb) + 8))
        if op == "mul":
            rc, n1, n2 = L.sh_dev_mod64_poly_mul(ctx, m, w, k, d.at(ia), na, d.at(ib), nb, d.at(o1)), (na + nb - 1 if na and nb else 0), 0
        elif op == "divmod":
            rc = L.sh_dev_mod64_poly_divmod(ctx, m, w, k, d.at(ia), na, d.at(ib), nb, d.at(o1), d.at(o2))
            n1, n2 = max(na - nb + 1, 0), min(na, nb - 1)
        elif op == "zpoly":
            rc, n1, n2 = L.sh_dev_mod64_zpoly(ctx, m, w, k, d.at(ia), na, d.at(o1)), na + 1, 0
        elif op == "lagrange":
            rc, n1, n2 = L.sh_dev_mod64_lagrange_interp(ctx, m, w, k, d.at(ia), d.at(ib), na, d.at(o1)), na, 0
        elif op == "multi_inv":
            rc, n1, n2 = L.sh_dev_mod64_multi_inv(ctx, m, d.at(ia), d.at(o1), na), na, 0
        else:
            rc, n1, n2 = L.sh_dev_mod64_multi_interp_4(ctx, m, d.at(ia), d.at(ib), na // 4, d.at(o1)), na, 0
        _lib.check(rc, "sh_dev_mod64_* " + op)
        _lib.check(L.sh_sync(ctx), "sh_sync")
        assert d.get(o1 + n1, 1) == [FULL]  # nothing beyond the output
        return [d.get(o1, n1), d.get(o2, n2)] if op == "divmod" else [d.get(o1, n1)]
    finally:
        d.free()


@pytest.mark.parametrize("p", mc.FIXTURE_MODULI, ids=IDS.get)
def test_fixture_device_forms(L, G, p):
    """the fixture through the sh_dev_* forms: plain words in, canonical words out, on 16-byte and on 8-byte aligned addresses"""
    from starks_amd import _lib
    for i, c in enumerate(c for c in G if c["p"] == p):
        got = _dev_case(L, _lib.ctx(), p, c["op"], shift=i % 2, **mc.fixture_words(p, c))
        for rec, g in zip(mc.recorded(c), mc.normal(c, got)):
            assert mc.matches(rec, g), (c["op"], c["name"])


# ---- equality with the generic 32-byte entries, and exact ints at these sizes ---------------------------------------------------------
SIZES = [1, 2, 3, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025]  # 257 crosses one pass to two at the default tile


def _operand(rnd, p, n):
    """n words: random 64-bit values, a zero, p itself and 2^64 - 1 among them"""
    v = unwords(_rand_words(rnd, n))
    for i, x in ((n // 2, 0), (n // 3, p), (n // 5, FULL)):
        if n > 5:
            v[i] = x
    return v


@pytest.mark.parametrize("p", FIELDS3, ids=IDS.get)
@pytest.mark.parametrize("n", SIZES)
def test_products_and_zpoly_equal_generic_and_ints(L, p, n):
    from starks_amd.polynomial import mod64_mul_words, mod_mul_wire
    from starks_amd.poly_utils import mod64_zpoly_words, mod_zpoly_wire
    rnd = random.Random(n + p % 1000)
    xs, a, b = _operand(rnd, p, n), _operand(rnd, p, n), _operand(rnd, p, n // 3 + 1)
    z = mod64_zpoly_words(p, xs)
    assert bytes(z) == _from_wire(mod_zpoly_wire(p, _to_wire(words(p, xs)))) and list(z) == mc.zpoly(p, xs)
    c = mod64_mul_words(p, a, b)
    assert bytes(c) == _from_wire(mod_mul_wire(p, _to_wire(words(p, a)), _to_wire(words(p, b)))) and list(c) == mc.mul(p, a, b)
    from starks_amd import _lib
    assert _dev_case(L, _lib.ctx(), p, "mul", shift=n % 2, a=a, b=b) == [list(c)]
    assert _dev_case(L, _lib.ctx(), p, "zpoly", shift=1 - n % 2, xs=xs) == [list(z)]


@pytest.mark.parametrize("p", FIELDS3, ids=IDS.get)
def test_divmod_equals_generic_and_ints(L, p):
    from starks_amd import _lib
    from starks_amd.polynomial import mod64_divmod_words, mod_divmod_wire
    for na, nb in mc.DIVMOD_SIZES:
        rnd = random.Random(na * 11 + nb)
        a, b = _operand(rnd, p, na), _operand(rnd, p, nb)
        b[-1] = b[-1] % p or 1
        q, r = mod64_divmod_words(p, a, b)
        gq, gr = mod_divmod_wire(p, _to_wire(words(p, a)), _to_wire(words(p, b)))
        assert (bytes(q), bytes(r)) == (_from_wire(gq), _from_wire(gr)), (na, nb)
        assert (list(q), list(r)) == mc.divmod_(p, a, b), (na, nb)
        assert _dev_case(L, _lib.ctx(), p, "divmod", shift=(na + nb) % 2, a=a, b=b) == [list(q), list(r)], (na, nb)


@pytest.mark.parametrize("p", FIELDS3, ids=IDS.get)
@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 257, 700])
def test_lagrange_equals_generic_and_ints(L, p, n):
    from starks_amd import _lib
    from starks_amd.poly_utils import mod64_lagrange_interp_words, mod_lagrange_interp_wire
    rnd = random.Random(7 * n)
    xs, ys = unwords(_rand_words(rnd, n)), _operand(rnd, p, n)
    if n > 4:
        xs[2] = xs[1]  # a repeated x
        xs[-1] = p     # the point 0, stored as p
    out = mod64_lagrange_interp_words(p, xs, ys)
    assert bytes(out) == _from_wire(mod_lagrange_interp_wire(p, _to_wire(words(p, xs)), _to_wire(words(p, ys))))
    assert list(out) == mc.lagrange(p, xs, ys)
    assert _dev_case(L, _lib.ctx(), p, "lagrange", shift=n % 2, xs=xs, ys=ys) == [list(out)]


@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.BABYBEAR], ids=IDS.get)
def test_product_three_pass_transform(L, p):
    """2^16 + 1 by 2^16 coefficients: a 2^17-point transform, three passes at the default tile; the generic entry's words, and
    a b = a(r) b(r) at a random point"""
    from starks_amd.polynomial import mod64_mul_words, mod_mul_wire
    rnd = random.Random(17)
    na, nb = (1 << 16) + 1, 1 << 16
    assert mc.max_transform(mc.OP_MUL, na, nb) == 1 << 17
    a, b = _rand_words(rnd, na), _rand_words(rnd, nb)
    c = mod64_mul_words(p, a, b)
    assert len(c) == na + nb - 1 and bytes(c) == _from_wire(mod_mul_wire(p, _to_wire(a), _to_wire(b)))
    r = rnd.randrange(p)
    assert _horner(p, bytes(c), r) == _horner(p, a, r) * _horner(p, b, r) % p


# ---- the batch inversion at its level boundaries -------------------------------------------------------------------------------------
def _sampled(n, T, rnd):
    """at most 4096 positions of [0, n): the first and last item of every tile edge, the ends, and random ones"""
    edges = sorted({i for k in range(0, n // T + 2) for i in (k * T - 1, k * T) if 0 <= i < n} | {0, n - 1})
    if len(edges) > 4096:
        edges = sorted(set(edges[::len(edges) // 2048 + 1][:2046]) | set(edges[:16]) | set(edges[-16:]) | {0, n - 1})
    more = 4096 - len(edges)
    return sorted(set(edges) | set(rnd.sample(range(n), min(n, more))))[:4096] if more > 0 else edges


@pytest.mark.parametrize("n", [1, IV_T - 1, IV_T, IV_T + 1, IV_T * IV_T - 1, IV_T * IV_T, IV_T * IV_T + 1])
def test_multi_inv_level_boundaries(L, n):
    """one below, at and one above each level boundary of the 2048-value tile, up to three levels: the generic entry's words on the
    same values, exact ints at the tile edges, 0 exactly where a zero or a multiple of p was planted at a tile edge"""
    import numpy as np
    from starks_amd.poly_utils import mod64_multi_inv_words, mod_multi_inv_wire
    p = mc.P63 if n % 2 else mc.BABYBEAR
    rnd = random.Random(n)
    raw = np.frombuffer(_rand_words(rnd, n), dtype=np.uint64).copy()
    zeros = sorted({0, n // 2, n - 1, min(IV_T, n - 1), min(IV_T - 1, n - 1), (n - 1) // IV_T * IV_T})
    plant = [0, p, p * (FULL // p)]
    for j, i in enumerate(zeros):
        raw[i] = plant[j % 3]
    out = mod64_multi_inv_words(p, raw.tobytes())
    assert len(out) == n and bytes(out) == _from_wire(mod_multi_inv_wire(p, _to_wire(raw.tobytes())))
    o = np.frombuffer(out, dtype=np.uint64)
    nz = np.flatnonzero(raw % np.uint64(p) == 0).tolist()
    assert set(zeros) <= set(nz) and np.flatnonzero(o == 0).tolist() == nz and int(o.max()) < p
    for i in _sampled(n, IV_T, rnd):
        v = int(raw[i]) % p
        assert int(o[i]) == (pow(v, p - 2, p) if v else 0), i
    if n <= IV_T + 1:  # the device form, in place
        from starks_amd import _lib
        d = Dev(L, _lib.ctx(), n + 1)
        try:
            d.put(1, raw.tobytes())
            assert L.sh_dev_mod64_multi_inv(_lib.ctx(), p, d.at(1), d.at(1), n) == 0
            assert d.get(1, n) == list(out)
        finally:
            d.free()


@pytest.mark.parametrize("rows", [1, ROW_T - 1, ROW_T, ROW_T + 1, ROW_T * ROW_T - 1, ROW_T * ROW_T, ROW_T * ROW_T + 1])
def test_multi_interp_4_level_boundaries(L, rows):
    """the row tile's boundaries, up to three levels: the generic entry's words, and the exact cubic of the rows at the tile edges,
    degenerate rows among them"""
    from starks_amd.poly_utils import mod64_multi_interp_4_words, mod_multi_interp_4_wire
    p = mc.GOLDILOCKS if rows % 2 else mc.P63
    rnd = random.Random(rows)
    xs, ys = bytearray(_rand_words(rnd, 4 * rows)), _rand_words(rnd, 4 * rows)
    special = sorted({0, rows - 1, min(ROW_T, rows - 1), rows // 2})
    for r in special[1:]:
        xs[32 * r + 8:32 * r + 16] = xs[32 * r:32 * r + 8]  # a repeated x
    out = mod64_multi_interp_4_words(p, bytes(xs), ys)
    assert len(out) == 4 * rows
    assert bytes(out) == _from_wire(mod_multi_interp_4_wire(p, _to_wire(bytes(xs)), _to_wire(ys), rows))
    picked = set(special) | set(_sampled(rows, ROW_T, rnd)[::4])
    got = bytes(out)
    for r in sorted(picked):
        x4, y4, c4 = (unwords(bytes(b[32 * r:32 * r + 32])) for b in (xs, ys, got))
        assert c4 == mc.lagrange(p, x4, y4), r


@pytest.mark.parametrize("p", [mc.BIG, 3], ids=IDS.get)
def test_fields_of_little_two_adicity(L, p):
    """2^64 - 59 (2-adicity 2) and 3 (2-adicity 1): the inversions, which run no transform, at a size of two levels, and every
    product, division, zpoly and interpolation the field admits"""
    from starks_amd.polynomial import mod64_divmod_words, mod64_mul_words
    from starks_amd.poly_utils import (mod64_lagrange_interp_words, mod64_multi_interp_4_words, mod64_multi_inv_words,
                                       mod64_zpoly_words)
    rnd = random.Random(p % 1000)
    v = unwords(_rand_words(rnd, IV_T + 5))
    v[0], v[1], v[IV_T] = 0, p, p * (FULL // p)
    assert list(mod64_multi_inv_words(p, v)) == mc.multi_inv(p, v)
    xs, ys = unwords(_rand_words(rnd, 4 * (ROW_T + 3))), unwords(_rand_words(rnd, 4 * (ROW_T + 3)))
    xs[5] = xs[4]
    got = list(mod64_multi_interp_4_words(p, xs, ys))
    for r in (0, 1, 2, ROW_T - 1, ROW_T, ROW_T + 2):
        assert got[4 * r:4 * r + 4] == mc.lagrange(p, xs[4 * r:4 * r + 4], ys[4 * r:4 * r + 4]), r
    ran = 0
    for na, nb in mc.MUL_SIZES:
        if mc.admits(p, mc.OP_MUL, na, nb):
            a, b = unwords(_rand_words(rnd, na)), unwords(_rand_words(rnd, nb))
            assert list(mod64_mul_words(p, a, b)) == mc.mul(p, a, b)
            ran += 1
    for na, nb in mc.DIVMOD_SIZES:
        if mc.admits(p, mc.OP_DIVMOD, na, nb):
            a, b = unwords(_rand_words(rnd, na)), unwords(_rand_words(rnd, nb))
            b[-1] = b[-1] % p or 1
            assert tuple(list(x) for x in mod64_divmod_words(p, a, b)) == mc.divmod_(p, a, b)
            ran += 1
    for n in (1, 2, 3):
        xs = unwords(_rand_words(rnd, n))
        if mc.admits(p, mc.OP_ZPOLY, n):
            assert list(mod64_zpoly_words(p, xs)) == mc.zpoly(p, xs)
            ran += 1
        if mc.admits(p, mc.OP_LAGRANGE, n):
            assert list(mod64_lagrange_interp_words(p, xs, xs[::-1])) == mc.lagrange(p, xs, xs[::-1])
            ran += 1
    assert ran == (4 + 5 + 3 + 2 if p == mc.BIG else 2 + 2 + 2 + 0)
    # one coefficient too many for the field: refused with the sizes named
    from starks_amd import _lib
    m, w, k = _args(p)
    out = ctypes.create_string_buffer(8 * 16)
    n = (1 << k) + 1
    assert L.sh_mod64_zpoly(_lib.ctx(), m, w, k, words(p, list(range(n))), n, out) == ROOT_ORDER
    assert _err(L).startswith("sh_mod64_zpoly: ") and str(2 << k) in _err(L) and str(1 << k) in _err(L)


# ---- refusals and the empty cases ----------------------------------------------------------------------------------------------------
def test_refusals_and_empty_cases(L):
    from starks_amd import _lib
    c = _lib.ctx()
    p = 97
    m, w, k = _args(p)
    assert k == 5
    one, a = words(p, [1]), words(p, list(range(1, 21)))
    poison = bytes([0xee]) * 512
    buf = ctypes.create_string_buffer(poison, len(poison))
    names = []

    def refused(name, rc, code=INVALID, word=""):
        assert rc == code, (name, rc, _err(L))
        assert _err(L).startswith(name + ": ") and word in _err(L), (name, _err(L))
        names.append(name)

    # the modulus: even, 0, 1
    refused("sh_mod64_multi_inv", L.sh_mod64_multi_inv(c, 96, one, 1, buf), word="odd")
    refused("sh_mod64_multi_inv", L.sh_mod64_multi_inv(c, 0, one, 1, buf), word="odd")
    refused("sh_mod64_multi_interp_4", L.sh_mod64_multi_interp_4(c, 1, one * 4, one * 4, 1, buf), word="odd")
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, 96, w, k, one, 1, one, 1, buf), word="odd")
    refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, 1, w, k, one, 1, one, 1, buf, buf), word="odd")
    refused("sh_mod64_zpoly", L.sh_mod64_zpoly(c, 0, w, k, one, 1, buf), word="odd")
    refused("sh_mod64_lagrange_interp", L.sh_mod64_lagrange_interp(c, 2**64 - 2, w, k, one, one, 1, buf), word="odd")
    # the root: at or above p, of the wrong order, too small for the call, root_log 29
    refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, m, p, 0, a, 3, a, 2, buf, buf), ROOT_ORDER, "below")
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, m, p + w, k, a, 3, a, 3, buf), ROOT_ORDER, "below")
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, m, pow(w, 2, p), 5, a, 3, a, 3, buf), ROOT_ORDER, "order")  # order 16 as 32
    refused("sh_mod64_zpoly", L.sh_mod64_zpoly(c, m, w, 4, a, 3, buf), ROOT_ORDER, "order")                          # order 32 as 16
    refused("sh_mod64_lagrange_interp", L.sh_mod64_lagrange_interp(c, m, p - 1, 2, a, a, 2, buf), ROOT_ORDER, "order")  # -1 as order 4
    assert L.sh_mod_poly_max_transform(0, 20, 20) == 64
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, m, w, k, a, 20, a, 20, buf), ROOT_ORDER, "needs")
    assert "64" in _err(L) and "32" in _err(L)
    refused("sh_mod64_lagrange_interp", L.sh_mod64_lagrange_interp(c, m, w, k, a, a, 17, buf), ROOT_ORDER, "needs")
    refused("sh_mod64_zpoly", L.sh_mod64_zpoly(c, m, 1, 0, a, 1, buf), ROOT_ORDER, "needs")
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, m, w, 29, a, 3, a, 3, buf), UNSUPPORTED, "28")
    refused("sh_mod64_zpoly", L.sh_mod64_zpoly(c, m, w, 29, a, 3, buf), UNSUPPORTED, "28")
    # each size limit
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, m, w, k, one, (1 << 25) + 1, one, 1, buf), word="2^25")
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, m, w, k, one, 1 << 24, one, (1 << 24) + 2, buf), word="2^25")
    refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, m, w, k, one, (1 << 24) + 1, one, 1, buf, buf), word="2^24")
    refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, m, w, k, one, 1, one, (1 << 24) + 1, buf, buf), word="2^24")
    refused("sh_mod64_zpoly", L.sh_mod64_zpoly(c, m, w, k, one, (1 << 20) + 1, buf), word="2^20")
    refused("sh_mod64_lagrange_interp", L.sh_mod64_lagrange_interp(c, m, w, k, one, one, (1 << 20) + 1, buf), word="2^20")
    refused("sh_mod64_multi_inv", L.sh_mod64_multi_inv(c, m, one, (1 << 52) + 1, buf), word="too many")
    refused("sh_mod64_multi_interp_4", L.sh_mod64_multi_interp_4(c, m, one, one, (1 << 52) + 1, buf), word="too many")
    # null pointers
    refused("sh_mod64_multi_inv", L.sh_mod64_multi_inv(c, m, None, 1, buf), word="null")
    refused("sh_mod64_multi_interp_4", L.sh_mod64_multi_interp_4(c, m, one * 4, None, 1, buf), word="null")
    refused("sh_mod64_poly_mul", L.sh_mod64_poly_mul(c, m, w, k, None, 1, one, 1, buf), word="null")
    refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, m, w, k, a, 3, a, 2, None, buf), word="null")
    refused("sh_mod64_zpoly", L.sh_mod64_zpoly(c, m, w, k, one, 1, None), word="null")
    refused("sh_mod64_lagrange_interp", L.sh_mod64_lagrange_interp(c, m, w, k, one, None, 1, buf), word="null")
    # the divisor: empty, a leading word of 0, of p itself, of another multiple of p
    refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, m, w, k, one, 1, one, 0, buf, buf), word="empty")
    for lead in (0, p, 5 * p, p * (FULL // p)):
        refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, m, w, k, a, 3, words(p, [1, lead]), 2, buf, buf), word="leading")
    G = mc.GOLDILOCKS
    refused("sh_mod64_poly_divmod", L.sh_mod64_poly_divmod(c, G, *_args(G)[1:], a, 3, words(G, [1, G]), 2, buf, buf), word="leading")
    assert buf.raw == poison  # nothing was written
    # the empty cases
    assert L.sh_mod64_poly_mul(c, m, w, k, one, 0, one, 1, buf) == 0
    assert L.sh_mod64_lagrange_interp(c, m, w, k, one, one, 0, buf) == 0
    assert L.sh_mod64_multi_inv(c, m, one, 0, buf) == 0 and L.sh_mod64_multi_interp_4(c, m, one, one, 0, buf) == 0
    assert L.sh_mod64_poly_divmod(c, m, w, k, one, 0, one, 1, buf, buf) == 0
    assert buf.raw == poison
    assert L.sh_mod64_zpoly(c, m, 1, 0, None, 0, buf) == 0 and unwords(buf.raw[:8]) == [1] and buf.raw[8:] == poison[8:]
    q, r = ctypes.create_string_buffer(poison[:64], 64), ctypes.create_string_buffer(poison[:64], 64)
    assert L.sh_mod64_poly_divmod(c, m, w, k, words(p, [5, 98, 3]), 3, a, 20, q, r) == 0  # shorter than the divisor: its own remainder
    assert q.raw == poison[:64] and unwords(r.raw[:24]) == [5, 1, 3] and r.raw[24:] == poison[24:64]
    # device forms: each overlap rule, and a divisor whose leading word is 0 mod p (the one read-back), before any launch
    d = Dev(L, c, 64)
    try:
        d.put(0, [0xee] * 64)
        d.put(8, [1, 2, 3, p])  # a divisor ending in the word p
        at = d.at
        refused("sh_dev_mod64_poly_mul", L.sh_dev_mod64_poly_mul(c, m, w, k, at(0), 8, at(8), 8, at(4)), word="overlap")
        refused("sh_dev_mod64_poly_mul", L.sh_dev_mod64_poly_mul(c, m, w, k, at(0), 8, at(8), 8, at(15)), word="overlap")
        refused("sh_dev_mod64_zpoly", L.sh_dev_mod64_zpoly(c, m, w, k, at(0), 8, at(7)), word="overlap")
        refused("sh_dev_mod64_lagrange_interp", L.sh_dev_mod64_lagrange_interp(c, m, w, k, at(0), at(8), 8, at(15)), word="overlap")
        refused("sh_dev_mod64_lagrange_interp", L.sh_dev_mod64_lagrange_interp(c, m, w, k, at(0), at(8), 8, at(0)), word="overlap")
        refused("sh_dev_mod64_poly_divmod", L.sh_dev_mod64_poly_divmod(c, m, w, k, at(0), 8, at(8), 4, at(9), at(40)), word="overlap")
        refused("sh_dev_mod64_poly_divmod", L.sh_dev_mod64_poly_divmod(c, m, w, k, at(0), 8, at(8), 4, at(20), at(7)), word="overlap")
        refused("sh_dev_mod64_poly_divmod", L.sh_dev_mod64_poly_divmod(c, m, w, k, at(0), 8, at(8), 4, at(20), at(20)), word="overlap")
        refused("sh_dev_mod64_poly_divmod", L.sh_dev_mod64_poly_divmod(c, m, w, k, at(0), 8, at(8), 4, at(20), at(40)), word="leading")
        refused("sh_dev_mod64_multi_inv", L.sh_dev_mod64_multi_inv(c, m, at(0), at(4), 8), word="overlap")
        refused("sh_dev_mod64_multi_interp_4", L.sh_dev_mod64_multi_interp_4(c, m, at(0), at(16), 2, at(4)), word="overlap")
        refused("sh_dev_mod64_multi_interp_4", L.sh_dev_mod64_multi_interp_4(c, m, at(0), at(16), 2, at(20)), word="overlap")
        refused("sh_dev_mod64_multi_inv", L.sh_dev_mod64_multi_inv(c, 96, at(0), at(16), 8), word="odd")
        refused("sh_dev_mod64_multi_inv", L.sh_dev_mod64_multi_inv(c, m, None, at(16), 8), word="null")
        refused("sh_dev_mod64_zpoly", L.sh_dev_mod64_zpoly(c, m, w, 4, at(0), 8, at(20)), ROOT_ORDER, "order")
        refused("sh_dev_mod64_zpoly", L.sh_dev_mod64_zpoly(c, m, w, 29, at(0), 8, at(20)), UNSUPPORTED, "28")
        refused("sh_dev_mod64_poly_mul", L.sh_dev_mod64_poly_mul(c, m, w, k, at(0), 20, at(20), 20, at(40)), ROOT_ORDER, "needs")
        _lib.check(L.sh_sync(c), "sh_sync")
        assert d.get(0, 8) + d.get(12, 52) == [0xee] * 60  # nothing was written
        # in-place forms that ARE allowed
        d.put(0, [3, 5, 0, p + 7])
        assert L.sh_dev_mod64_multi_inv(c, m, at(0), at(0), 4) == 0
        assert d.get(0, 4) == mc.multi_inv(p, [3, 5, 0, 7])
        d.put(0, [1, 2, 3, 4, 9, 9, 9, 9])
        d.put(16, [5, 6, 0, 1] * 2)
        assert L.sh_dev_mod64_multi_interp_4(c, m, at(0), at(16), 2, at(16)) == 0
        assert d.get(16, 8) == mc.multi_interp_4(p, [1, 2, 3, 4, 9, 9, 9, 9], [5, 6, 0, 1] * 2)
    finally:
        d.free()
    assert len(set(names)) == 12


# ---- contexts ------------------------------------------------------------------------------------------------------------------------
def _stats(L, c):
    out = (ctypes.c_uint64 * 4)()
    assert L.sh_ctx_stats(c, out) == 0
    return list(out)


def test_two_contexts_interleaved_and_plan_statistics(L):
    """two contexts with different moduli, 32-byte generic calls and MiMC polynomial calls in between on one of them: the words of
    separate runs; the packed plans are counted by the plan cache's statistics, built once and then hit"""
    from starks_amd import _lib
    from starks_amd.polynomial import mod64_mul_words, mod_mul_wire, mul_wire
    from starks_amd.poly_utils import mod64_lagrange_interp_words, mod64_zpoly_words, mod_zpoly_wire, zpoly_wire
    c1 = _lib.ctx()
    c2 = ctypes.c_void_p()
    assert L.sh_ctx_create(_lib.default_device(), ctypes.byref(c2)) == 0
    try:
        rnd = random.Random(31)
        n = 1500
        pa, pb = mc.GOLDILOCKS, mc.BABYBEAR
        xa, ya, xb, yb = (_rand_words(rnd, n) for _ in range(4))
        wx = _to_wire(xa)
        want = [bytes(mod64_lagrange_interp_words(pa, xa, ya)), bytes(mod64_lagrange_interp_words(pb, xb, yb)),
                bytes(mod64_mul_words(pb, xb, yb)), bytes(mod64_zpoly_words(pa, xa)), mod_zpoly_wire(pa, wx), zpoly_wire(wx)]
        (ma, wa, ka), (mb, wb, kb) = _args(pa), _args(pb)
        m32, w32, k32 = _lib.mod_poly_args(pa)
        out = [ctypes.create_string_buffer(32 * (2 * n)) for _ in range(6)]
        assert _stats(L, c2) == [0, 0, 0, 0]
        built = []
        for _ in range(2):
            _lib.check(L.sh_mod64_lagrange_interp(c1, ma, wa, ka, xa, ya, n, out[0]), "goldilocks on ctx 1")
            _lib.check(L.sh_mod64_lagrange_interp(c2, mb, wb, kb, xb, yb, n, out[1]), "babybear on ctx 2")
            _lib.check(L.sh_mod_zpoly(c1, m32, w32, k32, wx, n, out[4]), "32-byte goldilocks on ctx 1")
            _lib.check(L.sh_mod64_poly_mul(c1, mb, wb, kb, xb, n, yb, n, out[2]), "babybear on ctx 1")
            _lib.check(L.sh_zpoly(c1, wx, n, out[5]), "mimc on ctx 1")
            _lib.check(L.sh_mod64_zpoly(c2, ma, wa, ka, xa, n, out[3]), "goldilocks on ctx 2")
            assert mul_wire(wx[:3200], wx[:3200]) == mul_wire(wx[:3200], wx[:3200])
            got = [out[0].raw[:8 * n], out[1].raw[:8 * n], out[2].raw[:8 * (2 * n - 1)], out[3].raw[:8 * (n + 1)], out[4].raw[:32 * (n + 1)],
                   out[5].raw[:32 * (n + 1)]]
            assert got == want
            built.append(_stats(L, c2))
        # ctx 2 ran only packed calls: lagrange_interp over BabyBear uses the sizes 2 .. 4096 in both directions, zpoly over Goldilocks
        # 2 .. 2048: every one is a plan, counted once; the 2-point transform's root -1 is its own inverse, so one plan serves both
        # of its directions in each field
        assert built[0][0] == built[0][2] == (2 * 12 - 1) + (2 * 11 - 1) and built[0][1] > 0 and built[0][3] == 0
        assert built[1] == built[0]  # the second round built nothing
        assert mod_mul_wire(pb, _to_wire(xb), _to_wire(yb)) == _to_wire(want[2])
    finally:
        L.sh_ctx_destroy(c2)


# ---- the Python forms ----------------------------------------------------------------------------------------------------------------
def test_python_forms_and_routing(L, monkeypatch):
    """the six word forms on lists and on bytes give the same words, memoryviews of format 'Q'; Polynomial.__mul__ over Goldilocks
    still takes the 32-byte path"""
    from starks_amd import IntegersModP, poly_utils, polynomial
    from starks_amd.polynomial import polynomials_over
    p = mc.GOLDILOCKS
    rnd = random.Random(5)
    a, b = unwords(_rand_words(rnd, 70)), unwords(_rand_words(rnd, 33))
    b[-1] = b[-1] % p or 1
    xs, ys = a[:40], b + a[:7]
    pairs = [
        (polynomial.mod64_mul_words(p, a, b), polynomial.mod64_mul_words(p, words(p, a), words(p, b)), mc.mul(p, a, b)),
        (poly_utils.mod64_zpoly_words(p, xs), poly_utils.mod64_zpoly_words(p, bytearray(words(p, xs))), mc.zpoly(p, xs)),
        (poly_utils.mod64_lagrange_interp_words(p, xs, ys), poly_utils.mod64_lagrange_interp_words(p, words(p, xs), words(p, ys)),
         mc.lagrange(p, xs, ys)),
        (poly_utils.mod64_multi_inv_words(p, a), poly_utils.mod64_multi_inv_words(p, words(p, a)), mc.multi_inv(p, a)),
        (poly_utils.mod64_multi_interp_4_words(p, xs, ys), poly_utils.mod64_multi_interp_4_words(p, words(p, xs), words(p, ys)),
         mc.multi_interp_4(p, xs, ys)),
    ]
    for from_list, from_bytes, want in pairs:
        assert from_list.format == from_bytes.format == "Q" and list(from_list) == list(from_bytes) == want
    q1, r1 = polynomial.mod64_divmod_words(p, a, b)
    q2, r2 = polynomial.mod64_divmod_words(p, words(p, a), words(p, b))
    assert (list(q1), list(r1)) == (list(q2), list(r2)) == mc.divmod_(p, a, b) and q1.format == r1.format == "Q"
    assert [len(x) for x in polynomial.mod64_divmod_words(p, a[:5], b)] == [0, 5]
    w, k = mc.two_adic_root(p)
    assert list(polynomial.mod64_mul_words(p, a, b, root=(pow(w, 3, p), k))) == mc.mul(p, a, b)
    # routing does not change
    calls = []
    real = polynomial.mod_mul_wire
    monkeypatch.setattr(polynomial, "mod_mul_wire", lambda *x, **y: calls.append("mod_mul_wire") or real(*x, **y))
    monkeypatch.setattr(polynomial, "mod64_mul_words", lambda *x, **y: pytest.fail("Polynomial.__mul__ must keep the 32-byte path"))
    Poly = polynomials_over(IntegersModP(p))
    prod = Poly([v % p for v in a]) * Poly([v % p for v in b])
    assert calls == ["mod_mul_wire"] and [int(v) for v in prod] == mc.strip(mc.mul(p, a, b))


if __name__ == "__main__" and sys.argv[1:] == ["tile-child"]:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    cases = [c for c in mc.resolved(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mod_poly.json"))))
             if c["p"] in mc.FIXTURE_MODULI]
    print(_digest(cases))
