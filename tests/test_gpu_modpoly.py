"""Polynomial products, division, zpoly, lagrange_interp, multi_inv and multi_interp_4 over any prime modulus below 2^256 on the
MI355X (the sh_mod_* / sh_dev_mod_* entries of include/starkhip.h; csrc/modpoly.hip, api_modpoly.hip; starks_amd.polynomial and
poly_utils' mod_*_wire forms): byte-identical to tests/golden/mod_poly.json (the live reference over IntegersModP(p)); over the MiMC
prime byte-identical to the MiMC entries; exact against Python ints around the tile and pass boundaries of the generic transform;
O(n) identities at random points above that; the batch inversion at its level boundaries; every refusal with its code and the
entry's name; two contexts and MiMC calls interleaved.  All comparisons are exact."""
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
import modpoly_cases as mp  # noqa: E402
from modpoly_cases import ints, matches, strip, wire  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, ROOT_ORDER, UNSUPPORTED = -1, -2, -6
FIELDS3 = [mp.BN254, mp.GOLDILOCKS, 65537]
IDS = {mp.BN254: "bn254", mp.BLS12_381: "bls12_381", mp.GOLDILOCKS: "goldilocks", 65537: "f65537", 97: "f97", 12289: "f12289"}
IV_T, ROW_T = 512, 256  # the tiles the implementation chose (modpoly_items.cuh: MP_IV_LANES x MP_IV_CHUNK, x MP_IV_ROW_CHUNK)


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


@pytest.fixture(scope="module")
def G():
    return mp.resolved(load_golden("mod_poly.json"))


def _mb(p):
    return int(p).to_bytes(32, "big")


def _args(p, root=None):
    from starks_amd import _lib
    return _lib.mod_poly_args(p, root)


def _rand_wire(rnd, p, n):
    """n random 256-bit values as wire bytes, fast (any 256-bit value is an input: the entries take it mod p)"""
    import numpy as np
    raw = np.random.default_rng(rnd.getrandbits(64)).integers(0, 256, size=(n, 32), dtype=np.uint8)
    return raw.tobytes()


def _horner_wire(p, raw, x):
    y = 0
    mv = memoryview(raw)
    for i in range(len(raw) - 32, -32, -32):
        y = (y * x + int.from_bytes(mv[i:i + 32], "big")) % p
    return y


def _err(L):
    from starks_amd import _lib
    return L.sh_last_error(_lib.ctx()).decode()


# ---- host-buffer forms through ctypes (what the Python explicit forms wrap) ----------------------------------------------------------
def _fixture_outputs(c):
    """every output of a fixture case through the Python explicit forms, as lists of ints"""
    from starks_amd.polynomial import mod_divmod_wire, mod_mul_wire
    from starks_amd.poly_utils import mod_lagrange_interp_wire, mod_multi_interp_4_wire, mod_multi_inv_wire, mod_zpoly_wire
    p, op = c["p"], c["op"]
    if op == "mul":
        return [strip(ints(mod_mul_wire(p, wire(p, c["a"]), wire(p, c["b"]))))]
    if op == "divmod":
        q, r = mod_divmod_wire(p, wire(p, c["a"]), wire(p, c["b"]))
        return [strip(ints(q)), strip(ints(r))]
    if op == "zpoly":
        return [ints(mod_zpoly_wire(p, wire(p, c["xs"])))]
    if op == "lagrange":
        return [strip(ints(mod_lagrange_interp_wire(p, wire(p, c["xs"]), wire(p, c["ys"]))))]
    if op == "multi_inv":
        v = list(c["in"])
        for i in c["zeros"]:
            v[i] = 0
        return [ints(mod_multi_inv_wire(p, wire(p, v)))]
    return [ints(mod_multi_interp_4_wire(p, wire(p, c["xs"]), wire(p, c["ys"]), len(c["xs"]) // 4))]


def _recorded(c):
    return [c["q"], c["r"]] if c["op"] == "divmod" else [c["out"]]


@pytest.mark.parametrize("p", mp.FIXTURE_MODULI, ids=IDS.get)
def test_fixture_bytes(L, G, p):
    """the live reference's outputs over IntegersModP(p) through the host-buffer forms (the Python explicit forms)"""
    for c in (c for c in G if c["p"] == p):
        for rec, got in zip(_recorded(c), _fixture_outputs(c)):
            assert matches(rec, got), (c["op"], c["name"])


def _digest(cases):
    h = hashlib.sha256()
    for c in cases:
        for got in _fixture_outputs(c):
            h.update(wire(c["p"], got) + b"|")
    return h.hexdigest()


def test_fixture_with_four_element_tiles(L, G):
    """STARKHIP_MODNTT_TILE_LOG=4 in a child process: every transform above 16 points runs several passes, so every tree level does;
    the child's outputs over BN254 and 65537 equal this process's"""
    cases = [c for c in G if c["p"] in (mp.BN254, 65537)]
    env = dict(os.environ, STARKHIP_MODNTT_TILE_LOG="4")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "tile-child"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == _digest(cases)
    for c in cases[::7]:
        for rec, got in zip(_recorded(c), _fixture_outputs(c)):
            assert matches(rec, got)


# ---- device forms --------------------------------------------------------------------------------------------------------------------
class Dev(object):
    """device buffers of plain limbs: upload ints as 8 x u32 little-endian limbs, unreduced, download the same way"""

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


def _dev_case(L, ctx, p, op, **f):
    """one call of a device form on ints (any 256-bit values), the outputs as ints; the output area is poisoned first"""
    from starks_amd import _lib
    m, w, k = _args(p)
    a, b = f.get("a", f.get("xs", f.get("in", []))), f.get("b", f.get("ys", []))
    na, nb = len(a), len(b)
    d = Dev(L, ctx, na + nb + 2 * (na + nb) + 8)
    try:
        o1, o2 = na + nb, na + nb + na + nb + 4
        d.put(0, a)
        d.put(na, b)
        d.put(o1, [2**256 - 1] * (2 * (na + nb) + 8))
        if op == "mul":
            rc, n1, n2 = L.sh_dev_mod_poly_mul(ctx, m, w, k, d.at(0), na, d.at(na), nb, d.at(o1)), (na + nb - 1 if na and nb else 0), 0
        elif op == "divmod":
            rc = L.sh_dev_mod_poly_divmod(ctx, m, w, k, d.at(0), na, d.at(na), nb, d.at(o1), d.at(o2))
            n1, n2 = max(na - nb + 1, 0), min(na, nb - 1)
        elif op == "zpoly":
            rc, n1, n2 = L.sh_dev_mod_zpoly(ctx, m, w, k, d.at(0), na, d.at(o1)), na + 1, 0
        elif op == "lagrange":
            rc, n1, n2 = L.sh_dev_mod_lagrange_interp(ctx, m, w, k, d.at(0), d.at(na), na, d.at(o1)), na, 0
        elif op == "multi_inv":
            rc, n1, n2 = L.sh_dev_mod_multi_inv(ctx, m, d.at(0), d.at(o1), na), na, 0
        else:
            rc, n1, n2 = L.sh_dev_mod_multi_interp_4(ctx, m, d.at(0), d.at(na), na // 4, d.at(o1)), na, 0
        _lib.check(rc, "sh_dev_mod_* " + op)
        _lib.check(L.sh_sync(ctx), "sh_sync")
        assert d.get(o1 + n1, 1) == [2**256 - 1]  # nothing beyond the output
        return [d.get(o1, n1), d.get(o2, n2)] if op == "divmod" else [d.get(o1, n1)]
    finally:
        d.free()


@pytest.mark.parametrize("p", [mp.BN254, 97], ids=IDS.get)
def test_fixture_device_forms(L, G, p):
    """the fixture through the sh_dev_* forms: plain limbs in (as stored: >= p included), canonical limbs out"""
    from starks_amd import _lib
    for c in (c for c in G if c["p"] == p):
        f = {k: [int(v) % 2**256 if int(v) >= 0 else int(v) % p for v in c[k]] for k in ("a", "b", "xs", "ys", "in") if k in c}
        if c["op"] == "multi_inv":
            for i in c["zeros"]:
                f["in"][i] = 0
        got = _dev_case(L, _lib.ctx(), p, c["op"], **f)
        for rec, g in zip(_recorded(c), got):
            assert matches(rec, g if c["op"] in ("zpoly", "multi_inv", "multi_interp_4") else strip(g)), (c["op"], c["name"])


# ---- the MiMC prime: the yardstick that needs no oracle ------------------------------------------------------------------------------
def test_equals_mimc_entries(L):
    """over the MiMC prime the generic entries give the MiMC entries' bytes on the same inputs, inputs stored as x + p included"""
    from starks_amd.polynomial import divmod_wire, mod_divmod_wire, mod_mul_wire, mul_wire
    from starks_amd.poly_utils import (lagrange_interp_wire, mod_lagrange_interp_wire, mod_multi_interp_4_wire, mod_multi_inv_wire,
                                       mod_zpoly_wire, multi_interp_4_wire, multi_inv_wire, zpoly_wire)
    p, rnd = mp.MIMC_P, random.Random(77)
    n = 3000

    def vals(k):
        v = [rnd.randrange(p) for _ in range(k)]
        for i in range(0, k, 5):
            if v[i] < 2**256 - p:
                v[i] += p  # stored as x + p
        v[1 % k] = rnd.randrange(2**256 - p) + p
        return v

    a, b, xs, ys = wire(p, vals(n)), wire(p, vals(n // 3)), wire(p, vals(1500)), wire(p, vals(1500))
    assert mod_mul_wire(p, a, b) == mul_wire(a, b)
    assert mod_divmod_wire(p, a, b) == divmod_wire(a, b)
    assert mod_divmod_wire(p, b, a) == divmod_wire(b, a)
    assert mod_zpoly_wire(p, xs) == zpoly_wire(xs)
    xr = xs[:32] + xs[:32] + xs[64:]  # a repeated x
    assert mod_lagrange_interp_wire(p, xr, ys) == lagrange_interp_wire(xr, ys)
    z = wire(p, [0, p, 5]) + a
    assert mod_multi_inv_wire(p, z) == multi_inv_wire(z)
    rows = 700
    x4 = bytearray(wire(p, vals(4 * rows)))
    x4[128 + 32:128 + 64] = x4[128:128 + 32]      # row 1: a pair
    x4[256 + 32:256 + 128] = x4[256:256 + 32] * 3  # row 2: all four equal
    y4 = wire(p, vals(4 * rows))
    assert mod_multi_interp_4_wire(p, bytes(x4), y4, rows) == multi_interp_4_wire(bytes(x4), y4, rows)


# ---- exact against Python ints around a tile (2^10 elements) and a pass boundary of the generic transform ----------------------------
SIZES = [1, 2, 3, 31, 32, 33, 1023, 1024, 1025, 2047, 2048, 2049]


@pytest.mark.parametrize("p", FIELDS3, ids=IDS.get)
@pytest.mark.parametrize("n", SIZES)
def test_exact_products_zpoly_divmod(L, p, n):
    from starks_amd.polynomial import mod_divmod_wire, mod_mul_wire
    from starks_amd.poly_utils import mod_zpoly_wire
    rnd = random.Random(n + p % 1000)
    xs = [rnd.randrange(p) for _ in range(n)]
    assert ints(mod_zpoly_wire(p, wire(p, xs))) == mp.zpoly(p, xs)
    a = [rnd.randrange(2**256) for _ in range(n)]  # any 256-bit value
    b = [rnd.randrange(p) for _ in range(n // 3 + 1)]
    b[-1] = b[-1] or 1
    assert ints(mod_mul_wire(p, wire(p, a), wire(p, b))) == mp.mul(p, a, b)
    q, r = mod_divmod_wire(p, wire(p, a), wire(p, b))
    assert (ints(q), ints(r)) == mp.divmod_(p, a, b)


@pytest.mark.parametrize("p", [mp.BN254, mp.GOLDILOCKS], ids=IDS.get)
def test_product_three_pass_transform(L, p):
    """just over 2^20 result coefficients: a 2^21-point transform, three passes; a b at two random points equals a(r) b(r)"""
    from starks_amd.polynomial import mod_mul_wire
    rnd = random.Random(21)
    na, nb = (1 << 19) + 7, (1 << 19) + 11
    a, b = _rand_wire(rnd, p, na), _rand_wire(rnd, p, nb)
    c = mod_mul_wire(p, a, b)
    assert len(c) == 32 * (na + nb - 1) and na + nb - 1 > 1 << 20
    for _ in range(2):
        r = rnd.randrange(p)
        assert _horner_wire(p, c, r) == _horner_wire(p, a, r) * _horner_wire(p, b, r) % p
    assert all(int.from_bytes(c[i:i + 32], "big") < p for i in range(0, 32 * 4096, 32))  # canonical


@pytest.mark.parametrize("p", [mp.BN254, mp.GOLDILOCKS], ids=IDS.get)
def test_divmod_identity(L, p):
    """2^16 + 5 by 2^15 - 3 coefficients: a = q b + r at random points, and the lengths"""
    from starks_amd.polynomial import mod_divmod_wire
    rnd = random.Random(16)
    na, nb = (1 << 16) + 5, (1 << 15) - 3
    a, b = _rand_wire(rnd, p, na), _rand_wire(rnd, p, nb)
    q, rem = mod_divmod_wire(p, a, b)
    assert len(q) == 32 * (na - nb + 1) and len(rem) == 32 * (nb - 1)
    for _ in range(2):
        x = rnd.randrange(p)
        assert _horner_wire(p, a, x) == (_horner_wire(p, q, x) * _horner_wire(p, b, x) + _horner_wire(p, rem, x)) % p


@pytest.mark.parametrize("p", FIELDS3, ids=IDS.get)
@pytest.mark.parametrize("n", [1, 2, 5, 64, 65, 257, 700])
def test_exact_lagrange(L, p, n):
    from starks_amd.poly_utils import mod_lagrange_interp_wire
    rnd = random.Random(7 * n)
    xs = [rnd.randrange(p) for _ in range(n)]
    ys = [rnd.randrange(2**256) for _ in range(n)]
    if n > 4:
        xs[2] = xs[1]
        xs[-1] = 0
    assert ints(mod_lagrange_interp_wire(p, wire(p, xs), wire(p, ys))) == mp.lagrange(p, xs, ys)


def test_lagrange_roots_of_unity_12289(L):
    """over the 2^12 powers of a root of unity of 12289's field the interpolant is the inverse transform of ys"""
    from starks_amd import fft
    from starks_amd.poly_utils import mod_lagrange_interp_wire
    p, n = 12289, 1 << 12
    w, k = mp.two_adic_root(p)
    assert k == 12
    rnd = random.Random(12)
    ys = wire(p, [rnd.randrange(p) for _ in range(n)])
    xs = wire(p, [pow(w, i, p) for i in range(n)])
    # needs a transform of 2^13 > 2^12: refused with the sizes in the text; the largest n this field admits is 2^11
    out = ctypes.create_string_buffer(32 * n)
    from starks_amd import _lib
    m, wb, kk = _args(p)
    assert L.sh_mod_lagrange_interp(_lib.ctx(), m, wb, kk, xs, ys, n, out) == ROOT_ORDER
    assert "8192" in _err(L) and "4096" in _err(L) and _err(L).startswith("sh_mod_lagrange_interp")
    h = n // 2
    w2 = pow(w, 2, p)
    xs2 = wire(p, [pow(w2, i, p) for i in range(h)])
    assert mod_lagrange_interp_wire(p, xs2, ys[:32 * h]) == fft.mod_ntt_bytes(p, ys[:32 * h], h, w2, inverse=True)


# ---- the batch inversion at its level boundaries -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, IV_T - 1, IV_T, IV_T + 1, IV_T * IV_T - 1, IV_T * IV_T, IV_T * IV_T + 1])
def test_multi_inv_level_boundaries(L, n):
    """one below, at and one above each level boundary of the 512-value tile, up to three levels: in * out == 1, zeros planted"""
    import numpy as np
    from starks_amd.poly_utils import mod_multi_inv_wire
    p = mp.BN254
    rnd = random.Random(n)
    raw = bytearray(_rand_wire(rnd, p, n))
    zeros = sorted({0, n // 2, n - 1, min(IV_T, n - 1)})
    for i in zeros:
        raw[32 * i:32 * i + 32] = bytes(32) if i % 2 == 0 else _mb(p)  # 0, or p itself
    out = mod_multi_inv_wire(p, bytes(raw))
    assert len(out) == 32 * n
    zset, vi, wi = set(zeros), ints(bytes(raw)), ints(out)
    assert all(w < p and v * w % p == (0 if i in zset else 1) for i, (v, w) in enumerate(zip(vi, wi)))  # every element
    o = np.frombuffer(out, dtype=np.uint8).reshape(-1, 32)
    assert np.flatnonzero(~o.any(axis=1)).tolist() == zeros  # 0 exactly where the value is 0 mod p
    if n <= IV_T + 1:
        assert wi == mp.multi_inv(p, vi)


@pytest.mark.parametrize("rows", [1, ROW_T - 1, ROW_T, ROW_T + 1, ROW_T * ROW_T - 1, ROW_T * ROW_T, ROW_T * ROW_T + 1])
def test_multi_interp_4_level_boundaries(L, rows):
    """the row tile's boundaries, up to three levels: the cubic through each sampled row's points, degenerate rows by the exact rule"""
    from starks_amd.poly_utils import mod_multi_interp_4_wire
    p = mp.GOLDILOCKS
    rnd = random.Random(rows)
    xs, ys = bytearray(_rand_wire(rnd, p, 4 * rows)), _rand_wire(rnd, p, 4 * rows)
    special = sorted({0, rows - 1, min(ROW_T, rows - 1), rows // 2})
    for r in special[1:]:
        xs[128 * r + 32:128 * r + 64] = xs[128 * r:128 * r + 32]  # a repeated x
    out = mod_multi_interp_4_wire(p, bytes(xs), ys, rows)
    assert len(out) == 128 * rows
    for r in sorted(set(special) | set(rnd.sample(range(rows), min(rows, 2000))) | {x for x in (ROW_T - 1, ROW_T * ROW_T - 1) if x < rows}):
        x4, y4, c4 = (ints(bytes(b[128 * r:128 * r + 128])) for b in (xs, ys, out))
        assert c4 == mp.lagrange(p, x4, y4), r


# ---- refusals and the empty cases ----------------------------------------------------------------------------------------------------
def test_root_order_refusals(L):
    from starks_amd import _lib
    c = _lib.ctx()
    p = 97
    m, w, k = _args(p)
    assert k == 5
    a = wire(p, list(range(1, 21)))
    poison = bytes([0xee]) * (32 * 64)
    out = ctypes.create_string_buffer(poison, len(poison))
    # 20 x 20 coefficients over 97: size 64 against a root of order 32
    assert L.sh_mod_poly_max_transform(0, 20, 20) == 64
    assert L.sh_mod_poly_mul(c, m, w, k, a, 20, a, 20, out) == ROOT_ORDER
    assert _err(L).startswith("sh_mod_poly_mul: ") and "64" in _err(L) and "32" in _err(L)
    # a root of the wrong order: order 16 given as 32, order 32 given as 16; -1 given as order 4
    w16 = (pow(int.from_bytes(w, "big"), 2, p)).to_bytes(32, "big")
    assert L.sh_mod_poly_mul(c, m, w16, 5, a, 3, a, 3, out) == ROOT_ORDER and "order" in _err(L)
    assert L.sh_mod_zpoly(c, m, w, 4, a, 3, out) == ROOT_ORDER and _err(L).startswith("sh_mod_zpoly: ") and "order" in _err(L)
    assert L.sh_mod_lagrange_interp(c, m, _mb(p - 1), 2, a, a, 2, out) == ROOT_ORDER and _err(L).startswith("sh_mod_lagrange_interp: ")
    # a root at or above p
    assert L.sh_mod_poly_divmod(c, m, _mb(p), 0, a, 3, a, 2, out, out) == ROOT_ORDER
    assert _err(L).startswith("sh_mod_poly_divmod: ") and "below" in _err(L)
    assert L.sh_mod_poly_mul(c, m, _mb(p + int.from_bytes(w, "big")), k, a, 3, a, 3, out) == ROOT_ORDER and "below" in _err(L)
    assert L.sh_mod_poly_mul(c, m, w, 27, a, 3, a, 3, out) == UNSUPPORTED
    assert out.raw == poison  # nothing was written
    # root_log = 0 takes the root 1 and admits no transform at all
    assert L.sh_mod_zpoly(c, m, _mb(1), 0, a, 0, out) == 0 and ints(out.raw[:32]) == [1]
    assert L.sh_mod_zpoly(c, m, _mb(1), 0, a, 1, out) == ROOT_ORDER


def test_other_refusals_and_empty_cases(L):
    from starks_amd import _lib
    c = _lib.ctx()
    p = mp.BN254
    m, w, k = _args(p)
    one = wire(p, [1])
    poison = bytes([0xee]) * 256
    buf = ctypes.create_string_buffer(poison, len(poison))
    names = []

    def refused(name, rc, code=INVALID, word=""):
        assert rc == code, (name, rc)
        assert _err(L).startswith(name + ": ") and word in _err(L), (name, _err(L))
        names.append(name)

    even, tiny = _mb(p - 1), _mb(1)
    refused("sh_mod_multi_inv", L.sh_mod_multi_inv(c, even, one, 1, buf), word="odd")
    refused("sh_mod_multi_inv", L.sh_mod_multi_inv(c, m, None, 1, buf), word="null")
    refused("sh_mod_multi_interp_4", L.sh_mod_multi_interp_4(c, tiny, one * 4, one * 4, 1, buf), word="odd")
    refused("sh_mod_poly_mul", L.sh_mod_poly_mul(c, even, w, k, one, 1, one, 1, buf), word="odd")
    refused("sh_mod_poly_mul", L.sh_mod_poly_mul(c, m, w, k, one, (1 << 25) + 1, one, 1, buf), word="2^25")
    refused("sh_mod_poly_mul", L.sh_mod_poly_mul(c, m, w, k, one, 1 << 24, one, (1 << 24) + 2, buf), word="2^25")
    refused("sh_mod_poly_mul", L.sh_mod_poly_mul(c, m, w, k, None, 1, one, 1, buf), word="null")
    refused("sh_mod_poly_divmod", L.sh_mod_poly_divmod(c, m, w, k, one, 1, one, 0, buf, buf), word="empty")
    refused("sh_mod_poly_divmod", L.sh_mod_poly_divmod(c, m, w, k, one, 1, wire(p, [1, 0]), 2, buf, buf), word="leading")
    refused("sh_mod_poly_divmod", L.sh_mod_poly_divmod(c, m, w, k, one, 1, wire(p, [1, p]), 2, buf, buf), word="leading")  # == 0 mod p
    refused("sh_mod_poly_divmod", L.sh_mod_poly_divmod(c, m, w, k, one, (1 << 24) + 1, one, 1, buf, buf), word="2^24")
    refused("sh_mod_zpoly", L.sh_mod_zpoly(c, m, w, k, one, (1 << 20) + 1, buf), word="2^20")
    refused("sh_mod_zpoly", L.sh_mod_zpoly(c, m, None, k, one, 1, buf), word="null")
    refused("sh_mod_lagrange_interp", L.sh_mod_lagrange_interp(c, m, w, k, one, one, (1 << 20) + 1, buf), word="2^20")
    refused("sh_mod_lagrange_interp", L.sh_mod_lagrange_interp(c, None, w, k, one, one, 1, buf), word="null")
    assert buf.raw == poison  # nothing was written
    # the empty cases
    assert L.sh_mod_poly_mul(c, m, w, k, one, 0, one, 1, buf) == 0
    assert L.sh_mod_lagrange_interp(c, m, w, k, one, one, 0, buf) == 0
    assert L.sh_mod_multi_inv(c, m, one, 0, buf) == 0 and L.sh_mod_multi_interp_4(c, m, one, one, 0, buf) == 0
    assert L.sh_mod_poly_divmod(c, m, w, k, one, 0, one, 1, buf, buf) == 0
    assert buf.raw == poison
    assert L.sh_mod_zpoly(c, m, w, k, b"", 0, buf) == 0 and ints(buf.raw[:32]) == [1]
    # device forms: overlaps, and a divisor whose leading coefficient is zero mod p (the one read-back), before any launch
    d = Dev(L, c, 64)
    try:
        d.put(0, [0xee] * 64)
        d.put(8, [1, 2, 3, p])  # a divisor ending in p == 0
        at = d.at
        refused("sh_dev_mod_poly_mul", L.sh_dev_mod_poly_mul(c, m, w, k, at(0), 8, at(8), 8, at(4)), word="overlap")
        refused("sh_dev_mod_zpoly", L.sh_dev_mod_zpoly(c, m, w, k, at(0), 8, at(7)), word="overlap")
        refused("sh_dev_mod_lagrange_interp", L.sh_dev_mod_lagrange_interp(c, m, w, k, at(0), at(8), 8, at(15)), word="overlap")
        refused("sh_dev_mod_poly_divmod", L.sh_dev_mod_poly_divmod(c, m, w, k, at(0), 8, at(8), 4, at(9), at(40)), word="overlap")
        refused("sh_dev_mod_poly_divmod", L.sh_dev_mod_poly_divmod(c, m, w, k, at(0), 8, at(8), 4, at(20), at(20)), word="overlap")
        refused("sh_dev_mod_poly_divmod", L.sh_dev_mod_poly_divmod(c, m, w, k, at(0), 8, at(8), 4, at(20), at(40)), word="leading")
        refused("sh_dev_mod_multi_inv", L.sh_dev_mod_multi_inv(c, m, at(0), at(4), 8), word="overlap")
        refused("sh_dev_mod_multi_interp_4", L.sh_dev_mod_multi_interp_4(c, m, at(0), at(16), 2, at(4)), word="overlap")
        refused("sh_dev_mod_multi_inv", L.sh_dev_mod_multi_inv(c, even, at(0), at(16), 8), word="odd")
        refused("sh_dev_mod_zpoly", L.sh_dev_mod_zpoly(c, m, w, 4, at(0), 8, at(20)), ROOT_ORDER, "order")
        _lib.check(L.sh_sync(c), "sh_sync")
        assert d.get(16, 48) == [0xee] * 48  # nothing was written
        # in-place forms that ARE allowed
        d.put(0, [3, 5, 0, p + 7])
        assert L.sh_dev_mod_multi_inv(c, m, at(0), at(0), 4) == 0
        assert d.get(0, 4) == mp.multi_inv(p, [3, 5, 0, 7])
    finally:
        d.free()
    assert len(set(names)) == 12


# ---- contexts ------------------------------------------------------------------------------------------------------------------------
def test_two_contexts_and_mimc_calls_interleaved(L):
    """two contexts with different moduli, MiMC calls in between on one of them: the single-context bytes"""
    from starks_amd import _lib
    from starks_amd.polynomial import mod_mul_wire, mul_wire
    from starks_amd.poly_utils import lagrange_interp_wire, mod_lagrange_interp_wire, mod_zpoly_wire
    c1, c2 = _lib.ctx(), _lib.second_ctx()
    rnd = random.Random(31)
    n = 2500
    pa, pb = mp.BN254, mp.GOLDILOCKS
    xa, ya, xb, yb = (_rand_wire(rnd, q, n) for q in (pa, pa, pb, pb))
    want = [mod_lagrange_interp_wire(pa, xa, ya), mod_lagrange_interp_wire(pb, xb, yb), lagrange_interp_wire(xa, ya),
            mod_mul_wire(pb, xb, yb), mod_zpoly_wire(pa, xa)]
    ma, wa, ka = _args(pa)
    mb_, wb, kb = _args(pb)
    out = [ctypes.create_string_buffer(32 * (2 * n)) for _ in range(5)]
    for _ in range(2):
        _lib.check(L.sh_mod_lagrange_interp(c1, ma, wa, ka, xa, ya, n, out[0]), "bn254 on ctx 1")
        _lib.check(L.sh_mod_lagrange_interp(c2, mb_, wb, kb, xb, yb, n, out[1]), "goldilocks on ctx 2")
        _lib.check(L.sh_lagrange_interp(c1, xa, ya, n, out[2]), "mimc on ctx 1")
        _lib.check(L.sh_mod_poly_mul(c1, mb_, wb, kb, xb, n, yb, n, out[3]), "goldilocks on ctx 1")
        _lib.check(L.sh_mod_zpoly(c2, ma, wa, ka, xa, n, out[4]), "bn254 on ctx 2")
        assert mul_wire(xa[:3200], ya[:3200]) == mul_wire(xa[:3200], ya[:3200])
        assert [out[0].raw[:32 * n], out[1].raw[:32 * n], out[2].raw[:32 * n], out[3].raw[:32 * (2 * n - 1)], out[4].raw[:32 * (n + 1)]] == want


# ---- Python routing ------------------------------------------------------------------------------------------------------------------
def test_python_routing(L):
    """Polynomial and poly_utils over BN254 at and above the thresholds return WireList-backed results equal to the host loops'"""
    from starks_amd import IntegersModP, _lib, poly_utils, polynomial
    from starks_amd.polynomial import polynomials_over
    from starks_amd.wireseq import WireList
    assert _lib._ctx is not None
    if None in list(polynomial.MOD_DEVICE_MIN.values()) + list(poly_utils.MOD_DEVICE_MIN.values()):
        pytest.fail("routing thresholds are not set: profiles/r21_mod_poly.json has not been measured")
    p = mp.BN254
    F = IntegersModP(p)
    Poly = polynomials_over(F)
    rnd = random.Random(5)
    n = max(polynomial.MOD_DEVICE_MIN.values())
    a, b = [rnd.randrange(p) for _ in range(2 * n)], [rnd.randrange(p) for _ in range(n)]  # the shorter side is at the threshold
    prod = Poly(a) * Poly(b)
    assert isinstance(prod.coefficients, WireList) and [int(v) for v in prod] == strip(mp.mul(p, a, b))
    q, r = divmod(Poly(a), Poly(b))
    assert isinstance(q.coefficients, WireList) and ([int(v) for v in q], [int(v) for v in r]) == tuple(strip(x) for x in mp.divmod_(p, a, b))
    assert Poly(a) / Poly(b) == q and Poly(a) % Poly(b) == r
    small = Poly(a[:2]) * Poly(b[:2])  # below the threshold: the host loop, the same values
    assert not isinstance(small.coefficients, WireList) and [int(v) for v in small] == strip(mp.mul(p, a[:2], b[:2]))
    m = poly_utils.MOD_DEVICE_MIN
    xs = [rnd.randrange(p) for _ in range(max(m["zpoly"], m["lagrange_interp"]))]
    z = poly_utils.zpoly(F, xs[:m["zpoly"]])
    assert isinstance(z.coefficients, WireList) and [int(v) for v in z] == mp.zpoly(p, xs[:m["zpoly"]])
    k = m["lagrange_interp"]
    lg = poly_utils.lagrange_interp(F, xs[:k], a[:k] if len(a) >= k else (a * k)[:k])
    assert isinstance(lg.coefficients, WireList) and [int(v) for v in lg] == strip(mp.lagrange(p, xs[:k], (a * k)[:k]))
    vals = [F(v) for v in (a * (m["multi_inv"] // len(a) + 1))[:m["multi_inv"]]]
    vals[3] = F(0)
    inv = poly_utils.multi_inv(F, vals)
    want = mp.multi_inv(p, [int(v) for v in vals])
    want[3] = 1  # the reference's 1 for a zero field element
    assert isinstance(inv, WireList) and [int(v) for v in inv] == want
    rows = m["multi_interp_4"]
    x4 = [[F(rnd.randrange(p)) for _ in range(4)] for _ in range(rows)]
    y4 = [[F(rnd.randrange(p)) for _ in range(4)] for _ in range(rows)]
    got = poly_utils.multi_interp_4(F, x4, y4)
    for r_ in (0, rows - 1):
        assert [int(v) for v in got[r_]] == strip(mp.lagrange(p, [int(v) for v in x4[r_]], [int(v) for v in y4[r_]]))


if __name__ == "__main__" and sys.argv[1:] == ["tile-child"]:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    cases = [c for c in mp.resolved(json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mod_poly.json"))))
             if c["p"] in (mp.BN254, 65537)]
    print(_digest(cases))
