"""Polynomial evaluation at arbitrary points on packed 64-bit words on the MI355X (sh_mod64_poly_eval / sh_dev_mod64_poly_eval of
include/starkhip.h; csrc/mod64eval.hip, mod64eval_items.cuh, api_mod64poly.hip; polynomial.mod64_eval_words): the words of
tests/golden/mod_poly_eval.json below 2^64 (the live reference over IntegersModP(p)); exact against Python-int Horner around the group
size, the workgroup split and the transform's tile over ten moduli, unreduced words among the inputs; word for word the 32-byte twin on
the same values; both forced paths byte-identical in fresh child processes; consistent with the packed transform; every refusal with
its code and the entry's name.  All comparisons are exact."""
import ctypes
import hashlib
import os
import random
import struct
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import load_golden  # noqa: E402
import mod64eval_cases as mc  # noqa: E402
import modpoly_cases as mp  # noqa: E402
from mod64eval_cases import FIELDS, IDS, evaluate, unwords, words  # noqa: E402

pytestmark = pytest.mark.gpu

INVALID, ROOT_ORDER, UNSUPPORTED = -1, -2, -6
POISON = 2**64 - 1
FORCED = [(1000, 3, 1), (1025, 129, 1), (5000, 300, 2), (1 << 12, 1 << 10, 1)]
SMALL = [3, 97, mc.BIG]  # 2-adicity 1, 5 and 2: no tree fits 129 points


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
    return _lib.mod64_poly_args(p, root)


def _err(L):
    from starks_amd import _lib
    return L.sh_last_error(_lib.ctx()).decode()


def _host(L, ctx, p, coefs, xs, batch=1, root=None):
    """sh_mod64_poly_eval on ints (any 64-bit values) -> ints"""
    from starks_amd import _lib
    m, w, k = _args(p, root)
    n = len(coefs) // batch
    out = ctypes.create_string_buffer(8 * max(batch * len(xs), 1))
    rc = L.sh_mod64_poly_eval(ctx, m, w, k, words(p, coefs) if n else None, n, batch, words(p, xs) if xs else None, len(xs), out)
    _lib.check(rc, "sh_mod64_poly_eval")
    return unwords(out.raw[:8 * batch * len(xs)])


class Dev(object):
    """a device buffer of `size`-byte elements (8: words, 32: limbs), little-endian ints up and down, unreduced"""

    def __init__(self, L, c, elems, size=8):
        from starks_amd import _lib
        self.L, self.c, self.d, self._lib, self.size = L, c, ctypes.c_void_p(), _lib, size
        _lib.check(L.sh_dev_alloc(c, size * max(elems, 1), ctypes.byref(self.d)), "sh_dev_alloc")

    def at(self, k):
        return ctypes.c_void_p(self.d.value + self.size * k)

    def put(self, k, vals):
        vals = list(vals)
        raw = struct.pack("<%dQ" % len(vals), *vals) if self.size == 8 else b"".join(int(v).to_bytes(32, "little") for v in vals)
        if raw:
            self._lib.check(self.L.sh_dev_upload(self.c, raw, self.at(k), len(raw)), "sh_dev_upload")

    def get(self, k, n):
        buf = ctypes.create_string_buffer(self.size * max(n, 1))
        if n:
            self._lib.check(self.L.sh_dev_download(self.c, self.at(k), buf, self.size * n), "sh_dev_download")
        if self.size == 8:
            return list(struct.unpack("<%dQ" % n, buf.raw[:8 * n]))
        return [int.from_bytes(buf.raw[32 * i:32 * (i + 1)], "little") for i in range(n)]

    def free(self):
        self.L.sh_dev_free(self.c, self.d)


def _dev(L, ctx, p, coefs, xs, batch=1, root=None, shift=0):
    """sh_dev_mod64_poly_eval on ints -> ints; the output area is poisoned first.  shift = 1 puts every array on an odd word: 8-byte
    alignment only, the kernels' two-word accesses fall back to single words"""
    from starks_amd import _lib
    m, w, k = _args(p, root)
    nc, nx = len(coefs), len(xs)
    o_c, o_x = shift, shift + nc + (nc & 1)
    o_o = o_x + nx + (nx & 1)
    d = Dev(L, ctx, o_o + batch * nx + 4)
    try:
        d.put(o_c, coefs)
        d.put(o_x, xs)
        d.put(o_o, [POISON] * (batch * nx))
        rc = L.sh_dev_mod64_poly_eval(ctx, m, w, k, d.at(o_c) if nc else None, nc // batch, batch, d.at(o_x) if nx else None, nx,
                                      d.at(o_o) if nx else None)
        _lib.check(rc, "sh_dev_mod64_poly_eval")
        return d.get(o_o, batch * nx)
    finally:
        d.free()


_WANT = {}


def _case(p, n, m, batch=1):
    key = (p, n, m, batch)
    if key not in _WANT:
        coefs, xs = mc.word_inputs(p, n, m, batch)
        _WANT[key] = (coefs, xs, evaluate(p, coefs, xs, batch))
    return _WANT[key]


# ---- the fixture and exact Horner -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [mc.GOLDILOCKS, 65537, 97], ids=IDS.get)
def test_fixture_words(L, ctx, p):
    mine = [c for c in mp.resolved(load_golden("mod_poly_eval.json")) if c["p"] == p]
    assert len(mine) == 18
    for c in mine:
        coefs, xs = [v % p for v in c["a"]], [v % p for v in c["xs"]]
        assert mp.matches(c["out"], _host(L, ctx, p, coefs, xs)), ("host", c["name"])
        assert mp.matches(c["out"], _dev(L, ctx, p, coefs, xs)), ("dev", c["name"])


SHAPES = [(1, 1, 1), (255, 3, 1), (256, 4, 1), (257, 5, 1), (1025, 9, 1), (1000, 1000, 1), (1025, 1025, 1), ((1 << 15) + 5, 5, 1),
          (1 << 16, 1, 1), (9, 7, 3), (1025, 2, 3), (0, 5, 3)] + [(257, m, 1) for m in mc.GROUP_MS]


@pytest.mark.parametrize("n,m,batch", SHAPES)
def test_exact_goldilocks(L, ctx, n, m, batch):
    """the group size (m = G - 1, G, G + 1, 2 G + 1), the transform's 2^10 tile (1000 and 1025 points), W > 1 (2^15 + 5 and 2^16 coefficients),
    batches and n = 0; inputs stored unreduced, the point 0 and a repeated point; both call forms, and the device form once more on
    arrays that are only 8-byte aligned"""
    p = mc.GOLDILOCKS
    coefs, xs, want = _case(p, n, m, batch)
    if n >= 1 << 15:
        assert mc.direct_shape(n, m, batch, mc.M6E_GROUP)[0] > 1
    assert _dev(L, ctx, p, coefs, xs, batch) == want
    assert _dev(L, ctx, p, coefs, xs, batch, shift=1) == want
    assert _host(L, ctx, p, coefs, xs, batch) == want


# (n, m, batch) -> (W, lanes per unit SL = min(W, 64), 16-byte pairs when the arrays are aligned): every way through m6e_sum_kernel
SUMS = {(1 << 20, 1, 1): (64, 64, False), (1 << 21, 1, 1): (128, 64, False), (1 << 16, 2, 1): (4, 4, True), (1 << 16, 4, 1): (4, 4, True),
        (1 << 17, 4, 1): (8, 8, True), (1 << 18, 2, 1): (16, 16, True), (1 << 15, 2, 3): (2, 2, True), (1 << 15, 3, 2): (2, 2, False)}


@pytest.mark.parametrize("n,m,batch", list(SUMS), ids=lambda v: str(v))
def test_sum_of_the_workgroups(L, ctx, n, m, batch):
    """the second launch of the direct path on the shapes it is shaped for: W = 64 (every lane of a wave one load), W = 128 (two loads
    per lane: the strided loop), W = 2 .. 16 (shuffles over part of a wave), an even m (the 16-byte pairs, one polynomial and a batch)
    and an odd m in a batch (single words); each on 16-byte aligned arrays and on arrays at an odd word.  root_log = 0 keeps every call on the direct path"""
    p = mc.GOLDILOCKS
    W, SL, pairs = SUMS[(n, m, batch)]
    assert mc.direct_shape(n, m, batch, mc.M6E_GROUP)[0] == W and min(W, 64) == SL and pairs == (m % 2 == 0)
    rnd = random.Random(n + 7 * m + batch)
    coefs = [rnd.getrandbits(64) for _ in range(batch * n)]  # any words: about 2^-32 of them at or above p
    coefs[5], coefs[n - 1] = p, POISON
    xs = [rnd.getrandbits(64) for _ in range(m)]
    want = evaluate(p, coefs, xs, batch)
    assert _dev(L, ctx, p, coefs, xs, batch, root=(1, 0)) == want
    assert _dev(L, ctx, p, coefs, xs, batch, root=(1, 0), shift=1) == want
    assert _host(L, ctx, p, coefs, xs, batch, root=(1, 0)) == want


@pytest.mark.parametrize("p", [q for q in FIELDS if q != mc.GOLDILOCKS], ids=IDS.get)
def test_exact_other_fields(L, ctx, p):
    """unreduced words, p itself and 2^64 - 1 among the inputs; the default path (tree where the rule and the field allow it)"""
    for n, m, batch in [(257, 5, 1), (1000, 3, 1), (129, 129, 2)]:
        coefs, xs, _ = _case(p, n, m, batch)
        coefs, xs = list(coefs), list(xs)
        coefs[3], coefs[4], xs[1], xs[m - 1] = p, POISON, p, POISON
        want = evaluate(p, coefs, xs, batch)
        assert sum(v >= p for v in coefs) >= 2 and sum(v >= p for v in xs) >= 2  # at 2^64 - 59 few residues have a second word
        assert _dev(L, ctx, p, coefs, xs, batch) == want, (n, m, batch)
        assert _host(L, ctx, p, coefs, xs, batch) == want, (n, m, batch)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.BABYBEAR], ids=IDS.get)
def test_equals_the_twin_word_for_word(L, ctx, p):
    """sh_dev_mod_poly_eval over the same modulus on the values after sh_dev_mod64_to_limbs, brought back by sh_dev_mod64_from_limbs"""
    from starks_amd import _lib
    gm, gw, gk = _lib.mod_poly_args(p)
    for n, m in ((3000, 5), (1 << 17, 1 << 17)):  # one shape the rule sends to the direct path and one to the tree
        assert mc.direct_preferred(mc.M6E_COST, n, m, 1) == (m == 5)
        rnd = random.Random(n + m)
        coefs, xs = [rnd.getrandbits(64) for _ in range(n)], [rnd.getrandbits(64) for _ in range(m)]  # any words, most at or above p
        some = [0, 1, m - 1]  # the yardstick is the twin; a few points against exact values too
        wd, ld = Dev(L, ctx, n + m + 2 * m + 8), Dev(L, ctx, n + 2 * m + 8, 32)
        try:
            o_x, o_o, o_t = n + (n & 1), n + (n & 1) + m + (m & 1), n + (n & 1) + 2 * (m + (m & 1))
            wd.put(0, coefs)
            wd.put(o_x, xs)
            _lib.check(L.sh_dev_mod64_to_limbs(ctx, wd.at(0), ld.at(0), n), "to_limbs")
            _lib.check(L.sh_dev_mod64_to_limbs(ctx, wd.at(o_x), ld.at(n), m), "to_limbs")
            _lib.check(L.sh_dev_mod_poly_eval(ctx, gm, gw, gk, ld.at(0), n, 1, ld.at(n), m, ld.at(n + m)), "sh_dev_mod_poly_eval")
            _lib.check(L.sh_dev_mod64_from_limbs(ctx, p, ld.at(n + m), wd.at(o_t), m), "from_limbs")
            mod, w, k = _args(p)
            _lib.check(L.sh_dev_mod64_poly_eval(ctx, mod, w, k, wd.at(0), n, 1, wd.at(o_x), m, wd.at(o_o)), "sh_dev_mod64_poly_eval")
            got = wd.get(o_o, m)
            assert got == wd.get(o_t, m), (n, m)
            assert [got[i] for i in some] == evaluate(p, coefs, [xs[i] for i in some]), (n, m)
        finally:
            wd.free()
            ld.free()


# ---- forced paths, each in a fresh child process ------------------------------------------------------------------------------------
def _path_digests():
    """what a child prints: one sha256 per FORCED shape over Goldilocks (host-buffer form), then per modulus of SMALL the code, the
    text and the output words of m = 129 with root = (1, 0) into a prefilled buffer"""
    from starks_amd import _lib
    L, c = _lib.lib(), _lib.ctx()
    lines = []
    for n, m, batch in FORCED:
        coefs, xs = mc.word_inputs(mc.GOLDILOCKS, n, m, batch)
        lines.append(hashlib.sha256(words(mc.GOLDILOCKS, _host(L, c, mc.GOLDILOCKS, coefs, xs, batch))).hexdigest())
    for q in SMALL:
        coefs, xs = mc.word_inputs(q, 50, 129)
        out = ctypes.create_string_buffer(b"\xa5" * (8 * 129), 8 * 129)
        rc = L.sh_mod64_poly_eval(c, q, 1, 0, words(q, coefs), 50, 1, words(q, xs), 129, out)
        lines.append("%d %s|%s" % (rc, L.sh_last_error(c).decode() if rc else "", hashlib.sha256(out.raw).hexdigest()))
    return lines


def test_forced_paths_are_byte_identical(L, ctx):
    """STARKHIP_EVAL_PATH=direct and =tree in child processes started fresh: the same bytes as each other and as this process's
    default choice; the first three shapes also against exact values.  Over 3, 97 and 2^64 - 59 with root = (1, 0) at 129 points the
    default and the forced direct path run, a forced tree returns SH_ERR_ROOT_ORDER ("needs") and leaves the prefilled output untouched"""
    got = {}
    for path in ("direct", "tree"):
        env = dict(os.environ, STARKHIP_EVAL_PATH=path)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "path-child"], capture_output=True, text=True, env=env, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        got[path] = out.stdout.strip().splitlines()[-len(FORCED) - len(SMALL):]
    mine = _path_digests()
    k = len(FORCED)
    assert got["direct"][:k] == got["tree"][:k] == mine[:k]
    for (n, m, batch), digest in zip(FORCED[:3], mine):
        assert digest == hashlib.sha256(words(mc.GOLDILOCKS, _case(mc.GOLDILOCKS, n, m, batch)[2])).hexdigest(), (n, m, batch)
    for j, q in enumerate(SMALL):
        coefs, xs = mc.word_inputs(q, 50, 129)
        assert got["direct"][k + j] == mine[k + j] == "0 |" + hashlib.sha256(words(q, evaluate(q, coefs, xs))).hexdigest(), q
        head, digest = got["tree"][k + j].split("|")
        code, text = head.split(" ", 1)
        assert int(code) == ROOT_ORDER and text.startswith("sh_mod64_poly_eval: ") and "needs" in text, q
        assert digest == hashlib.sha256(b"\xa5" * (8 * 129)).hexdigest(), q


def test_grid_shape_never_changes_a_bit(L, ctx):
    """one polynomial of 2^16 coefficients: W = 4 at 5 points (a full group and a group of one) and at 1 point (one point per lane),
    against exact values; root_log = 0 keeps both calls on the direct path"""
    p, n = mc.GOLDILOCKS, 1 << 16
    coefs, xs, want = _case(p, n, 5)
    assert mc.direct_shape(n, 5, 1, mc.M6E_GROUP) == (4, 64, mc.M6E_GROUP) and mc.direct_shape(n, 1, 1, mc.M6E_GROUP) == (4, 64, 1)
    assert _dev(L, ctx, p, coefs, xs, root=(1, 0)) == want
    assert _dev(L, ctx, p, coefs, xs[:1], root=(1, 0)) == want[:1]


@pytest.mark.parametrize("p", [3, 97, mc.BIG], ids=IDS.get)
def test_small_two_adicity_runs_direct(L, ctx, p):
    coefs, xs, want = _case(p, 300, 129)
    assert _dev(L, ctx, p, coefs, xs, root=(1, 0)) == want
    assert _host(L, ctx, p, coefs, xs, root=(1, 0)) == want
    assert _dev(L, ctx, p, coefs, xs) == want  # the field's own root: the tree needs 512


# ---- results pinned elsewhere, context behaviour ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.BABYBEAR], ids=IDS.get)
def test_consistent_with_the_transform(L, ctx, p):
    """1024 coefficients at the 1024 powers of the root: sh_dev_mod64_ntt's forward transform"""
    from starks_amd import _lib
    n = 1 << 10
    w, k = mc.two_adic_root(p)
    w = pow(w, 1 << (k - 10), p)
    coefs = mc.word_inputs(p, n, 1)[0]
    xs, x = [], 1
    for _ in range(n):
        xs.append(x)
        x = x * w % p
    d = Dev(L, ctx, 2 * n)
    try:
        d.put(0, coefs)
        _lib.check(L.sh_dev_mod64_ntt(ctx, p, d.at(0), n, d.at(n), n, 1, w, 0), "sh_dev_mod64_ntt")
        want = d.get(n, n)
    finally:
        d.free()
    assert _dev(L, ctx, p, coefs, xs) == want
    assert want[0] == sum(coefs) % p


def test_moduli_twin_and_mimc_calls_interleave(L, ctx):
    from starks_amd.polynomial import eval_wire, mod_eval_wire
    p1, p2 = mc.GOLDILOCKS, 97
    c1, x1, w1 = _case(p1, 1025, 9)
    c2, x2, w2 = _case(p2, 129, 129, 2)
    cg, xg = mp.vec(mp.BN254, 5, 300, 5), mp.vec(mp.BN254, 6, 33, 3)
    wg = evaluate(mp.BN254, cg, xg)
    cm, xm = mp.vec(mp.MIMC_P, 7, 257, 5), mp.vec(mp.MIMC_P, 8, 5, 3)
    wm = evaluate(mp.MIMC_P, cm, xm)
    for _ in range(2):
        assert _dev(L, ctx, p1, c1, x1) == w1
        assert mp.ints(mod_eval_wire(mp.BN254, mp.wire(mp.BN254, cg), mp.wire(mp.BN254, xg))) == wg
        assert _host(L, ctx, p2, c2, x2, 2) == w2
        assert mp.ints(eval_wire(mp.wire(mp.MIMC_P, cm), mp.wire(mp.MIMC_P, xm))) == wm
        assert _host(L, ctx, p1, c1, x1) == w1


def test_refusals(L, ctx):
    """every refusal of the contract, before any launch, with the entry's name opening sh_last_error; the output stays as it was"""
    p = mc.GOLDILOCKS
    m, w, k = _args(p)
    d = Dev(L, ctx, 64)
    try:
        d.put(0, list(range(64)))
        A, X, O = d.at(0), d.at(16), d.at(32)

        def dev(code, word, mod=m, root=w, rl=k, coefs=A, n=8, batch=1, xs=X, mm=4, out=O):
            assert L.sh_dev_mod64_poly_eval(ctx, mod, root, rl, coefs, n, batch, xs, mm, out) == code, word
            assert _err(L).startswith("sh_dev_mod64_poly_eval: ") and word in _err(L), _err(L)

        dev(INVALID, "batch", batch=0)
        dev(INVALID, "null", coefs=None)
        dev(INVALID, "null", xs=None)
        dev(INVALID, "null", out=None)
        dev(UNSUPPORTED, "2^25", n=(1 << 25) + 1)
        dev(UNSUPPORTED, "2^26", n=1 << 25, batch=3)
        dev(UNSUPPORTED, "2^20", mm=(1 << 20) + 1)
        dev(INVALID, "overlaps", out=d.at(7))    # the last coefficient
        dev(INVALID, "overlaps", out=d.at(13))   # [13, 17) reaches the first point
        dev(INVALID, "overlaps", out=A, n=0, coefs=None, xs=d.at(3))
        dev(INVALID, "modulus", mod=p + 1)
        dev(INVALID, "modulus", mod=0)
        dev(INVALID, "modulus", mod=1)
        dev(UNSUPPORTED, "28", root=1, rl=29)
        dev(ROOT_ORDER, "below", mod=97, root=97 + 28, rl=5)
        dev(ROOT_ORDER, "order", rl=k - 1)
        dev(ROOT_ORDER, "order", root=1)
        assert d.get(32, 4) == [32, 33, 34, 35]  # nothing was launched
        # valid degenerate calls: m = 0 with null xs and out writes nothing; n = 0 with null coefs writes zeros; out directly behind xs
        assert L.sh_dev_mod64_poly_eval(ctx, m, w, k, A, 8, 1, None, 0, None) == 0
        assert L.sh_dev_mod64_poly_eval(ctx, m, w, k, None, 0, 2, X, 4, d.at(20)) == 0
        assert d.get(20, 8) == [0] * 8 and d.get(28, 1) == [28]
        assert L.sh_dev_mod64_poly_eval(ctx, m, 1, 0, A, 8, 1, X, 4, O) == 0
        assert d.get(32, 4) == evaluate(p, list(range(8)), [16, 17, 18, 19])
    finally:
        d.free()
    buf = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    co, xs = words(p, range(8)), words(p, range(4))

    def host(code, word, mod=m, root=w, rl=k, coefs=co, n=8, batch=1, pts=xs, mm=4, out=buf):
        assert L.sh_mod64_poly_eval(ctx, mod, root, rl, coefs, n, batch, pts, mm, out) == code, word
        assert _err(L).startswith("sh_mod64_poly_eval: ") and word in _err(L), _err(L)

    host(INVALID, "batch", batch=0)
    host(INVALID, "null", coefs=None)
    host(INVALID, "null", pts=None)
    host(INVALID, "null", out=None)
    host(UNSUPPORTED, "2^25", n=(1 << 25) + 1)
    host(UNSUPPORTED, "2^26", n=1 << 24, batch=5)
    host(UNSUPPORTED, "2^20", mm=(1 << 20) + 1)
    host(INVALID, "modulus", mod=2**40)
    host(UNSUPPORTED, "28", root=1, rl=29)
    host(ROOT_ORDER, "below", root=p)
    host(ROOT_ORDER, "order", rl=k - 2)
    assert buf.raw == b"\xa5" * 64
    assert L.sh_mod64_poly_eval(ctx, m, w, k, None, 0, 1, None, 0, None) == 0


# ---- Python ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [mc.GOLDILOCKS, 97], ids=IDS.get)
def test_python_form(L, ctx, p):
    from array import array
    from starks_amd.polynomial import mod64_eval_words
    coefs, xs, want = _case(p, 129, 129, 2)
    for c, x in ((coefs, xs), (words(p, coefs), words(p, xs)), (memoryview(array("Q", coefs)), memoryview(array("Q", xs)))):
        out = mod64_eval_words(p, c, x, batch=2)
        assert isinstance(out, memoryview) and out.format == "Q" and list(out) == want
    assert list(mod64_eval_words(p, coefs, xs, batch=2, root=(1, 0))) == want
    assert list(mod64_eval_words(p, [], xs[:3])) == [0, 0, 0] and len(mod64_eval_words(p, coefs, [])) == 0
    with pytest.raises(ValueError):
        mod64_eval_words(p, coefs[:5], xs, batch=2)


if __name__ == "__main__" and sys.argv[1:] == ["path-child"]:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    print("\n".join(_path_digests()))
