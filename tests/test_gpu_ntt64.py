"""The packed-word transform (sh_mod64_ntt, sh_dev_mod64_ntt, sh_mod64_mul_polys, sh_dev_mod64_from_limbs / _to_limbs: any odd modulus
below 2^64 on native 64-bit words, starks_amd/csrc/fp64m.cuh and ntt64_items.cuh) on the MI355X: every size 2^0 .. 2^14 over eleven
moduli against the exact oracle of tests/modntt_cases.py and tests/golden/mod64_ntt.json (the live reference's fft_1d / mul_polys);
forced plans in child processes; the generic 32-byte path as yardstick up to 2^24; the 2^28 limit; a low-degree extension and its
commitment; two moduli on two contexts at once; the plan cache; the conversions; the Python entry points; the errors.  Every rejected
call is refused on the host before any launch.  All comparisons are exact."""
import array
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden
import modntt_cases as mc
import ntt64_cases as nc
from ntt64_cases import MODULI, ints, root_of, words

pytestmark = pytest.mark.gpu

OK, INVALID, ROOT_ORDER, UNSUPPORTED = 0, -1, -2, -6
GL, BIG = nc.GOLDILOCKS, nc.BIG18


def b32(x):
    return int(x).to_bytes(32, "big")


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def _ctx():
    from starks_amd import _lib
    return _lib.ctx()


def ntt64(L, p, vals, n, w, inv=False, batch=1, ctx=None):
    """sh_mod64_ntt on `vals` = batch * n_in ints; returns batch * n ints"""
    out = ctypes.create_string_buffer(8 * n * batch)
    rc = L.sh_mod64_ntt(ctx or _ctx(), p, words(vals), len(vals) // batch, out, n, batch, w, 1 if inv else 0)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))
    return ints(out.raw)


class Dev(object):
    """a device buffer of `nbytes` bytes on a context"""

    def __init__(self, L, nbytes, ctx=None):
        self.L, self.ctx, self.nbytes = L, ctx or _ctx(), nbytes
        self.ptr = ctypes.c_void_p()
        assert L.sh_dev_alloc(self.ctx, max(nbytes, 32), ctypes.byref(self.ptr)) == OK

    def put(self, raw):
        assert self.L.sh_dev_upload(self.ctx, raw, self.ptr, len(raw)) == OK
        return self

    def get(self, first=0, nbytes=None):
        nbytes = self.nbytes - first if nbytes is None else nbytes
        out = ctypes.create_string_buffer(nbytes)
        assert self.L.sh_dev_download(self.ctx, ctypes.c_void_p(self.ptr.value + first), out, nbytes) == OK
        return out.raw

    def words(self, first=0, count=None):
        return ints(self.get(8 * first, None if count is None else 8 * count))

    def free(self):
        assert self.L.sh_sync(self.ctx) == OK
        assert self.L.sh_dev_free(self.ctx, self.ptr) == OK


def dev_ntt64(L, p, src, n_in, dst, n, w, inv=False, batch=1, ctx=None):
    rc = L.sh_dev_mod64_ntt(ctx or _ctx(), p, src.ptr, n_in, dst.ptr, n, batch, w, 1 if inv else 0)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))


# ---- 1. every size -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_every_size(L, name):
    """n = 2^0 .. 2^14 as far as the modulus has roots, forward and inverse, n_in = 1, n / 2 + 1 and n, batch 1 and 3, inputs >= p
    included"""
    p = MODULI[name]
    top = min(14, nc.max_log(name))
    blob = nc.inputs(1234, 3 << top, p)
    for lg in range(top + 1):
        n, w = 1 << lg, root_of(name, 1 << lg)
        for inv in (False, True):
            s = pow(n, -1, p) if inv else 1
            assert ntt64(L, p, blob[:1], n, w, inv) == [blob[0] * s % p] * n, (name, lg, inv)  # one value: a constant vector
            for n_in in sorted({n // 2 + 1, n} - {1}):
                if n_in > n:
                    continue
                want = [mc.transform(blob[b * n_in:(b + 1) * n_in], n, p, w, inv) for b in range(3)]
                assert ntt64(L, p, blob[:n_in], n, w, inv) == want[0], (name, lg, n_in, inv)
                assert ntt64(L, p, blob[:3 * n_in], n, w, inv, batch=3) == want[0] + want[1] + want[2], (name, lg, n_in, inv)


def test_goldilocks_2_to_the_16(L):
    n, w = 1 << 16, root_of("goldilocks", 1 << 16)
    x = nc.inputs(16, n, GL)
    for inv in (False, True):
        assert ntt64(L, GL, x, n, w, inv) == mc.transform(x, n, GL, w, inv)
    assert ntt64(L, GL, x[:n // 2 + 1], n, w) == mc.transform(x[:n // 2 + 1], n, GL, w)


# ---- 2. the fixture ------------------------------------------------------------------------------------------------------------------
def test_fixture(L):
    """the live reference's fft_1d outputs over Goldilocks, BabyBear and 65537 at n = 8, 64, 1024"""
    for c in load_golden("mod64_ntt.json")["cases"]:
        n, p, w, s = c["n"], c["p"], c["root"], c["seed"]
        full, short = nc.inputs(s, n, p), nc.inputs(s + 1, n // 2 + 1, p)
        assert mc.recorded(ntt64(L, p, full, n, w)) == c["forward"]
        assert mc.recorded(ntt64(L, p, full, n, w, True)) == c["inverse"]
        assert mc.recorded(ntt64(L, p, short, n, w)) == c["padded"]


# ---- 3. forced plans (child processes: the knob is read once per process) ------------------------------------------------------------
PLAN_MODULI = ("goldilocks", "big18")


def _plan_inputs(name):
    return nc.inputs(4321, 5 << 12, MODULI[name])


def _digest(vals):
    return hashlib.sha256(words(vals)).hexdigest()


def _plan_child():
    """every n = 2^1 .. 2^12: batch 1 forward and inverse through sh_mod64_ntt, batch 5 forward IN PLACE through sh_dev_mod64_ntt"""
    from starks_amd import _lib
    L = _lib.lib()
    out = []
    for name in PLAN_MODULI:
        p, blob = MODULI[name], _plan_inputs(name)
        buf = Dev(L, 8 * (5 << 12))
        for lg in range(1, 13):
            n, w = 1 << lg, root_of(name, 1 << lg)
            out.append(_digest(ntt64(L, p, blob[:n], n, w)))
            out.append(_digest(ntt64(L, p, blob[:n], n, w, True)))
            buf.put(words(blob[:5 * n]))
            dev_ntt64(L, p, buf, n, buf, n, w, batch=5)
            out.append(_digest(buf.words(0, 5 * n)))
        buf.free()
    if os.environ.get("STARKHIP_MOD64_TILE_LOG") == "2":
        _grid_2d_round_trip(L)
    print(json.dumps(out))


def _grid_2d_round_trip(L):
    """tile log 2 at n = 2^25: 25 passes of 2^23 two-column tiles each, twice the 2^22 workgroups one grid row holds, so every launch
    takes the 2-D grid; forward then inverse in place = x mod p on eight 2^12-word windows, first and last included"""
    n, p = 1 << 25, GL
    w = root_of("goldilocks", n)
    c = _ctx()
    x, y = Dev(L, 8 * n), Dev(L, 8 * n)
    assert L.sh_dev_fill_seeded(c, x.ptr, n // 4, 25) == OK
    dev_ntt64(L, p, x, n, y, n, w)
    dev_ntt64(L, p, y, n, y, n, w, True)
    win = 1 << 12
    for i in range(8):
        first = (n - win) * i // 7
        assert y.words(first, win) == [v % p for v in x.words(first, win)], i
    for d in (x, y):
        d.free()


_PLAN_WANT = []


def _plan_want():
    if not _PLAN_WANT:
        for name in PLAN_MODULI:
            p, blob = MODULI[name], _plan_inputs(name)
            for lg in range(1, 13):
                n, w = 1 << lg, root_of(name, 1 << lg)
                _PLAN_WANT.append(_digest(mc.transform(blob[:n], n, p, w)))
                _PLAN_WANT.append(_digest(mc.transform(blob[:n], n, p, w, True)))
                _PLAN_WANT.append(_digest([v for b in range(5) for v in mc.transform(blob[b * n:(b + 1) * n], n, p, w)]))
    return _PLAN_WANT


@pytest.mark.parametrize("tile_log", [2, 3, 5, 8, 13])
def test_forced_plans(tile_log):
    """STARKHIP_MOD64_TILE_LOG = 2, 3, 5, 8: up to twelve passes, uneven radices, batch strides, at sizes the oracle covers; 13: the
    largest tile, 64 KiB of LDS; 2 also runs one 2^25-point round trip, whose launches take the 2-D grid"""
    env = dict(os.environ, STARKHIP_MOD64_TILE_LOG=str(tile_log))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "plan-child"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got, want = json.loads(out.stdout.strip().splitlines()[-1]), _plan_want()
    assert len(got) == len(want)
    assert [i for i, (g, w) in enumerate(zip(got, want)) if g != w] == []


# ---- 4. the generic path as yardstick at size ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lg,batch", [("goldilocks", 20, 1), ("goldilocks", 24, 1), ("goldilocks", 20, 8), ("big18", 18, 1)])
def test_equals_generic_path(L, name, lg, batch):
    """seeded 256-bit limbs -> from_limbs -> sh_dev_mod64_ntt -> to_limbs gives sh_dev_mod_ntt's bytes on the same limbs, forward and
    inverse"""
    n, p = 1 << lg, MODULI[name]
    w = root_of(name, n)
    total = n * batch
    c = _ctx()
    x, a, b, wd = Dev(L, 32 * total), Dev(L, 32 * total), Dev(L, 32 * total), Dev(L, 8 * total)
    assert L.sh_dev_fill_seeded(c, x.ptr, total, 64 + lg) == OK
    head = [int.from_bytes(x.get(32 * i, 32), "little") for i in range(16)]
    assert any(v >= p for v in head)  # 256-bit limbs: from_limbs' reduction is what this shape exercises at size
    assert L.sh_dev_mod64_from_limbs(c, p, x.ptr, wd.ptr, total) == OK
    assert wd.words(0, 16) == [v % p for v in head]
    for inv in (0, 1):
        assert L.sh_dev_mod_ntt(c, b32(p), x.ptr, a.ptr, n, batch, b32(w), inv) == OK, L.sh_last_error(c)
        dev_ntt64(L, p, wd, n, wd, n, w, bool(inv), batch)
        assert L.sh_dev_mod64_to_limbs(c, wd.ptr, b.ptr, total) == OK
        assert a.get() == b.get(), (name, lg, batch, inv)
        assert L.sh_dev_mod64_from_limbs(c, p, x.ptr, wd.ptr, total) == OK  # the next direction starts from the same input
    for d in (x, a, b, wd):
        d.free()


# ---- 5. the 2^28 limit -----------------------------------------------------------------------------------------------------------------
def test_limit_2_to_the_28(L):
    """one 2^28-point round trip over Goldilocks (the largest plan, four passes, offsets past 2^31 bytes): x -> forward -> inverse in
    place = x mod p, compared on sixteen 2^15-word windows spread over the vector, first and last included"""
    n, p = 1 << 28, GL
    w = root_of("goldilocks", n)
    c = _ctx()
    x, y = Dev(L, 8 * n), Dev(L, 8 * n)
    assert L.sh_dev_fill_seeded(c, x.ptr, n // 4, 28) == OK  # 2^26 seeded 32-byte values = 2^28 words of any 64-bit value
    dev_ntt64(L, p, x, n, y, n, w)
    dev_ntt64(L, p, y, n, y, n, w, True)
    win = 1 << 15
    for i in range(16):
        first = (n - win) * i // 15
        assert y.words(first, win) == [v % p for v in x.words(first, win)], i
    for d in (x, y):
        d.free()
    assert L.sh_ctx_trim(c) == OK  # the 2 GiB work buffer goes back


# ---- 6. a low-degree extension and its commitment ---------------------------------------------------------------------------------------
def test_lde_and_commitment(L):
    """a 2^10-step Goldilocks column: the inverse at 2^10, then the forward transform with n_in = 2^10 and n = 2^13; every 8th value
    is the trace, and to_limbs + sh_dev_merkelize gives the root of the hashlib tree over the 32-byte big-endian values"""
    steps, ext, p = 1 << 10, 8, GL
    n = steps * ext
    g2 = root_of("goldilocks", n)
    g1 = pow(g2, ext, p)
    trace = [v % p for v in nc.inputs(61, steps, p)]
    c = _ctx()
    t, ev, lm, tree = Dev(L, 8 * steps).put(words(trace)), Dev(L, 8 * n), Dev(L, 32 * n), Dev(L, 64 * n)
    dev_ntt64(L, p, t, steps, t, steps, g1, True)
    dev_ntt64(L, p, t, steps, ev, n, g2)
    vals = ev.words()
    assert vals[::ext] == trace
    assert vals == mc.transform(mc.transform(trace, steps, p, g1, True), n, p, g2)
    assert L.sh_dev_mod64_to_limbs(c, ev.ptr, lm.ptr, n) == OK
    assert L.sh_dev_merkelize(c, lm.ptr, n, 1, tree.ptr) == OK
    leaves = [b32(v) for v in vals]
    nodes = [b""] * n + [leaves[i + j * (n // 4)] for i in range(n // 4) for j in range(4)]
    for i in range(n - 1, 0, -1):
        nodes[i] = hashlib.blake2s(nodes[2 * i] + nodes[2 * i + 1]).digest()
    assert tree.get(32, 32) == nodes[1]
    for d in (t, ev, lm, tree):
        d.free()


# ---- 7. sh_mod64_mul_polys -----------------------------------------------------------------------------------------------------------
def mul_polys(L, p, a, b, n, w):
    out = ctypes.create_string_buffer(8 * n)
    rc = L.sh_mod64_mul_polys(_ctx(), p, words(a), len(a), words(b), len(b), out, n, w)
    assert rc == OK, (rc, L.sh_last_error(_ctx()))
    return ints(out.raw)


def test_mul_polys(L):
    for c in load_golden("mod64_ntt.json")["cases"]:
        n, p, s = c["n"], c["p"], c["seed"]
        assert mc.recorded(mul_polys(L, p, nc.inputs(s + 2, n // 2 + 1, p), nc.inputs(s + 3, n // 4 + 1, p), n, c["root"])) == c["mul_polys"]
    for name in ("goldilocks", "big18", "babybear", "f257", "composite", "all_ones"):
        p = MODULI[name]
        for lg in range(min(6, nc.max_log(name)) + 1):
            n = 1 << lg
            for n_a, n_b in sorted({(n, n), (n // 2 + 1, 1), (0, n)}):
                a, b = nc.inputs(lg, n_a, p), nc.inputs(lg + 50, n_b, p)
                assert mul_polys(L, p, a, b, n, root_of(name, n)) == mc.cyclic_times_n([v % p for v in a], [v % p for v in b], n, p)


# ---- 8. two moduli at once -----------------------------------------------------------------------------------------------------------
def test_two_moduli_on_two_contexts(L):
    """Goldilocks on one context and BabyBear on another, 2^16-point transforms enqueued alternately with no synchronisation in
    between: each result equals its single-context bytes (a modulus kept in a device global fails here)"""
    from starks_amd import _lib
    n, rounds = 1 << 16, 6
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    names = ["goldilocks", "babybear"]
    src, dst, want = [], [], []
    for c, name in zip(ctxs, names):
        s = Dev(L, 8 * n, c)
        assert L.sh_dev_fill_seeded(c, s.ptr, n // 4, 5) == OK
        d = [Dev(L, 8 * n, c) for _ in range(rounds)]
        dev_ntt64(L, MODULI[name], s, n, d[0], n, root_of(name, n), ctx=c)
        want.append(d[0].get())
        assert L.sh_sync(c) == OK
        src.append(s)
        dst.append(d)
    assert want[0] != want[1]
    x = src[0].words(0, 256)
    assert ints(want[0])[0] == sum(src[0].words()) % GL and len(x) == 256
    for r in range(rounds):
        for k in (0, 1):
            dev_ntt64(L, MODULI[names[k]], src[k], n, dst[k][r], n, root_of(names[k], n), ctx=ctxs[k])
    for k in (0, 1):
        assert L.sh_sync(ctxs[k]) == OK
        for r in range(rounds):
            assert dst[k][r].get() == want[k], (k, r)
    for k in (0, 1):
        for d in [src[k]] + dst[k]:
            d.free()


# ---- 9. plan cache -------------------------------------------------------------------------------------------------------------------
def _stats(L, c):
    out = (ctypes.c_uint64 * 4)()
    assert L.sh_ctx_stats(c, out) == OK
    return list(out)


def test_plan_cache(L):
    """the tables are a plan: counted, charged to the byte budget, evicted by the same LRU pass, dropped by sh_ctx_trim; a 32-byte
    plan and a packed-word plan of the same modulus and root are two plans"""
    from starks_amd import _lib
    c = ctypes.c_void_p()
    assert L.sh_ctx_create(_lib.default_device(), ctypes.byref(c)) == OK
    try:
        lg = 12
        n, w = 1 << lg, root_of("goldilocks", 1 << lg)
        bound = 8 * (2 ** ((lg + 1) // 2 + 1) + 2 ** 11)  # include/starkhip.h: 8 (2^(h+1) + 2^(t-1)), h = ceil(lg / 2), t = 12
        x = nc.inputs(8, n, GL)
        want = mc.transform(x, n, GL, w)
        assert _stats(L, c) == [0, 0, 0, 0]
        assert ntt64(L, GL, x, n, w, ctx=c) == want
        first = _stats(L, c)
        B = first[1]
        assert first == [1, B, 1, 0] and 0 < B <= bound
        assert B == 8 * (2 ** 6 + 2 ** 6 + 2 ** 5)  # lo | hi | the stage twiddles of the (6, 6) plan
        assert ntt64(L, GL, x, n, w, ctx=c) == want  # a hit: nothing is built
        assert _stats(L, c) == [1, B, 1, 0]
        out = ctypes.create_string_buffer(32 * n)
        assert L.sh_mod_ntt(c, b32(GL), mc.wire(x), n, out, n, 1, b32(w), 0) == OK
        assert mc.ints(out.raw) == want
        assert _stats(L, c) == [2, B + (32 << 11), 2, 0]  # the 32-byte path's table is a plan of its own
        assert L.sh_ctx_set_plan_budget(c, B - 1) == OK  # below either: everything goes
        assert _stats(L, c) == [0, 0, 2, 2]
        assert ntt64(L, GL, x, n, w, ctx=c) == want  # built again; the budget is checked on entry, so it stays for this call
        assert _stats(L, c) == [1, B, 3, 2]
        assert ntt64(L, GL, x, n, w, True, ctx=c) == mc.transform(x, n, GL, w, True)  # the entry evicts the forward plan
        assert _stats(L, c) == [1, B, 4, 3]
        assert L.sh_ctx_trim(c) == OK
        assert _stats(L, c)[:2] == [0, 0]
        assert ntt64(L, GL, x, n, w, ctx=c) == want
    finally:
        L.sh_ctx_destroy(c)


# ---- 10. errors and limits -------------------------------------------------------------------------------------------------------------
def test_errors(L):
    c, p = _ctx(), GL
    out, ones = ctypes.create_string_buffer(8 * 64), words([1] * 64)
    d = Dev(L, 8 * 128)
    w = root_of("goldilocks", 64)
    before = _stats(L, c)

    def three(mod, root, n, batch=1, n_in=None):
        n_in = min(n, 64) if n_in is None else n_in
        rc = L.sh_mod64_ntt(c, mod, ones, n_in, out, n, batch, root, 0)
        msg = L.sh_last_error(c).decode()
        assert L.sh_dev_mod64_ntt(c, mod, d.ptr, n_in, d.ptr, n, batch, root, 0) == rc
        if batch == 1:
            assert L.sh_mod64_mul_polys(c, mod, ones, n_in, ones, 1, out, n, root) == rc
        return rc, msg

    for bad in (p - 1, 0, 1, 2, 1 << 63):
        rc, msg = three(bad, 1, 1)
        assert rc == INVALID and "odd" in msg, (bad, msg)
    rc, msg = three(p, root_of("goldilocks", 32), 64)
    assert rc == ROOT_ORDER and "order" in msg
    rc, msg = three(p, root_of("goldilocks", 128), 64)
    assert rc == ROOT_ORDER and "order" in msg
    rc, msg = three(nc.BABYBEAR, nc.BABYBEAR + root_of("babybear", 64), 64)
    assert rc == ROOT_ORDER and "below" in msg
    rc, msg = three(p, p, 1)
    assert rc == ROOT_ORDER and "below" in msg
    rc, msg = three(p, 2, 1)
    assert rc == ROOT_ORDER and "order" in msg
    assert three(p, p - 1, 3)[0] == INVALID          # n is no power of two
    assert three(p, p - 1, 2, n_in=3)[0] == INVALID  # more inputs than n
    assert three(p, w, 64, batch=0)[0] == INVALID
    assert three(p, root_of("goldilocks", 1 << 29), 1 << 29)[0] == UNSUPPORTED
    assert three(p, root_of("goldilocks", 1 << 20), 1 << 20, batch=257)[0] == UNSUPPORTED
    assert L.sh_mod64_ntt(c, p, None, 64, out, 64, 1, w, 0) == INVALID
    assert L.sh_mod64_ntt(c, p, ones, 64, None, 64, 1, w, 0) == INVALID
    assert L.sh_dev_mod64_ntt(c, p, None, 64, d.ptr, 64, 1, w, 0) == INVALID
    assert L.sh_dev_mod64_ntt(c, p, d.ptr, 64, None, 64, 1, w, 0) == INVALID
    assert L.sh_mod64_mul_polys(c, p, None, 1, ones, 1, out, 64, w) == INVALID
    # overlap: the same buffer with n_in < n, and a shifted one
    assert L.sh_dev_mod64_ntt(c, p, d.ptr, 32, d.ptr, 64, 1, w, 0) == INVALID
    assert L.sh_dev_mod64_ntt(c, p, d.ptr, 64, ctypes.c_void_p(d.ptr.value + 8), 64, 1, w, 0) == INVALID
    assert L.sh_dev_mod64_from_limbs(c, 4, d.ptr, d.ptr, 1) == INVALID and "odd" in L.sh_last_error(c).decode()
    assert _stats(L, c) == before  # no table was built, nothing was launched
    assert L.sh_sync(c) == OK
    assert ntt64(L, p, [1] * 64, 64, w) == [64] + [0] * 63
    d.free()


# ---- 11. conversions -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["goldilocks", "big18", "koalabear", "f3", "all_ones"])
def test_conversions(L, name):
    p, c = MODULI[name], _ctx()
    vals = [0, 1, p - 1, p, p + 1, (1 << 64) - 1, 1 << 64, (1 << 256) - 1, p << 192, mc.MIMC_P, 1 << 255] + mc.inputs(3, 300, 1 << 255)
    k = len(vals)
    lm, wd, back = Dev(L, 32 * k).put(nc.limbs(vals)), Dev(L, 8 * k), Dev(L, 32 * k)
    assert L.sh_dev_mod64_from_limbs(c, p, lm.ptr, wd.ptr, k) == OK
    assert wd.words() == [v % p for v in vals]
    raw = nc.inputs(4, k, p)  # to_limbs reduces nothing: values at or above p stay
    wd.put(words(raw))
    assert L.sh_dev_mod64_to_limbs(c, wd.ptr, back.ptr, k) == OK
    assert back.get() == nc.limbs(raw)
    assert L.sh_dev_mod64_from_limbs(c, p, back.ptr, wd.ptr, k) == OK
    assert wd.words() == [v % p for v in raw]
    for d in (lm, wd, back):
        d.free()


# ---- 12. Python ----------------------------------------------------------------------------------------------------------------------
def _python_child():
    """starks_amd.fft.mod64_ntt / mod64_mul_polys in a process that holds no context"""
    from starks_amd import _lib, fft
    assert _lib._ctx is None
    p, n = GL, 1 << 10
    w = root_of("goldilocks", n)
    x = nc.inputs(14, n // 2 + 3, p)
    want = mc.transform(x, n, p, w)
    forms = [words(x), array.array("Q", x), list(x), bytearray(words(x))]
    try:
        import numpy
        forms.append(numpy.array(x, dtype=numpy.uint64))
    except ImportError:
        pass
    ok = []
    for data in forms:
        out = fft.mod64_ntt(p, data, n, w)
        ok.append(isinstance(out, memoryview) and out.format == "Q" and isinstance(out.obj, bytearray) and list(out) == want)
    assert _lib._ctx is not None
    back = fft.mod64_ntt(p, fft.mod64_ntt(p, x, n, w), n, w, inverse=True)
    ok.append(list(back) == [v % p for v in x] + [0] * (n - len(x)))
    two = fft.mod64_ntt(p, x[:200] + x[200:400], n, w, batch=2)
    ok.append(list(two) == mc.transform(x[:200], n, p, w) + mc.transform(x[200:400], n, p, w))
    a, b = nc.inputs(15, 300, p), nc.inputs(16, 700, p)
    prod = fft.mod64_mul_polys(p, a, array.array("Q", b), n, w)
    ok.append(prod.format == "Q" and list(prod) == mc.mul_polys(a, b, n, p, w))
    print(json.dumps(ok))


def test_python_entry_points():
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "python-child"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])
    assert len(got) >= 7 and all(got), got


def test_import_creates_no_context():
    code = ("import sys; sys.path.insert(0, %r); import starks_amd.fft as f; from starks_amd import _lib; "
            "assert _lib._ctx is None and _lib._lib is None; assert callable(f.mod64_ntt) and callable(f.mod64_mul_polys); "
            "assert 'numpy' not in sys.modules; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    {"plan-child": _plan_child, "python-child": _python_child}[sys.argv[1]]()
