"""The generic transform (sh_mod_ntt, sh_dev_mod_ntt, sh_mod_mul_polys: any odd modulus below 2^256, starks_amd/csrc/fpm.cuh and
modntt_items.cuh) on the MI355X: every size 2^0 .. 2^14 over nine prime moduli and a composite one against the exact oracle of
tests/modntt_cases.py and tests/golden/mod_ntt.json (the live reference's fft_1d / mul_polys); forced multi-pass plans in child
processes; the tuned MiMC transform as yardstick up to 2^24; BN254 and BLS12-381 at 2^20 and the 2^26 limit; two moduli on two
contexts at once; the plan cache; the Python call sites; the errors.  Every rejected call is refused on the host before any launch."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden
import modntt_cases as mc
from modntt_cases import MODULI, ints, root_of, wire

pytestmark = pytest.mark.gpu

OK, INVALID, ROOT_ORDER, UNSUPPORTED = 0, -1, -2, -6


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


def mod_ntt(L, p, vals, n, w, inv=False, batch=1, ctx=None):
    """sh_mod_ntt on `vals` = batch * n_in ints; returns batch * n ints"""
    out = ctypes.create_string_buffer(32 * n * batch)
    rc = L.sh_mod_ntt(ctx or _ctx(), b32(p), wire(vals), len(vals) // batch, out, n, batch, b32(w), 1 if inv else 0)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))
    return ints(out.raw)


class Dev(object):
    """a device buffer of `count` 32-byte values on a context"""

    def __init__(self, L, count, ctx=None):
        self.L, self.ctx, self.count = L, ctx or _ctx(), count
        self.ptr = ctypes.c_void_p()
        assert L.sh_dev_alloc(self.ctx, 32 * max(count, 1), ctypes.byref(self.ptr)) == OK

    def put(self, vals):  # plain values as 8 x u32 little-endian limbs = 32 little-endian bytes
        raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
        assert self.L.sh_dev_upload(self.ctx, raw, self.ptr, len(raw)) == OK
        return self

    def get(self, first=0, count=None):
        count = self.count - first if count is None else count
        out = ctypes.create_string_buffer(32 * count)
        assert self.L.sh_dev_download(self.ctx, ctypes.c_void_p(self.ptr.value + 32 * first), out, 32 * count) == OK
        return out.raw

    def ints(self, first=0, count=None):
        raw = self.get(first, count)
        return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]

    def free(self):
        assert self.L.sh_sync(self.ctx) == OK
        assert self.L.sh_dev_free(self.ctx, self.ptr) == OK


def dev_mod_ntt(L, p, src, dst, n, w, inv=False, batch=1, ctx=None):
    rc = L.sh_dev_mod_ntt(ctx or _ctx(), b32(p), src.ptr, dst.ptr, n, batch, b32(w), 1 if inv else 0)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))


# ---- 1. every size -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_every_size(L, name):
    """n = 2^0 .. 2^14 as far as the modulus has roots, forward and inverse, n_in = 1, n / 2 + 1 and n, inputs >= p included"""
    p = MODULI[name]
    top = min(14, mc.max_log(name))
    blob = mc.inputs(1234, 1 << top, p)
    for lg in range(top + 1):
        n, w = 1 << lg, root_of(name, 1 << lg)
        for inv in (False, True):
            s = pow(n, -1, p) if inv else 1
            assert mod_ntt(L, p, blob[:1], n, w, inv) == [blob[0] * s % p] * n, (name, lg, inv)  # one value: a constant vector
            for n_in in sorted({n // 2 + 1, n} - {1}):
                if n_in <= n:
                    assert mod_ntt(L, p, blob[:n_in], n, w, inv) == mc.transform(blob[:n_in], n, p, w, inv), (name, lg, n_in, inv)


def test_fixture(L):
    """the live reference's fft_1d and mul_polys outputs over BN254, BLS12-381 and 65537 at n = 8, 64, 1024"""
    for c in load_golden("mod_ntt.json")["cases"]:
        n, p, w, s = c["n"], c["p"], c["root"], c["seed"]
        full, short = mc.inputs(s, n, p), mc.inputs(s + 1, n // 2 + 1, p)
        assert mc.recorded(mod_ntt(L, p, full, n, w)) == c["forward"]
        assert mc.recorded(mod_ntt(L, p, full, n, w, True)) == c["inverse"]
        assert mc.recorded(mod_ntt(L, p, short, n, w)) == c["padded"]


# ---- 2. forced plans (child processes: the knob is read once per process) ---------------------------------------------------------
PLAN_MODULI = ("bn254", "mimc")


def _plan_inputs(name):
    return mc.inputs(4321, 5 << 12, MODULI[name])


def _digest(vals):
    return hashlib.sha256(wire(vals)).hexdigest()


def _plan_child():
    """every n = 2^1 .. 2^12: batch 1 forward and inverse through sh_mod_ntt, batch 5 forward IN PLACE through sh_dev_mod_ntt"""
    from starks_amd import _lib
    L = _lib.lib()
    out = []
    for name in PLAN_MODULI:
        p, blob = MODULI[name], _plan_inputs(name)
        buf = Dev(L, 5 << 12)
        for lg in range(1, 13):
            n, w = 1 << lg, root_of(name, 1 << lg)
            out.append(_digest(mod_ntt(L, p, blob[:n], n, w)))
            out.append(_digest(mod_ntt(L, p, blob[:n], n, w, True)))
            buf.put(blob[:5 * n])
            dev_mod_ntt(L, p, buf, buf, n, w, batch=5)
            out.append(_digest(buf.ints(0, 5 * n)))
        buf.free()
    print(json.dumps(out))


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


@pytest.mark.parametrize("tile_log", [2, 3, 5])
def test_forced_plans(tile_log):
    """STARKHIP_MODNTT_TILE_LOG = 2, 3, 5: up to six passes, uneven last passes, batch strides, at sizes the oracle covers"""
    env = dict(os.environ, STARKHIP_MODNTT_TILE_LOG=str(tile_log))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "plan-child"], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got, want = json.loads(out.stdout.strip().splitlines()[-1]), _plan_want()
    assert len(got) == len(want)
    assert [i for i, (g, w) in enumerate(zip(got, want)) if g != w] == []


# ---- 3. the tuned MiMC transform as yardstick at size ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lg,batch", [(17, 1), (20, 1), (24, 1), (20, 8)])
def test_equals_tuned_mimc_transform(L, lg, batch):
    """over the MiMC prime sh_dev_mod_ntt gives sh_dev_ntt's values byte for byte, forward and inverse, on seeded vectors (both
    downloaded through sh_dev_to_wire, which canonicalises the tuned path's lazily reduced limbs)"""
    n, p = 1 << lg, mc.MIMC_P
    w = root_of("mimc", n)
    total = n * batch
    x, a, b = Dev(L, total), Dev(L, total), Dev(L, total)
    assert L.sh_dev_fill_seeded(_ctx(), x.ptr, total, 99 + lg) == OK
    wa, wb = ctypes.create_string_buffer(32 * total), ctypes.create_string_buffer(32 * total)
    for inv in (0, 1):
        assert L.sh_dev_ntt(_ctx(), x.ptr, a.ptr, n, batch, b32(w), inv) == OK
        dev_mod_ntt(L, p, x, b, n, w, bool(inv), batch)
        assert L.sh_dev_to_wire(_ctx(), a.ptr, wa, total) == OK
        assert L.sh_dev_to_wire(_ctx(), b.ptr, wb, total) == OK
        assert wa.raw == wb.raw, (lg, batch, inv)
    for d in (x, a, b):
        d.free()


# ---- 4. at size in another field ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "bls12_381"])
def test_two_to_the_20(L, name):
    n, p = 1 << 20, MODULI[name]
    w = root_of(name, n)
    x, y, z = Dev(L, n), Dev(L, n), Dev(L, n)
    assert L.sh_dev_fill_seeded(_ctx(), x.ptr, n, 7) == OK
    dev_mod_ntt(L, p, x, y, n, w)
    dev_mod_ntt(L, p, y, z, n, w, True)
    xs = x.ints()
    assert any(v >= p for v in xs[:64])
    assert z.ints() == [v % p for v in xs]
    for k in (0, 1, 0x5a5a5, n - 1):  # four forward values against Horner at root^k
        pt, acc = pow(w, k, p), 0
        for c in reversed(xs):
            acc = (acc * pt + c) % p
        assert y.ints(k, 1) == [acc], k
    for d in (x, y, z):
        d.free()


def test_limit_2_to_the_26(L):
    """one 2^26-point round trip over BLS12-381 (the largest plan, 64-bit offsets): x -> forward -> inverse = x mod p, compared on
    sixteen 2^15-value windows spread over the vector, first and last included"""
    name, n = "bls12_381", 1 << 26
    p, w = MODULI[name], root_of(name, 1 << 26)
    x, y = Dev(L, n), Dev(L, n)
    assert L.sh_dev_fill_seeded(_ctx(), x.ptr, n, 26) == OK
    dev_mod_ntt(L, p, x, y, n, w)
    dev_mod_ntt(L, p, y, y, n, w, True)
    win = 1 << 15
    for i in range(16):
        first = (n - win) * i // 15
        assert y.ints(first, win) == [v % p for v in x.ints(first, win)], i
    for d in (x, y):
        d.free()
    assert L.sh_ctx_trim(_ctx()) == OK  # 2 GiB of tables and 2 GiB of work buffer go back


def test_size_limits(L):
    p, out = MODULI["bls12_381"], ctypes.create_string_buffer(64)
    c = _ctx()
    assert L.sh_mod_ntt(c, b32(p), b"\0" * 64, (1 << 26) + 1, out, 1 << 27, 1, b32(root_of("bls12_381", 1 << 27)), 0) == UNSUPPORTED
    assert L.sh_mod_ntt(c, b32(p), b"\0" * 64, 1, out, 1 << 20, 65, b32(root_of("bls12_381", 1 << 20)), 0) == UNSUPPORTED
    assert L.sh_dev_mod_ntt(c, b32(p), out, out, 1 << 27, 1, b32(root_of("bls12_381", 1 << 27)), 0) == UNSUPPORTED
    assert L.sh_dev_mod_ntt(c, b32(p), out, out, 1 << 13, 1 << 14, b32(root_of("bls12_381", 1 << 13)), 0) == UNSUPPORTED
    assert L.sh_mod_ntt(c, b32(p), b"\0" * 96, 3, out, 2, 1, b32(p - 1), 0) == INVALID  # more inputs than n
    assert L.sh_mod_ntt(c, b32(p), b"\0" * 64, 1, out, 3, 1, b32(p - 1), 0) == INVALID  # n is no power of two
    assert L.sh_sync(c) == OK


# ---- 5. sh_mod_mul_polys -------------------------------------------------------------------------------------------------------------
def mul_polys(L, p, a, b, n, w):
    out = ctypes.create_string_buffer(32 * n)
    rc = L.sh_mod_mul_polys(_ctx(), b32(p), wire(a), len(a), wire(b), len(b), out, n, b32(w))
    assert rc == OK, (rc, L.sh_last_error(_ctx()))
    return ints(out.raw)


def test_mul_polys(L):
    for c in load_golden("mod_ntt.json")["cases"]:
        n, p, s = c["n"], c["p"], c["seed"]
        assert mc.recorded(mul_polys(L, p, mc.inputs(s + 2, n // 2 + 1, p), mc.inputs(s + 3, n // 4 + 1, p), n, c["root"])) == c["mul_polys"]
    for name in ("bn254", "babybear", "f257", "composite"):
        p = MODULI[name]
        for lg in range(min(6, mc.max_log(name)) + 1):
            n = 1 << lg
            for n_a, n_b in {(n, n), (n // 2 + 1, 1), (0, n), (1, n // 2 + 1)}:
                a, b = mc.inputs(lg, n_a, p), mc.inputs(lg + 50, n_b, p)
                assert mul_polys(L, p, a, b, n, root_of(name, n)) == mc.cyclic_times_n([v % p for v in a], [v % p for v in b], n, p)


# ---- 6. two moduli at once -----------------------------------------------------------------------------------------------------------
def test_two_moduli_on_two_contexts(L):
    """BN254 on one context and BLS12-381 on another, 2^16-point transforms enqueued alternately with no synchronisation in between:
    each result equals its single-context bytes (a modulus kept in a device global fails here)"""
    from starks_amd import _lib
    n, rounds = 1 << 16, 6
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    names = ["bn254", "bls12_381"]
    src, dst, want = [], [], []
    for c, name in zip(ctxs, names):
        s = Dev(L, n, c)
        assert L.sh_dev_fill_seeded(c, s.ptr, n, 5) == OK
        d = [Dev(L, n, c) for _ in range(rounds)]
        dev_mod_ntt(L, MODULI[name], s, d[0], n, root_of(name, n), ctx=c)
        want.append(d[0].get())
        assert L.sh_sync(c) == OK
        src.append(s)
        dst.append(d)
    assert want[0] != want[1]
    for r in range(rounds):
        for k in (0, 1):
            dev_mod_ntt(L, MODULI[names[k]], src[k], dst[k][r], n, root_of(names[k], n), ctx=ctxs[k])
    for k in (0, 1):
        assert L.sh_sync(ctxs[k]) == OK
        for r in range(rounds):
            assert dst[k][r].get() == want[k], (k, r)
    for k in (0, 1):
        for d in [src[k]] + dst[k]:
            d.free()


# ---- 7. plan cache -------------------------------------------------------------------------------------------------------------------
def _stats(L, c):
    out = (ctypes.c_uint64 * 4)()
    assert L.sh_ctx_stats(c, out) == OK
    return list(out)


def test_plan_cache(L):
    """the tables are plans: counted, charged to the byte budget, evicted by the same LRU pass, dropped by sh_ctx_trim"""
    from starks_amd import _lib
    c = ctypes.c_void_p()
    assert L.sh_ctx_create(_lib.default_device(), ctypes.byref(c)) == OK
    try:
        n, table = 1 << 12, 32 << 11
        names = ["bn254", "goldilocks", "f65537"]
        x = mc.inputs(8, n, 1 << 255)
        want = {name: mc.transform(x, n, MODULI[name], root_of(name, n)) for name in names}
        for name in names:
            assert mod_ntt(L, MODULI[name], x, n, root_of(name, n), ctx=c) == want[name]
        assert _stats(L, c) == [3, 3 * table, 3, 0]
        assert mod_ntt(L, MODULI["bn254"], x, n, root_of("bn254", n), ctx=c) == want["bn254"]  # a hit: nothing is built
        assert _stats(L, c) == [3, 3 * table, 3, 0]
        assert L.sh_ctx_set_plan_budget(c, table - 1) == OK  # below one table: everything goes
        assert _stats(L, c) == [0, 0, 3, 3]
        assert mod_ntt(L, MODULI["goldilocks"], x, n, root_of("goldilocks", n), ctx=c) == want["goldilocks"]
        assert _stats(L, c) == [1, table, 4, 3]
        assert mod_ntt(L, MODULI["f65537"], x, n, root_of("f65537", n), ctx=c) == want["f65537"]  # the entry evicts goldilocks' table
        assert _stats(L, c) == [1, table, 5, 4]
        assert L.sh_ctx_trim(c) == OK
        assert _stats(L, c)[:2] == [0, 0]
        for name in names:
            assert mod_ntt(L, MODULI[name], x, n, root_of(name, n), ctx=c) == want[name]
    finally:
        L.sh_ctx_destroy(c)


def test_plan_cache_holds_both_kinds_of_plan(L):
    """a MiMC transform's plan and a generic-modulus table in one context share one cache: one count, one byte total, one LRU order.
    The MiMC plan's size is whatever the first statistics reading says; the 2^12-point table is 2^11 powers of 32 bytes."""
    from oracle import pyoracle
    from starks_amd import _lib
    c = ctypes.c_void_p()
    assert L.sh_ctx_create(_lib.default_device(), ctypes.byref(c)) == OK
    try:
        n, table = 1 << 12, 32 << 11
        P, p = mc.MIMC_P, MODULI["bn254"]
        wm, wb = root_of("mimc", n), root_of("bn254", n)
        xm, xb = [v % P for v in mc.inputs(21, n, P)], mc.inputs(22, n, p)
        want_m, want_b = pyoracle.fft_1d(xm, P, wm), mc.transform(xb, n, p, wb)

        def mimc_ntt():
            out = ctypes.create_string_buffer(32 * n)
            assert L.sh_ntt(c, wire(xm), n, out, n, b32(wm), 0) == OK, L.sh_last_error(c)
            return ints(out.raw)

        assert _stats(L, c) == [0, 0, 0, 0]
        assert mimc_ntt() == want_m
        first = _stats(L, c)
        mimc = first[1]
        assert first == [1, mimc, 1, 0] and mimc > 0 and mimc != table
        assert mod_ntt(L, p, xb, n, wb, ctx=c) == want_b
        assert _stats(L, c) == [2, mimc + table, 2, 0]
        assert mimc_ntt() == want_m  # a hit: nothing is built, and the table is now the least recently used of the two
        assert _stats(L, c) == [2, mimc + table, 2, 0]
        assert L.sh_ctx_set_plan_budget(c, mimc + table - 1) == OK  # one byte short of both: this entry evicts the table alone
        assert _stats(L, c) == [1, mimc, 2, 1]
        assert mimc_ntt() == want_m  # still a hit
        assert _stats(L, c) == [1, mimc, 2, 1]
        assert mod_ntt(L, p, xb, n, wb, ctx=c) == want_b  # built again, beside the MiMC plan
        assert _stats(L, c) == [2, mimc + table, 3, 1]
    finally:
        L.sh_ctx_destroy(c)


# ---- 8. Python call sites ------------------------------------------------------------------------------------------------------------
def test_python_call_sites(L):
    from starks_amd import IntegersModP, _lib, fft
    from starks_amd.merkle_tree import merkelize
    from starks_amd.wireseq import WireList
    _lib.ctx()
    p, n = mc.BN254, 1 << 10
    F, w = IntegersModP(p), root_of("bn254", 1 << 10)
    x = mc.inputs(11, n // 2 + 3, p)
    ev = fft.fft_1d(F, [F(v) for v in x], p, F(w))
    assert isinstance(ev, WireList) and ev.field is F and isinstance(ev[3], F)
    assert [int(v) for v in ev] == mc.transform(x, n, p, w)
    back = fft.fft_1d(F, ev, p, F(w), inv=True)
    assert isinstance(back, WireList) and [int(v) for v in back] == [v % p for v in x] + [0] * (n - len(x))
    nb = fft.NonBinaryFFT(F, F(w))
    ev2 = nb.fft([F(v) for v in x])
    assert isinstance(ev2, WireList) and ev2 == ev
    poly = nb.inv_fft(ev2)
    assert [int(v) for v in poly.coefficients] == [v % p for v in x]
    a, b = mc.inputs(12, 300, p), mc.inputs(13, 700, p)
    prod = fft.mul_polys([F(v) for v in a], [F(v) for v in b], F(w))
    assert isinstance(prod, WireList) and prod.field is F and [int(v) for v in prod] == mc.mul_polys(a, b, n, p, w)
    # the commitment of a trace over another field: the tree of the values' bytes
    tree = merkelize(ev)
    vals = [b32(v) for v in mc.transform(x, n, p, w)]
    nodes = [b""] * n + [vals[i + j * (n // 4)] for i in range(n // 4) for j in range(4)]
    for i in range(n - 1, 0, -1):
        nodes[i] = hashlib.blake2s(nodes[2 * i] + nodes[2 * i + 1]).digest()
    assert [bytes(v) for v in tree[1:]] == nodes[1:]


def _no_context_child():
    """order 2^13 over BN254 in a process that holds no context: the device is used (before this path existed the call raised)"""
    from starks_amd import IntegersModP, _lib, fft
    p, n = mc.BN254, 1 << 13
    F, w = IntegersModP(p), root_of("bn254", 1 << 13)
    x = mc.inputs(14, n, p)
    assert _lib._ctx is None
    out = fft.fft_1d(F, x, p, F(w))
    assert _lib._ctx is not None
    print(json.dumps([_digest([int(v) for v in out]), _digest(mc.transform(x, n, p, w))]))


def test_order_above_the_host_limit_without_a_context():
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "no-context-child"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got, want = json.loads(out.stdout.strip().splitlines()[-1])
    assert got == want


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(L):
    c, p = _ctx(), mc.BN254
    out, one = ctypes.create_string_buffer(32 * 64), b"\0" * 31 + b"\1"
    w = root_of("bn254", 64)
    before = _stats(L, c)

    def both(mod, root, n):
        rc = L.sh_mod_ntt(c, b32(mod), one * 64, 64, out, n, 1, b32(root), 0)
        msg = L.sh_last_error(c).decode()
        assert L.sh_dev_mod_ntt(c, b32(mod), out, out, n, 1, b32(root), 0) == rc
        assert L.sh_mod_mul_polys(c, b32(mod), one, 1, one, 1, out, n, b32(root)) == rc
        return rc, msg

    for bad in (p - 1, 0, 1, 2, 1 << 255):
        rc, msg = both(bad, 1, 1)
        assert rc == INVALID and "odd" in msg, (bad, msg)
    rc, msg = both(p, root_of("bn254", 32), 64)
    assert rc == ROOT_ORDER and "order" in msg
    rc, msg = both(p, root_of("bn254", 128), 64)
    assert rc == ROOT_ORDER and "order" in msg
    rc, msg = both(p, p + w, 64)
    assert rc == ROOT_ORDER and "below" in msg
    rc, msg = both(p, 2, 1)
    assert rc == ROOT_ORDER
    assert L.sh_mod_ntt(c, b32(p), one * 64, 64, out, 64, 0, b32(w), 0) == INVALID  # batch 0
    assert L.sh_mod_ntt(c, None, one * 64, 64, out, 64, 1, b32(w), 0) == INVALID
    assert _stats(L, c) == before  # no table was built, nothing was launched
    assert L.sh_sync(c) == OK
    assert mod_ntt(L, p, [1] * 64, 64, w) == [64] + [0] * 63


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    {"plan-child": _plan_child, "no-context-child": _no_context_child}[sys.argv[1]]()
