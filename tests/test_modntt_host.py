"""The generic transform's CPU half: starks_amd/csrc/fpm.cuh (Montgomery arithmetic with a run-time modulus) against Python ints for
ten moduli, and the pass bodies of starks_amd/csrc/modntt_items.cuh walked on the host by tests/native/modntt_host.cpp (hipcc) over
the grid the library launches -- every size 2^0 .. 2^12, default and forced tile logs, short inputs, batches -- against the exact
oracle of tests/modntt_cases.py and tests/golden/mod_ntt.json (the live reference's fft_1d and mul_polys).  The root check, the
routing rule of starks_amd/fft.py and its host path for other moduli.  CPU only."""
import os
import random
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden
import modntt_cases as mc
from modntt_cases import MODULI, ints, root_of, wire

G = load_golden("mod_ntt.json")
R = 1 << 256


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mn") / "modntt_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "modntt_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, args, **files):
    for name, data in files.items():
        (d / name).write_bytes(data)
    return subprocess.run([driver, args[0], str(d)] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=600)


def _arith(driver, d, p, op, a, b=None):
    out = _call(driver, d, ["arith", op], mod=wire([p]), a=wire(a), b=wire(b if b is not None else [0] * len(a)))
    assert out.returncode == 0, out.stderr
    return ints((d / "out").read_bytes())


# ---- (a) arithmetic ------------------------------------------------------------------------------------------------------------------
def _edges(p):
    return sorted({0, 1, p - 1, p, p + 1, R - 1, 1 << 255, int("ffffffff" * 8, 16), int("ffffffff00000000" * 4, 16), (p + 1) // 2, 2})


@pytest.mark.parametrize("name", sorted(MODULI))
def test_constants(driver, tmp_path, name):
    p = MODULI[name]
    out = _call(driver, tmp_path, ["consts"], mod=wire([p]))
    assert out.returncode == 0
    got = ints((tmp_path / "out").read_bytes())
    assert got == [p, R * R % p, R % p, (-pow(p, -1, 1 << 32)) % (1 << 32)]


@pytest.mark.parametrize("name", sorted(MODULI))
def test_arithmetic(driver, tmp_path, name):
    """every edge operand against every edge operand and 1000 seeded pairs.  fpm_mul takes any 256-bit first operand and a canonical
    second one and returns the exact residue a b R^-1 mod p; fpm_add / fpm_sub take canonical operands; the conversions any value."""
    p = MODULI[name]
    rnd = random.Random(p % 1000003)
    E = _edges(p)
    a = [x for x in E for _ in E] + [rnd.randrange(R) for _ in range(1000)]
    b = [y for _ in E for y in E] + [rnd.randrange(R) for _ in range(1000)]
    rinv = pow(R, -1, p)
    bc = [y % p for y in b]
    assert _arith(driver, tmp_path, p, "mul", a, bc) == [x * y * rinv % p for x, y in zip(a, bc)]
    ac = [x % p for x in a]
    assert _arith(driver, tmp_path, p, "add", ac, bc) == [(x + y) % p for x, y in zip(ac, bc)]
    assert _arith(driver, tmp_path, p, "sub", ac, bc) == [(x - y) % p for x, y in zip(ac, bc)]
    assert _arith(driver, tmp_path, p, "to_mont", a) == [x * R % p for x in a]
    assert _arith(driver, tmp_path, p, "from_mont", ac) == [x * rinv % p for x in ac]
    assert _arith(driver, tmp_path, p, "canon", a) == [x % p for x in a]


def test_ninth_word(driver, tmp_path):
    """moduli above 2^255 (the MiMC prime, secp256k1's order, 2^256 - 189): operands that drive the running sum past 2^256"""
    for p in (mc.MIMC_P, mc.SECP256K1_N, R - 189):
        a = [R - 1, p - 1, R - 1, p + 1 if p + 1 < R else p]
        b = [p - 1, p - 1, p - 2, p - 1]
        rinv = pow(R, -1, p)
        assert _arith(driver, tmp_path, p, "mul", a, b) == [x * y * rinv % p for x, y in zip(a, b)]


# ---- (b) transforms ------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(name, vals, n, inv):
    key = (name, n, inv, len(vals), vals[0] if vals else None, vals[-1] if vals else None)
    if key not in _ORACLE:
        _ORACLE[key] = mc.transform(vals, n, MODULI[name], root_of(name, n), inv)
    return _ORACLE[key]


def _walk(driver, d, name, cases, blob):
    """cases: (log_n, n_in, batch, inverse, tile_log, offset) -> the results, one list of ints per case, and the pass counts"""
    lines = ["%d %d %d %d %d %d %s" % (c + (wire([root_of(name, 1 << c[0])]).hex(),)) for c in cases]
    out = _call(driver, d, ["ntt"], mod=wire([MODULI[name]]), cases=("\n".join(lines) + "\n").encode(), **{"in": wire(blob)})
    assert out.returncode == 0, (out.returncode, out.stderr)
    got, res, k = ints((d / "out").read_bytes()), [], 0
    for c in cases:
        cnt = c[2] << c[0]
        res.append(got[k:k + cnt])
        k += cnt
    assert k == len(got)
    return res, [int(v) for v in out.stdout.split()]


@pytest.mark.parametrize("tile_log", [10, 2, 3, 5])
@pytest.mark.parametrize("name", ["bn254", "mimc", "f65537", "composite"])
def test_walk_every_size(driver, tmp_path, name, tile_log):
    """forward and inverse, n = 2^0 .. 2^12 (4369: up to 16), n_in = 0, 1, n - 1, n, batch 1 and 3; inputs include values >= p"""
    p, top = MODULI[name], min(12, mc.max_log(name))
    blob = mc.inputs(77, 3 << top, p)
    cases = [(lg, n_in, batch, inv, tile_log, 0) for lg in range(top + 1) for n_in in sorted({0, 1, (1 << lg) - 1, 1 << lg})
             for batch in (1, 3) for inv in (0, 1)]
    res, passes = _walk(driver, tmp_path, name, cases, blob)
    for (lg, n_in, batch, inv, _, _), got, m in zip(cases, res, passes):
        n = 1 << lg
        assert m == max(1, -(-lg // tile_log))
        want = [v for b in range(batch) for v in (_oracle(name, blob[b * n_in:(b + 1) * n_in], n, bool(inv)) if n_in else [0] * n)]
        assert got == want, (name, lg, n_in, batch, inv, tile_log)
    if tile_log == 2:
        assert max(passes) == (6 if top == 12 else 2)


@pytest.mark.parametrize("name", ["bn254", "mimc", "f65537", "composite"])
def test_walk_round_trip(driver, tmp_path, name):
    """inverse(forward(x)) = x mod p at every size, the two directions under different plans"""
    p, top = MODULI[name], min(12, mc.max_log(name))
    blob = mc.inputs(91, 1 << top, p)
    fwd = [(lg, 1 << lg, 1, 0, 3, 0) for lg in range(top + 1)]
    res, _ = _walk(driver, tmp_path, name, fwd, blob)
    flat = [v for r in res for v in r]
    back = [(lg, 1 << lg, 1, 1, 10, (1 << lg) - 1) for lg in range(top + 1)]
    res2, _ = _walk(driver, tmp_path, name, back, flat)
    for lg, got in enumerate(res2):
        assert got == [v % p for v in blob[:1 << lg]]


def test_oracle_is_the_definition():
    """the recursive oracle against sum_j x_j w^(jk) with pow, n <= 64, every modulus"""
    for name in sorted(MODULI):
        p = MODULI[name]
        for lg in range(min(6, mc.max_log(name)) + 1):
            n = 1 << lg
            x = mc.inputs(lg, n // 2 + 1, p)
            for inv in (False, True):
                assert mc.transform(x, n, p, root_of(name, n), inv) == mc.dft_pow(x, n, p, root_of(name, n), inv)


def test_roots_have_their_order():
    for name in sorted(MODULI):
        p = MODULI[name]
        for lg in range(mc.max_log(name) + 1):
            w = root_of(name, 1 << lg)
            assert pow(w, 1 << lg, p) == 1 and (lg == 0 or pow(w, 1 << (lg - 1), p) == p - 1)
    assert pow(129, 8, 4369) == 4368 and pow(253, 4, 4369) == 4368 and 17 * 257 == 4369


# ---- (c) root check ------------------------------------------------------------------------------------------------------------------
def _check(driver, d, p, root, n):
    return _call(driver, d, ["check", n], mod=wire([p]), root=wire([root])).returncode


def test_root_check(driver, tmp_path):
    for name in ("bn254", "mimc", "f65537", "goldilocks"):
        p = MODULI[name]
        for n in (1, 2, 4, 64, 1024):
            assert _check(driver, tmp_path, p, root_of(name, n), n) == 0
            assert _check(driver, tmp_path, p, root_of(name, 2 * n), n) == 3   # order 2n
            if n >= 2:
                assert _check(driver, tmp_path, p, root_of(name, n // 2), n) == 3  # order n / 2
            if p + root_of(name, n) < R:
                assert _check(driver, tmp_path, p, p + root_of(name, n), n) == 3  # the right residue, but not below p
        assert _check(driver, tmp_path, p, p, 1) == 3
    assert _check(driver, tmp_path, 4369, 129, 16) == 0 and _check(driver, tmp_path, 4369, 253, 8) == 0
    assert _check(driver, tmp_path, 4369, 129, 8) == 3
    for bad in (0, 1, 2, BN_EVEN, R - 2):
        assert _check(driver, tmp_path, bad, 1, 1) == 2
    assert _check(driver, tmp_path, 3, 2, 2) == 0 and _check(driver, tmp_path, 3, 1, 1) == 0


BN_EVEN = mc.BN254 - 1


# ---- (e) fixture ---------------------------------------------------------------------------------------------------------------------
def _fixture_inputs(c):
    n, p, s = c["n"], c["p"], c["seed"]
    return mc.inputs(s, n, p), mc.inputs(s + 1, n // 2 + 1, p), mc.inputs(s + 2, n // 2 + 1, p), mc.inputs(s + 3, n // 4 + 1, p)


def test_fixture_shape():
    assert sorted({c["modulus"] for c in G["cases"]}) == ["bls12_381", "bn254", "f65537"]
    assert sorted({c["n"] for c in G["cases"]}) == [8, 64, 1024] and len(G["cases"]) == 9
    for c in G["cases"]:
        assert c["p"] == MODULI[c["modulus"]] and c["root"] == root_of(c["modulus"], c["n"])
        assert all(c[k]["n"] == c["n"] and ("values" in c[k]) == (c["n"] <= 8) for k in ("forward", "inverse", "padded", "mul_polys"))


def test_fixture_oracle():
    """the oracle helper restates the live reference's fft_1d and mul_polys"""
    for c in G["cases"]:
        n, p, w = c["n"], c["p"], c["root"]
        full, short, a, b = _fixture_inputs(c)
        assert mc.recorded(mc.transform(full, n, p, w)) == c["forward"]
        assert mc.recorded(mc.transform(full, n, p, w, True)) == c["inverse"]
        assert mc.recorded(mc.transform(short, n, p, w)) == c["padded"]
        assert mc.recorded(mc.mul_polys(a, b, n, p, w)) == c["mul_polys"]
        if n <= 64:
            assert mc.recorded(mc.cyclic_times_n([v % p for v in a], [v % p for v in b], n, p)) == c["mul_polys"]


@pytest.mark.parametrize("tile_log", [10, 3])
def test_fixture_host_walk(driver, tmp_path, tile_log):
    for c in G["cases"]:
        name, n, lg = c["modulus"], c["n"], c["n"].bit_length() - 1
        full, short, a, b = _fixture_inputs(c)
        cases = [(lg, n, 1, 0, tile_log, 0), (lg, n, 1, 1, tile_log, 0), (lg, len(short), 1, 0, tile_log, n)]
        res, _ = _walk(driver, tmp_path, name, cases, full + short)
        assert [mc.recorded(r) for r in res] == [c[k] for k in ("forward", "inverse", "padded")], (name, n)
        out = _call(driver, tmp_path, ["mul", lg, len(a), len(b), tile_log], mod=wire([c["p"]]), root=wire([c["root"]]), a=wire(a), b=wire(b))
        assert out.returncode == 0
        assert mc.recorded(ints((tmp_path / "out").read_bytes())) == c["mul_polys"], (name, n)


# ---- (d) routing ---------------------------------------------------------------------------------------------------------------------
def test_host_path_without_a_context(monkeypatch):
    """no device context: fft_1d over BN254 at order 64 and mul_polys over 65537 at order 256 run _host_dft and equal the oracle"""
    from starks_amd import IntegersModP, _lib, fft
    monkeypatch.setattr(_lib, "_ctx", None)  # a process that holds none (other tests of a GPU run may have made one)
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("the host path must not ask for a context"))
    p = mc.BN254
    F = IntegersModP(p)
    w = root_of("bn254", 64)
    x = mc.inputs(3, 40, p)
    assert not fft._mod_on_device(p, w)
    assert [int(v) for v in fft.fft_1d(F, [F(v) for v in x], p, F(w))] == mc.transform(x, 64, p, w)
    assert [int(v) for v in fft.fft_1d(F, [F(v) for v in x], p, F(w), inv=True)] == mc.transform(x, 64, p, w, True)
    q = 65537
    Fq = IntegersModP(q)
    wq = root_of("f65537", 256)
    a, b = mc.inputs(4, 100, q), mc.inputs(5, 157, q)
    assert [int(v) for v in fft.mul_polys([Fq(v) for v in a], [Fq(v) for v in b], Fq(wq))] == mc.mul_polys(a, b, 256, q, wq)
    assert _lib._ctx is None


def test_routing_rule(monkeypatch):
    from starks_amd import _lib, fft
    bn, held = mc.BN254, object()
    for ctx, want_small in ((None, False), (held, True)):
        monkeypatch.setattr(_lib, "_ctx", ctx)
        assert fft._mod_on_device(bn, root_of("bn254", 64)) is want_small
        assert fft._mod_on_device(bn, root_of("bn254", 1 << 12)) is want_small      # _HOST_MAX_ORDER itself: the host still takes it
        assert fft._mod_on_device(bn, root_of("bn254", 1 << 13)) is True            # above it: today's code raises
        assert fft._mod_on_device(mc.GOLDILOCKS, root_of("goldilocks", 1 << 20)) is True
        assert fft._mod_on_device(bn, root_of("bn254", 32)) is False                # orders below 64 stay on the host
        assert fft._mod_on_device(31, 15) is False                                  # the reference's Z/31, order 6
        assert fft._mod_on_device(31, 2) is False                                   # order 5
        assert fft._mod_on_device(1 << 64, 3) is False                              # even
        assert fft._mod_on_device((1 << 256) + 297, 3) is False                     # 257 bits
        assert fft._mod_on_device(mc.MIMC_P, root_of("mimc", 1 << 10)) is False     # the MiMC prime keeps its own path
        assert fft._on_device(mc.MIMC_P, root_of("mimc", 1 << 10)) is True
        assert fft._mod_on_device(4369, 129) is False                               # order 16


def test_import_creates_no_context():
    code = ("import sys; sys.path.insert(0, %r); import starks_amd.fft as f; from starks_amd import _lib; "
            "assert _lib._ctx is None and _lib._lib is None; assert callable(f.mod_ntt_bytes); print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
