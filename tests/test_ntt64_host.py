"""The packed-word transform's CPU half: starks_amd/csrc/fp64m.cuh (Montgomery arithmetic on one 64-bit word with a run-time modulus)
against Python ints for eleven moduli, and the pass bodies and index maps of starks_amd/csrc/ntt64_items.cuh walked on the host by
tests/native/ntt64_host.cpp (hipcc) over the grid the library launches -- every size 2^0 .. 2^12, default and forced tile logs, short
inputs, batches -- against the exact oracle of tests/modntt_cases.py and tests/golden/mod64_ntt.json (the live reference's fft_1d and
mul_polys).  The root check; the run length of every global access and the bank-conflict degree of every LDS access under the default
plan; the same driver once more under AddressSanitizer and UBSan.  CPU only."""
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_golden
import modntt_cases as mc
import ntt64_cases as nc
from ntt64_cases import MODULI, ints, root_of, words

G = load_golden("mod64_ntt.json")
R = 1 << 64
HIPCC = ["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
         os.path.join(ROOT, "tests", "native", "ntt64_host.cpp")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("n64") / "ntt64_host")
    subprocess.check_call(HIPCC + ["-o", exe], stderr=subprocess.DEVNULL)
    return exe


@pytest.fixture(scope="module")
def san_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("n64san") / "ntt64_host_san")
    subprocess.check_call(HIPCC + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe],
                          stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, p, args, **files):
    for name, data in files.items():
        (d / name).write_bytes(data)
    return subprocess.run([driver, args[0], str(d), str(p)] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=900)


def _arith(driver, d, p, op, a, b=None):
    out = _call(driver, d, p, ["arith", op], a=words(a), b=words(b if b is not None else [0] * len(a)))
    assert out.returncode == 0, out.stderr
    return ints((d / "out").read_bytes())


# ---- (a) arithmetic ------------------------------------------------------------------------------------------------------------------
def _edges(p):
    return sorted({v for v in (0, 1, 2, p - 1, p, p + 1, (p + 1) // 2, 1 << 63, R - 1, 0xffffffff00000000, 0x00000000ffffffff) if v < R})


@pytest.mark.parametrize("name", sorted(MODULI))
def test_constants(driver, tmp_path, name):
    p = MODULI[name]
    out = _call(driver, tmp_path, p, ["consts"])
    assert out.returncode == 0
    assert ints((tmp_path / "out").read_bytes()) == [p, (-pow(p, -1, R)) % R, R * R % p, R % p]


@pytest.mark.parametrize("name", sorted(MODULI))
def test_arithmetic(driver, tmp_path, name):
    """every edge operand against every edge operand and 1000 seeded pairs.  f64_mul takes any 64-bit first operand and a canonical
    second one and returns the exact residue a b R^-1 mod p; f64_add / f64_sub take canonical operands; the conversions any value."""
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


@pytest.mark.parametrize("name", sorted(MODULI))
def test_from_limbs(driver, tmp_path, name):
    """the exact residue of 256-bit values: the edges 2^256 - 1, p 2^192, the MiMC prime, and seeded values"""
    p = MODULI[name]
    rnd = random.Random(p % 999983)
    vals = [0, 1, p - 1, p, p + 1, R - 1, R, (1 << 256) - 1, p << 192, mc.MIMC_P, (1 << 255), (p << 192) - 1]
    vals += [rnd.randrange(1 << 256) for _ in range(200)]
    out = _call(driver, tmp_path, p, ["from_limbs"], a=nc.limbs(vals))
    assert out.returncode == 0
    assert ints((tmp_path / "out").read_bytes()) == [v % p for v in vals]


# ---- (b) transforms ------------------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(name, vals, n, inv):
    key = (name, n, inv, len(vals), vals[0] if vals else None, vals[-1] if vals else None)
    if key not in _ORACLE:
        _ORACLE[key] = mc.transform(vals, n, MODULI[name], root_of(name, n), inv)
    return _ORACLE[key]


def _walk(driver, d, name, cases, blob):
    """cases: (log_n, n_in, batch, inverse, tile_log, offset) -> the results, one list of ints per case, and the pass counts"""
    lines = ["%d %d %d %d %d %d %d" % (c + (root_of(name, 1 << c[0]),)) for c in cases]
    out = _call(driver, d, MODULI[name], ["ntt"], cases=("\n".join(lines) + "\n").encode(), **{"in": words(blob)})
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got, res, k = ints((d / "out").read_bytes()), [], 0
    for c in cases:
        cnt = c[2] << c[0]
        res.append(got[k:k + cnt])
        k += cnt
    assert k == len(got)
    return res, [int(v) for v in out.stdout.split()]


def passes_of(lg, tile_log):
    """the documented plan rule (include/starkhip.h): the largest radix log is t - min(4, t // 2), m = ceil(lg / that)"""
    return max(1, -(-lg // (tile_log - min(4, tile_log // 2))))


def _grid(top, tile_log):
    return [(lg, n_in, batch, inv, tile_log, 0) for lg in range(top + 1) for n_in in sorted({0, 1, (1 << lg) - 1, 1 << lg})
            for batch in (1, 3) for inv in (0, 1)]


def _check_grid(name, cases, res, passes, blob):
    for (lg, n_in, batch, inv, tile_log, _), got, m in zip(cases, res, passes):
        n = 1 << lg
        assert m == passes_of(lg, tile_log), (lg, tile_log, m)
        want = [v for b in range(batch) for v in (_oracle(name, blob[b * n_in:(b + 1) * n_in], n, bool(inv)) if n_in else [0] * n)]
        assert got == want, (name, lg, n_in, batch, inv, tile_log)


@pytest.mark.parametrize("tile_log", [12, 13, 2, 3, 5, 8])
@pytest.mark.parametrize("name", ["goldilocks", "big18", "f65537", "composite"])
def test_walk_every_size(driver, tmp_path, name, tile_log):
    """forward and inverse, n = 2^0 .. 2^12 (4369: up to 16), n_in = 0, 1, n - 1, n, batch 1 and 3; inputs include values >= p"""
    p, top = MODULI[name], min(12, nc.max_log(name))
    blob = nc.inputs(77, 3 << top, p)
    cases = _grid(top, tile_log)
    res, passes = _walk(driver, tmp_path, name, cases, blob)
    _check_grid(name, cases, res, passes, blob)
    if tile_log == 2:
        assert max(passes) == (12 if top == 12 else 4)
    if tile_log == 12 and top == 12:
        assert passes[-1] == 2 and passes_of(16, 12) == 2 and passes_of(24, 12) == 3 and passes_of(28, 12) == 4


def test_walk_small_moduli(driver, tmp_path):
    """the moduli with few roots -- 3, 17, 257, 2^64 - 59, 2^64 - 1 -- and the 31-bit fields, default tile log and tile log 3"""
    for name in ("f3", "f17", "f257", "p64_59", "all_ones", "babybear", "koalabear"):
        p, top = MODULI[name], min(9, nc.max_log(name))
        blob = nc.inputs(78, 3 << top, p)
        for tile_log in (12, 3):
            cases = _grid(top, tile_log)
            res, passes = _walk(driver, tmp_path, name, cases, blob)
            _check_grid(name, cases, res, passes, blob)


@pytest.mark.parametrize("name", ["goldilocks", "big18", "f65537", "composite"])
def test_walk_round_trip(driver, tmp_path, name):
    """inverse(forward(x)) = x mod p at every size, the two directions under different plans"""
    p, top = MODULI[name], min(12, nc.max_log(name))
    blob = nc.inputs(91, 1 << top, p)
    fwd = [(lg, 1 << lg, 1, 0, 3, 0) for lg in range(top + 1)]
    res, _ = _walk(driver, tmp_path, name, fwd, blob)
    flat = [v for r in res for v in r]
    back = [(lg, 1 << lg, 1, 1, 12, (1 << lg) - 1) for lg in range(top + 1)]
    res2, _ = _walk(driver, tmp_path, name, back, flat)
    for lg, got in enumerate(res2):
        assert got == [v % p for v in blob[:1 << lg]]


def test_roots_have_their_order():
    for name in sorted(MODULI):
        p = MODULI[name]
        assert p % 2 == 1 and 3 <= p < R
        for lg in range(nc.max_log(name) + 1):
            w = root_of(name, 1 << lg)
            assert w < p and pow(w, 1 << lg, p) == 1 and (lg == 0 or pow(w, 1 << (lg - 1), p) == p - 1)
    for name, (p, v, base) in nc.PRIMES.items():
        assert (p - 1) % (1 << v) == 0 and ((p - 1) >> v) % 2 == 1, name
        assert all(pow(x, (p - 1) // 2, p) == 1 for x in range(1, base)) and pow(base, (p - 1) // 2, p) == p - 1, name  # the smallest
    assert nc.PRIMES["koalabear"] == (2**31 - 2**24 + 1, 24, 3)
    assert nc.BIG18 == 2**64 - 1835007 and nc.PRIMES["big18"][1:] == (18, 7)


def test_inputs_reach_above_the_modulus():
    for name in sorted(MODULI):
        p = MODULI[name]
        x = nc.inputs(5, 50, p)
        assert all(0 <= v < R for v in x) and any(v >= p for v in x)


# ---- (c) root and modulus check ------------------------------------------------------------------------------------------------------
def _check(driver, d, p, root, n):
    return _call(driver, d, p, ["check", n, root]).returncode


def test_root_check(driver, tmp_path):
    for name in ("goldilocks", "big18", "f65537", "babybear"):
        p = MODULI[name]
        for n in (1, 2, 4, 64, 1024):
            assert _check(driver, tmp_path, p, root_of(name, n), n) == 0
            assert _check(driver, tmp_path, p, root_of(name, 2 * n), n) == 3   # order 2n
            if n >= 2:
                assert _check(driver, tmp_path, p, root_of(name, n // 2), n) == 3  # order n / 2
            if p + root_of(name, n) < R:
                assert _check(driver, tmp_path, p, p + root_of(name, n), n) == 3  # the right residue, but not below p
        assert _check(driver, tmp_path, p, p, 1) == 3
        assert _check(driver, tmp_path, p, 2, 1) == 3  # n = 1: the root must be 1
    assert _check(driver, tmp_path, 4369, 129, 16) == 0 and _check(driver, tmp_path, 4369, 253, 8) == 0
    assert _check(driver, tmp_path, 4369, 129, 8) == 3
    for bad in (0, 1, 2, nc.GOLDILOCKS - 1, R - 2):
        assert _check(driver, tmp_path, bad, 1, 1) == 2
    assert _check(driver, tmp_path, 3, 2, 2) == 0 and _check(driver, tmp_path, 3, 1, 1) == 0
    assert _check(driver, tmp_path, R - 1, R - 2, 2) == 0 and _check(driver, tmp_path, R - 1, R - 1, 2) == 3


# ---- (d) fixture ---------------------------------------------------------------------------------------------------------------------
def _fixture_inputs(c):
    n, p, s = c["n"], c["p"], c["seed"]
    return nc.inputs(s, n, p), nc.inputs(s + 1, n // 2 + 1, p), nc.inputs(s + 2, n // 2 + 1, p), nc.inputs(s + 3, n // 4 + 1, p)


def test_fixture_shape():
    assert sorted({c["modulus"] for c in G["cases"]}) == ["babybear", "f65537", "goldilocks"]
    assert sorted({c["n"] for c in G["cases"]}) == [8, 64, 1024] and len(G["cases"]) == 9
    for c in G["cases"]:
        assert c["p"] == MODULI[c["modulus"]] and c["root"] == root_of(c["modulus"], c["n"])
        assert all(c[k]["n"] == c["n"] and ("values" in c[k]) == (c["n"] <= 8) for k in ("forward", "inverse", "padded", "mul_polys"))


def test_fixture_oracle():
    """the oracle helper restates the live reference's fft_1d and mul_polys over these moduli"""
    for c in G["cases"]:
        n, p, w = c["n"], c["p"], c["root"]
        full, short, a, b = _fixture_inputs(c)
        assert mc.recorded(mc.transform(full, n, p, w)) == c["forward"]
        assert mc.recorded(mc.transform(full, n, p, w, True)) == c["inverse"]
        assert mc.recorded(mc.transform(short, n, p, w)) == c["padded"]
        assert mc.recorded(mc.mul_polys(a, b, n, p, w)) == c["mul_polys"]
        if n <= 64:
            assert mc.recorded(mc.cyclic_times_n([v % p for v in a], [v % p for v in b], n, p)) == c["mul_polys"]


@pytest.mark.parametrize("tile_log", [12, 3])
def test_fixture_host_walk(driver, tmp_path, tile_log):
    for c in G["cases"]:
        name, n, lg = c["modulus"], c["n"], c["n"].bit_length() - 1
        full, short, a, b = _fixture_inputs(c)
        cases = [(lg, n, 1, 0, tile_log, 0), (lg, n, 1, 1, tile_log, 0), (lg, len(short), 1, 0, tile_log, n)]
        res, _ = _walk(driver, tmp_path, name, cases, full + short)
        assert [mc.recorded(r) for r in res] == [c[k] for k in ("forward", "inverse", "padded")], (name, n)
        out = _call(driver, tmp_path, c["p"], ["mul", lg, len(a), len(b), tile_log, c["root"]], a=words(a), b=words(b))
        assert out.returncode == 0
        assert mc.recorded(ints((tmp_path / "out").read_bytes())) == c["mul_polys"], (name, n)


def test_mul_small(driver, tmp_path):
    for name in ("goldilocks", "big18", "f257", "composite"):
        p = MODULI[name]
        for lg in range(min(6, nc.max_log(name)) + 1):
            n = 1 << lg
            for n_a, n_b in sorted({(n, n), (n // 2 + 1, 1), (0, n)}):
                a, b = nc.inputs(lg, n_a, p), nc.inputs(lg + 50, n_b, p)
                out = _call(driver, tmp_path, p, ["mul", lg, n_a, n_b, 12, root_of(name, n)], a=words(a), b=words(b))
                assert out.returncode == 0
                assert ints((tmp_path / "out").read_bytes()) == mc.cyclic_times_n([v % p for v in a], [v % p for v in b], n, p)


# ---- (e) the access patterns of the default plan --------------------------------------------------------------------------------------
SHAPES = [(16, 1), (20, 1), (20, 8), (24, 1), (28, 1)]


def _maps(driver, d, mode, lg, batch, tile_log=12):
    out = _call(driver, d, nc.GOLDILOCKS, [mode, lg, batch, tile_log])
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [[int(v) for v in line.split()] for line in out.stdout.splitlines()]
    assert [r[0] for r in rows] == list(range(passes_of(lg, tile_log)))
    return rows


@pytest.mark.parametrize("lg,batch", SHAPES)
def test_runs(driver, tmp_path, lg, batch):
    """every global load and store instruction of every pass addresses runs of at least 16 consecutive elements (128 bytes) per 16
    adjacent lanes: the first tile, the last tile and 64 between, enumerated through the maps the phases call"""
    for d, load_run, store_run in _maps(driver, tmp_path, "runs", lg, batch):
        assert load_run >= 16 and store_run >= 16, (lg, batch, d, load_run, store_run)


@pytest.mark.parametrize("lg,batch", SHAPES)
def test_banks(driver, tmp_path, lg, batch):
    """at most 2-way conflicts in any lane group of any LDS instruction (ds_read_b64: 2 x 32 lanes, 64 banks; ds_write_b64: 4 x 16
    lanes, 32 banks), same tiles"""
    for row in _maps(driver, tmp_path, "banks", lg, batch):
        assert max(row[1:]) <= 2, (lg, batch, row)
        print("banks", lg, batch, row)


def test_runs_see_a_strided_pass(driver, tmp_path):
    """the measure is not vacuous: a tile of 4 columns (tile log 5, radix 8) has runs of 4"""
    rows = _maps(driver, tmp_path, "runs", 16, 1, tile_log=5)
    assert min(r[1] for r in rows) < 16


# ---- (f) the same driver under AddressSanitizer and UBSan -----------------------------------------------------------------------------
def test_sanitizer_build(san_driver, tmp_path):
    """2^0 .. 2^10 at tile logs 12, 3 and 5 and the `runs` / `banks` enumeration: no report (a report exits non-zero)"""
    name = "big18"
    p = MODULI[name]
    blob = nc.inputs(77, 3 << 10, p)
    for tile_log in (12, 3, 5):
        cases = _grid(10, tile_log)
        res, passes = _walk(san_driver, tmp_path, name, cases, blob)
        _check_grid(name, cases, res, passes, blob)
    for mode in ("runs", "banks"):
        out = _call(san_driver, tmp_path, nc.GOLDILOCKS, [mode, 16, 1, 12])
        assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
        out = _call(san_driver, tmp_path, nc.GOLDILOCKS, [mode, 28, 1, 12])
        assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]


# ---- (g) the package --------------------------------------------------------------------------------------------------------------------
def test_import_creates_no_context():
    import sys
    code = ("import sys; sys.path.insert(0, %r); import starks_amd.fft as f; from starks_amd import _lib; "
            "assert _lib._ctx is None and _lib._lib is None; assert callable(f.mod64_ntt) and callable(f.mod64_mul_polys); "
            "assert 'numpy' not in sys.modules; print('ok')" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr
