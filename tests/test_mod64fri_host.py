"""The packed-word FRI commit's CPU half: tests/native/mod64fri_host.cpp (hipcc, host code under AddressSanitizer and UBSan; a
stand-alone program, nothing is loaded into Python under a sanitizer) walks the commit exactly as starks_amd/csrc/api_mod64fri.hip issues
it -- the transform through ntt64_items.cuh, the leaf, fold and gather items of mod64fri_items.cuh over the grids the library launches,
the upper tree levels with b2_hash_pair -- and every case of tests/mod64fri_cases.py up to n = 4096 equals the exact oracle
(oracle/pyoracle.py with p = the modulus) byte for byte; the oracle's verifier accepts each proof; the fold alone at the edge challenges
and round shifts; the tree alone; forced transform plans; the library cross-compiles and exports what the header declares.  CPU only.
What this half does NOT run: the index sampler (a device-only kernel; the driver samples with its own host copy of utils.py's
get_pseudorandom_indices) and fri_validate (restated as the driver's shape_ok): the GPU grid covers both (tests/test_gpu_mod64fri.py)."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
import mod64fri_cases as qc
import modfri_cases as fc
import ntt64_cases as nc
from mod64fri_cases import HOST_GRID, MODULI, root_of
from oracle import pyoracle

CSRC = os.path.join(ROOT, "starks_amd", "csrc")
SYMBOLS = ("sh_mod64_fri_prove", "sh_dev_mod64_fri_prove", "sh_mod64_fri_fold", "sh_dev_mod64_merkelize")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("m6") / "mod64fri_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-g", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "mod64fri_host.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, args, **files):
    for name, data in files.items():
        (d / name).write_bytes(data)
    return subprocess.run([driver, args[0], str(d)] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=600)


def _prove(driver, d, name, cases, tile_log=12):
    """the flat proofs of `cases` (all over MODULI[name]) from one run of the driver"""
    blob, lines = [], []
    for c in cases:
        lines.append("%d %d %d %d %d %d %d %d %d" % (c.n.bit_length() - 1, c.n_coeffs, c.batch, c.md, c.exclude, c.samples, tile_log, len(blob),
                                                     c.root))
        blob += c.coeffs()
    out = _call(driver, d, ["prove", MODULI[name]], cases=("\n".join(lines) + "\n").encode(), **{"in": nc.words(blob)})
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    raw, res, k = (d / "out").read_bytes(), [], 0
    for c in cases:
        ln = len(qc.oracle_flat(c))
        res.append(raw[k:k + ln])
        k += ln
    assert k == len(raw)
    return res


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(driver, tmp_path, name):
    """every case of the modulus: the host walk equals the oracle's flat proof byte for byte, and the oracle's verifier accepts it"""
    cases = [c for c in HOST_GRID if c.name == name]
    assert cases
    for c, got in zip(cases, _prove(driver, tmp_path, name, cases)):
        assert got == qc.oracle_flat(c), c.id
        if c.verify:
            for b, proof in enumerate(qc.oracle_proofs(c)):
                assert qc.oracle_verify(c, proof, b), c.id


def test_grid_covers_what_it_must():
    """a guard on the case table itself (tests/mod64fri_cases.py), not on the code: it keeps a later edit from dropping a form"""
    ids = {c.id for c in qc.GRID}
    assert len(ids) == len(qc.GRID)
    assert sorted(MODULI) == sorted(["f17", "f257", "f65537", "babybear", "goldilocks", "composite", "c2", "koalabear", "big18", "p64_59"])
    assert all(p % 2 == 1 and 3 <= p < 2**64 for p in MODULI.values())
    # every modfri_cases shape of a modulus below 2^64 is here under the same id, so that its oracle proofs are modfri_cases' own
    small = [c for c in fc.GRID if c.p < 2**64]
    assert small and all(c.id in ids and qc._BY_ID[c.id].coeffs() == [v % c.p for v in c.coeffs()] for c in small)
    have = {(c.name, c.n, c.md, c.n_coeffs, c.exclude, c.samples, c.batch, c.const) for c in qc.GRID}
    top = qc.BIG18 - 1
    for want in (("koalabear", 16, 16, 3, 0, 40, 1, None), ("koalabear", 64, 32, 32, 0, 40, 1, None), ("koalabear", 256, 128, 128, 0, 40, 1, None),
                 ("big18", 16, 16, 16, 0, 40, 1, None), ("big18", 64, 32, 32, 0, 40, 1, None), ("big18", 256, 128, 128, 0, 40, 1, None),
                 ("big18", 4096, 1024, 1000, 0, 40, 1, None), ("big18", 64, 32, 1, 0, 40, 1, top), ("big18", 16, 16, 1, 0, 40, 1, top),
                 ("p64_59", 4, 1, 1, 0, 40, 1, None)):
        assert want in have, want
    big = [c for c in qc.GRID if c.name == "big18"]
    assert any(c.batch == 3 and c.n == 64 for c in big) and {7, 80} <= {c.samples for c in big}
    assert any(c.exclude == 8 and c.n == 1024 for c in big)
    assert {c.rounds() for c in big} == {0, 1, 2, 3}
    # sums and the halving carry out of 64 bits, and the inputs include words at or above p
    assert qc.BIG18 == 2**64 - 1835007 and qc.BIG18 > 2**63 and top >> 63 == 1
    assert any(v >= qc.BIG18 for v in qc._BY_ID["big18-n64-md32-c32-x0-s40-b1"].coeffs())
    b = qc.BOTH_TREE_FORMS
    assert b.name == "big18" and b.n == 1 << 14 and b.batch == 3 and b.n * b.batch > 1 << 15 >= b.n // 4 * b.batch
    for c in qc.GRID + [b]:
        assert pow(c.root, c.n, c.p) == 1 and (c.n == 1 or pow(c.root, c.n // 2, c.p) == c.p - 1), c.id


def test_top_bit_leaves(driver, tmp_path):
    """the constant polynomial p - 1 over BIG18: every leaf, column value and final value is p - 1, top bit set, 24 zero bytes in front"""
    top = bytes(24) + (qc.BIG18 - 1).to_bytes(8, "big")
    cases = [c for c in HOST_GRID if c.const is not None]
    assert [c.n for c in cases] == [64, 16]
    for c, got in zip(cases, _prove(driver, tmp_path, "big18", cases)):
        assert got == qc.oracle_flat(c)
        assert got[-32 * (c.n >> (2 * c.rounds())):] == top * (c.n >> (2 * c.rounds()))
        if c.rounds():
            lg = c.n.bit_length() - 1
            first = got[32:32 + 32 * ((lg - 1) + 4 * (lg + 1))]  # the first sample's five branches: each opens with a leaf and its sibling
            assert first[:64] == top * 2 and first[32 * (lg - 1):32 * (lg - 1) + 64] == top * 2


@pytest.mark.parametrize("tile_log", [3, 5])
def test_forced_transform_plans(driver, tmp_path, tile_log):
    """the same proofs when the transform in front runs as several passes: the fold reads the lo | hi table of that plan"""
    cases = [c for c in HOST_GRID if c.name == "big18" and c.n in (64, 256) and c.const is None]
    assert len(cases) >= 4
    for c, got in zip(cases, _prove(driver, tmp_path, "big18", cases, tile_log)):
        assert got == qc.oracle_flat(c), c.id


# ---- the fold alone ------------------------------------------------------------------------------------------------------------------
def _sx(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("name", ["f257", "goldilocks", "big18", "c2"])
def test_fold(driver, tmp_path, name, shift):
    """m6_fold_item against pyoracle.fri_fold on n = 16 words whose round-0 domain has n << shift points, at the challenges 0, 1,
    p - 1, p, 2^256 - 1, a point of the domain (its row returns the row's own value) and the negative of one; words >= p included"""
    p, n = MODULI[name], 16
    w0 = root_of(name, n << shift)
    xs = pyoracle.get_power_cycle(pow(w0, 1 << shift, p), p)
    assert len(xs) == n
    vals = nc.inputs(5 + shift, n, p)
    sxs = fc.fold_challenges(p, xs, 6)
    out = _call(driver, tmp_path, ["fold", p, 4, shift, w0], values=nc.words(vals), sx=_sx(sxs))
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got = nc.ints((tmp_path / "out").read_bytes())
    canon = [v % p for v in vals]
    for k, sx in enumerate(sxs):
        assert got[4 * k:4 * k + 4] == pyoracle.fri_fold(canon, xs, sx % p, p), (name, shift, k)
    assert got[4 * 5 + 6 % 4] == canon[6]  # x* = xs[6]: the row through it (row 6 mod 4, slot 6 // 4) interpolates its own value


def test_fold_p64_59(driver, tmp_path):
    """n = 4, one row, over the largest prime below 2^64: every sum carries"""
    p, n = MODULI["p64_59"], 4
    w = root_of("p64_59", 4)
    xs = pyoracle.get_power_cycle(w, p)
    vals = [p - 1, 2**64 - 1, p - 2, 1]
    sxs = fc.fold_challenges(p, xs, 1)
    out = _call(driver, tmp_path, ["fold", p, 2, 0, w], values=nc.words(vals), sx=_sx(sxs))
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got = nc.ints((tmp_path / "out").read_bytes())
    assert got == [pyoracle.fri_fold([v % p for v in vals], xs, sx % p, p)[0] for sx in sxs]


# ---- the tree, hashed as stored ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(4, 1), (16, 3), (1024, 1)])
def test_tree(driver, tmp_path, n, batch):
    p = qc.BIG18
    vals = nc.inputs(n, n * batch, p)
    vals[0], vals[1], vals[2], vals[-1] = 0, p - 1, 2**64 - 1, 2**64 - 1
    out = _call(driver, tmp_path, ["tree", p, n.bit_length() - 1, batch], values=nc.words(vals))
    assert out.returncode == 0, out.stderr[-3000:]
    raw = (tmp_path / "out").read_bytes()
    for b in range(batch):
        want = pyoracle.merkelize(vals[b * n:(b + 1) * n])
        assert raw[64 * n * b:64 * n * (b + 1)] == bytes(32) + b"".join(want[1:]), (n, b)


# ---- the library ---------------------------------------------------------------------------------------------------------------------
def test_library_cross_compiles():
    """the two new translation units for gfx950, and the symbols the header declares in the built library"""
    for src in ("mod64fri.hip", "api_mod64fri.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=600)
    from starks_amd import _lib, fri
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header
    assert callable(fri.mod64_prove_flat) and callable(fri.mod64_fold)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " mod64fri.hip" in mk and " api_mod64fri.hip" in mk and " mod64fri_items.cuh" in mk
