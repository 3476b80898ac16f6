"""The generic-modulus FRI commit's CPU half: tests/native/modfri_host.cpp (hipcc, host code under AddressSanitizer and UBSan) walks the
commit exactly as starks_amd/csrc/api_modfri.hip issues it -- the transform through modntt_items.cuh, the leaf, fold and gather items of
modfri_items.cuh over the grids the library launches, the upper tree levels with b2_hash_pair -- and every case of
tests/modfri_cases.py up to n = 4096 equals the exact oracle (oracle/pyoracle.py with p = the modulus) byte for byte; the oracle's
verifier accepts each proof; the fold alone at the edge challenges and round shifts; the oracle against tests/golden/mod_fri.json (the
live reference's primitives); the library cross-compiles; the Python routing rule.  CPU only.
What this half does NOT run: the index sampler.  The library's sampler is a device-only kernel (fri_sample_all_kernel behind
shk_fri_sample_all), so the driver samples with its own host copy of utils.py's get_pseudorandom_indices; that kernel and its wrapper are
covered by the GPU grid alone (tests/test_gpu_modfri.py).  The driver's shape_ok likewise restates fri_validate, which lives in a
translation unit that needs the HIP runtime."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT, load_golden
import modfri_cases as fc
import modntt_cases as mc
from modfri_cases import HOST_GRID, MODULI, root_of
from modntt_cases import ints, wire
from oracle import pyoracle

CSRC = os.path.join(ROOT, "starks_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mf") / "modfri_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-g", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "modfri_host.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, args, **files):
    for name, data in files.items():
        (d / name).write_bytes(data)
    return subprocess.run([driver, args[0], str(d)] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=600)


def _prove(driver, d, name, cases, tile_log=10):
    """the flat proofs of `cases` (all over MODULI[name]) from one run of the driver"""
    blob, lines = [], []
    for c in cases:
        lines.append("%d %d %d %d %d %d %d %d %s" % (c.n.bit_length() - 1, c.n_coeffs, c.batch, c.md, c.exclude, c.samples, tile_log, len(blob),
                                                     wire([c.root]).hex()))
        blob += c.coeffs()
    out = _call(driver, d, ["prove"], mod=wire([MODULI[name]]), cases=("\n".join(lines) + "\n").encode(), **{"in": wire(blob)})
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    raw, res, k = (d / "out").read_bytes(), [], 0
    for c in cases:
        ln = len(fc.oracle_flat(c))
        res.append(raw[k:k + ln])
        k += ln
    assert k == len(raw)
    return res


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(driver, tmp_path, name):
    """every case of the modulus: the host walk equals the oracle's flat proof byte for byte, and the oracle's verifier accepts it"""
    cases = [c for c in HOST_GRID if c.name == name]
    assert cases and (name in ("f17", "composite") or any(c.rounds() for c in cases))
    for c, got in zip(cases, _prove(driver, tmp_path, name, cases)):
        assert got == fc.oracle_flat(c), c.id
        if c.verify:
            for b, proof in enumerate(fc.oracle_proofs(c)):
                assert fc.oracle_verify(c, proof, b), c.id


def test_grid_covers_what_it_must():
    """a guard on the case table itself (tests/modfri_cases.py), not on the code: it keeps a later edit from dropping a form"""
    ids = {c.id for c in fc.GRID}
    assert len(ids) == len(fc.GRID)
    for name in MODULI:
        for n, md, k in ((16, 16, 3), (16, 16, 16), (4, 1, 1), (1, 1, 1)):
            assert any(c.name == name and (c.n, c.md, c.n_coeffs) == (n, md, k) for c in fc.GRID), (name, n)
        if name not in ("f17", "composite"):
            assert any(c.name == name and c.rounds() >= 1 for c in fc.GRID), name
    assert {c.rounds() for c in fc.GRID} == {0, 1, 2, 3}
    assert {c.samples for c in fc.GRID} == {7, 40, 80} and {c.batch for c in fc.GRID} == {1, 3}
    assert fc.BOTH_TREE_FORMS.n * fc.BOTH_TREE_FORMS.batch > 1 << 15 >= fc.BOTH_TREE_FORMS.n // 4 * fc.BOTH_TREE_FORMS.batch
    assert fc.P43 > mc.MIMC_P and pow(7, (fc.P43 - 1) // 2, fc.P43) == fc.P43 - 1 and fc.C2 == 257 * 65537
    for n, w in fc.C2_ROOTS.items():
        assert pow(w, n // 2, fc.C2) == fc.C2 - 1


def test_above_the_mimc_prime(driver, tmp_path):
    """the constant polynomial p - 1 over P43: every leaf, column value and final value is p - 1 >= MIMC_P, unchanged"""
    top = wire([fc.P43 - 1])
    assert fc.P43 - 1 >= mc.MIMC_P
    cases = [c for c in HOST_GRID if c.const is not None]
    assert [c.n for c in cases] == [64, 16]
    for c, got in zip(cases, _prove(driver, tmp_path, "p43", cases)):
        assert got == fc.oracle_flat(c)
        assert got[-32 * (c.n >> (2 * c.rounds())):] == top * (c.n >> (2 * c.rounds()))
        if c.rounds():
            lg = c.n.bit_length() - 1
            first = got[32:32 + 32 * ((lg - 1) + 4 * (lg + 1))]  # the first sample's five branches: each opens with a leaf and its sibling
            assert first[:64] == top * 2 and first[32 * (lg - 1):32 * (lg - 1) + 64] == top * 2


@pytest.mark.parametrize("tile_log", [3, 5])
def test_forced_transform_plans(driver, tmp_path, tile_log):
    """the same proofs when the transform in front runs as several passes"""
    cases = [c for c in HOST_GRID if c.name == "bn254" and c.n in (64, 256)]
    for c, got in zip(cases, _prove(driver, tmp_path, "bn254", cases, tile_log)):
        assert got == fc.oracle_flat(c), c.id


# ---- the fold alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("name", ["f257", "goldilocks", "bn254", "p43", "c2", "mimc"])
def test_fold(driver, tmp_path, name, shift):
    """mf_fold_item against pyoracle.fri_fold on n = 16 values whose round-0 domain has n << shift points, at the challenges 0, 1,
    p - 1, p, 2^256 - 1, a point of the domain (its row returns the row's own value) and the negative of one; values >= p included"""
    p, n = MODULI[name], 16
    w0 = root_of(name, n << shift)
    xs = pyoracle.get_power_cycle(pow(w0, 1 << shift, p), p)
    assert len(xs) == n
    vals = mc.inputs(5 + shift, n, p)
    sxs = fc.fold_challenges(p, xs, 6)
    out = _call(driver, tmp_path, ["fold", 4, shift], mod=wire([p]), root=wire([w0]), values=wire(vals), sx=wire(sxs))
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    got = ints((tmp_path / "out").read_bytes())
    canon = [v % p for v in vals]
    for k, sx in enumerate(sxs):
        assert got[4 * k:4 * k + 4] == pyoracle.fri_fold(canon, xs, sx % p, p), (name, shift, k)
    assert got[4 * 5 + 6 % 4] == canon[6]  # x* = xs[6]: the row through it (row 6 mod 4, slot 6 // 4) interpolates its own value


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_oracle():
    """pyoracle over other moduli restates the live reference's primitives (tests/golden/generate_mod_fri.py)"""
    G = load_golden("mod_fri.json")["cases"]
    assert sorted(G) == sorted(fc.FIXTURE)
    for key, c in fc.FIXTURE.items():
        assert fc.recorded(c) == G[key], key
        assert G[key]["len"] == len(fc.oracle_flat(c)) and len(G[key]["rounds"]) == c.rounds()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mod_fri.json")) < 16384


def test_fixture_host_walk(driver, tmp_path):
    G = load_golden("mod_fri.json")["cases"]
    for key, c in fc.FIXTURE.items():
        got = _prove(driver, tmp_path, c.name, [c])[0]
        assert hashlib.sha256(got).hexdigest() == G[key]["sha256"] and got[:64].hex() == G[key]["head"], key


# ---- the tree, hashed as stored ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(4, 1), (16, 3), (1024, 1)])
def test_plain_tree(driver, tmp_path, n, batch):
    vals = mc.inputs(n, n * batch, fc.P43)
    vals[0], vals[1], vals[-1] = fc.P43 - 1, 2**256 - 1, 2**256 - 1
    out = _call(driver, tmp_path, ["tree", n.bit_length() - 1, batch], values=wire(vals))
    assert out.returncode == 0, out.stderr[-3000:]
    raw = (tmp_path / "out").read_bytes()
    for b in range(batch):
        want = pyoracle.merkelize(vals[b * n:(b + 1) * n])
        assert raw[64 * n * b:64 * n * (b + 1)] == bytes(32) + b"".join(want[1:]), (n, b)


# ---- the library and the Python call sites -------------------------------------------------------------------------------------------
def test_library_cross_compiles():
    """the two new translation units for gfx950, and the symbols the header declares in the built library"""
    for src in ("modfri.hip", "api_modfri.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=600)
    from starks_amd import _lib
    L = _lib.lib()
    for name in ("sh_mod_fri_prove", "sh_dev_mod_fri_prove", "sh_mod_fri_fold", "sh_dev_merkelize_plain"):
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("sh_mod_fri_prove", "sh_dev_mod_fri_prove", "sh_mod_fri_fold", "sh_dev_merkelize_plain"):
        assert "int %s(" % name in header


def test_routing_rule(monkeypatch):
    """without a device: a non-MiMC odd modulus goes to mod_prove_flat with its modulus, the MiMC prime keeps prove_flat, an even
    modulus and a root whose order is no power of two still raise NotImplementedError"""
    from starks_amd import IntegersModP, _lib, fri
    from starks_amd.wireseq import WireList
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("routing must not ask for a context"))
    calls = []
    c = fc.FIXTURE["bn254-64"]

    def fake_mod(modulus, coeff_bytes, n, root, md, exclude=0, samples=40, batch=1):
        calls.append(("mod", modulus, coeff_bytes, n, root, md, exclude, samples))
        return pyoracle.proof_flat(pyoracle.prove_low_degree(ints(coeff_bytes), root, md, p=modulus, exclude_multiples_of=exclude,
                                                             fri_spot_check_security_factor=samples))

    def fake_mimc(coeff_bytes, n, root, md, exclude=0, samples=40, batch=1):
        calls.append(("mimc", n))
        return bytes(32 * n)

    monkeypatch.setattr(fri, "mod_prove_flat", fake_mod)
    monkeypatch.setattr(fri, "prove_flat", fake_mimc)
    F = IntegersModP(c.p)
    co = [v % c.p for v in c.coeffs()]
    want = fc.oracle_proofs(c)[0]
    # field elements, plain ints under the driver's field, and a WireList over the field: the same call
    for f in ([F(v) for v in co], co, WireList(wire(co), F)):
        del calls[:]
        assert fri.SmoothSubgroupFRI(F).generate_proximity_proof(f, F(c.root), c.md) == want
        assert calls == [("mod", c.p, wire(co), 64, c.root, 32, 0, 40)]
    del calls[:]
    assert fri.prove_low_degree([F(v) for v in co], c.root, c.md, 4, 7)[-1] == want[-1]
    assert calls[0][6:] == (4, 7)
    # the MiMC prime keeps its own prover
    del calls[:]
    Fm = IntegersModP(mc.MIMC_P)
    fri.SmoothSubgroupFRI(Fm).generate_proximity_proof([Fm(1), Fm(2)], mc.root_of("mimc", 16), 16)
    fri.prove_low_degree([1, 2], mc.root_of("mimc", 16), 16)
    assert calls == [("mimc", 16), ("mimc", 16)]
    # not accelerated: an even modulus, a root of order 6 or 5 (the reference's Z/31), more coefficients than points
    del calls[:]
    Fe = IntegersModP(1 << 64)
    with pytest.raises(NotImplementedError):
        fri.SmoothSubgroupFRI(Fe).generate_proximity_proof([Fe(1)], Fe(3), 16)
    F31 = IntegersModP(31)
    for w in (15, 2):
        with pytest.raises(NotImplementedError):
            fri.SmoothSubgroupFRI(F31).generate_proximity_proof([F31(1)], F31(w), 16)
    with pytest.raises(ValueError):
        fri.prove_low_degree([F(1)] * 65, c.root, 32)
    assert calls == []
