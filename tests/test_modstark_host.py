"""The generic-modulus STARK prover's CPU half: tests/native/modstark_host.cpp (hipcc, host code under AddressSanitizer and UBSan)
walks the prover exactly as starks_amd/csrc/api_modstark.hip issues it -- the transforms through modntt_items.cuh, the items of
modstark_items.cuh over the grids modstark.hip launches, the trees and commit rounds through modfri_items.cuh -- and every case of
tests/modstark_cases.py equals the exact oracle (oracle/pyoracle.py with p = the modulus) byte for byte; the oracle's verifier accepts
each proof; the broken witnesses flag; the batch inversion against pow(v, -1, p); the oracle against tests/golden/mod_stark.json (the
live reference's STARK over IntegersModP(p)); the library cross-compiles; the Python routing rule.  CPU only.
What this half does NOT run: the index sampler (a device-only kernel of the MiMC path: the driver samples with its own host copy of
utils.py's get_pseudorandom_indices) and the host checks of api_modstark.hip, which need the HIP runtime; both are covered by
tests/test_gpu_modstark.py."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT, load_golden
import modntt_cases as mc
import modstark_cases as sc
from modstark_cases import HOST_GRID, MODULI
from modntt_cases import ints, wire
from oracle import pyoracle

CSRC = os.path.join(ROOT, "starks_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ms") / "modstark_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-g", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "modstark_host.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, args, **files):
    for name, data in files.items():
        (d / name).write_bytes(data)
    return subprocess.run([driver, args[0], str(d)] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=600)


def _prove(driver, d, name, cases, tile_log=10, witnesses=None):
    """-> ([flat proofs of each case], [flags of each case]) from one run of the driver; all cases over MODULI[name]"""
    blob, lines = b"", []
    for c in cases:
        lines.append("%d %d %d %d %d %d" % (c.steps, c.ext, c.width, c.samples, c.batch, tile_log))
        blob += c.witness_wire(witnesses) + c.input_wire() + c.terms_blob()
    out = _call(driver, d, ["prove"], mod=wire([MODULI[name]]), cases=("\n".join(lines) + "\n").encode(), **{"in": blob})
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    raw, flags, res, fl, k, j = (d / "out").read_bytes(), (d / "flags").read_bytes(), [], [], 0, 0
    for c in cases:
        ln = sc.proof_len(c) * c.batch
        res.append(raw[k:k + ln])
        fl.append(list(flags[j:j + c.batch]))
        k, j = k + ln, j + c.batch
    assert k == len(raw) and j == len(flags)
    return res, fl


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(driver, tmp_path, name):
    """every case of the modulus: the host walk equals the oracle's flat proof byte for byte, no flag is raised, and the oracle's
    verifier accepts the proof"""
    cases = [c for c in HOST_GRID if c.name == name]
    assert cases
    proofs, flags = _prove(driver, tmp_path, name, cases)
    for c, got, fl in zip(cases, proofs, flags):
        assert got == sc.oracle_flat(c), c.id
        assert fl == [0] * c.batch, c.id
        for b, proof in enumerate(sc.oracle_proofs(c)):
            assert sc.oracle_verify(c, proof, b), c.id


def test_grid_covers_what_it_must():
    """a guard on the case table itself (tests/modstark_cases.py), not on the code: it keeps a later edit from dropping a case"""
    ids = [c.id for c in sc.GRID]
    assert len(set(ids)) == len(ids)
    assert set(MODULI) == {"bn254", "bls12_381", "goldilocks", "mimc", "p43", "f257", "f65537", "f17"}
    have = {(c.name, c.steps, c.ext, c.width, c.degree) for c in sc.GRID if c.batch == 1 and c.samples == 80 and not c.plus_p}
    for name in MODULI:
        assert (name, 2, 8, 1, 1) in have
        if name != "f17":
            for shape in ((8, 8, 2, 3), (16, 4, 1, 3), (32, 8, 3, 3), (8, 8, 9, 5)):
                assert (name,) + shape in have, (name, shape)
    assert [c.shape for c in sc.GRID if c.name == "f17"] == ["s2"]
    assert any(c.name == "f257" and c.n == 257 - 1 for c in sc.GRID)  # the domain is the whole group
    assert any(set(d) == {(1, 1, 0)} for c in sc.GRID for d in c.sp)  # a product of two variables
    assert {c.batch for c in sc.GRID} == {1, 3} and {c.samples for c in sc.GRID} == {7, 80}
    assert any(any(all(v == 0 for v in d.values()) for d in c.sp) for c in sc.GRID)  # a zero step polynomial
    assert sum(1 for c in sc.GRID if c.plus_p) >= 3
    for c in sc.GRID:
        if c.plus_p and c.p < 2**255:  # stored values at or above p, in the witness, the inputs and the coefficients
            assert any(v >= c.p for v in ints(c.witness_wire())) and any(v >= c.p for v in c.terms()[1]), c.id
    assert any(c.plus_p and any(v >= c.p for v in ints(c.input_wire())) for c in sc.GRID)
    # zero, one and two commit rounds
    assert {0, 1, 2} <= {len(sc.oracle_proofs(c)[0][3]) - 1 for c in sc.GRID if c.name == "bn254"}
    assert sc.P43 > sc.MIMC_P and sc.P43_CONST.inputs == [[sc.P43 - 1]] and (sc.P43_CONST.steps, sc.P43_CONST.ext) == (16, 8)
    units, flags = sc.broken_witnesses()
    assert len(units) == 1 + sc.BREAK_BASE.width * sc.BREAK_BASE.steps == 17 and flags == [0] + [1] * 16
    for name in MODULI:  # G2 has full order over every modulus of the grid, and not over BabyBear
        for c in sc.GRID:
            if c.name == name:
                assert pow(pow(7, (c.p - 1) // c.n, c.p), c.n // 2, c.p) == c.p - 1
    assert pow(pow(7, (sc.BABYBEAR - 1) // 64, sc.BABYBEAR), 32, sc.BABYBEAR) != sc.BABYBEAR - 1


def test_above_the_mimc_prime(driver, tmp_path):
    """X' = X^3 from p - 1 over P43: the whole trace is p - 1 >= MIMC_P, and every P value in every opened leaf appears as p - 1"""
    c = sc.P43_CONST
    assert c.witnesses() == [[[sc.P43 - 1] * 16]] and sc.P43 - 1 >= sc.MIMC_P
    (got,), (fl,) = _prove(driver, tmp_path, "p43", [c])
    assert got == sc.oracle_flat(c) and fl == [0]
    opened = sc.opened_p_values(got, c)
    assert len(opened) == 4 * c.samples and set(opened) == {sc.P43 - 1}
    assert sc.oracle_verify(c, sc.oracle_proofs(c)[0])


def test_broken_witnesses(driver, tmp_path):
    """every single-element break of one small witness in one batch: exactly the broken proofs flag, the valid one keeps its bytes"""
    units, want = sc.broken_witnesses()
    base = sc.BREAK_BASE
    batch = sc.Case(base.name, base.shape, base.steps, base.ext, base.sp, batch=len(units), inputs=base.inputs * len(units), tag="-breakbatch")
    blob = batch.witness_wire(units) + batch.input_wire() + batch.terms_blob()
    out = _call(driver, tmp_path, ["prove"], mod=wire([base.p]), cases=b"%d %d %d %d %d 10\n" % (base.steps, base.ext, base.width, 80, len(units)),
                **{"in": blob})
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    assert list((tmp_path / "flags").read_bytes()) == want
    ln = sc.proof_len(base)
    assert (tmp_path / "out").read_bytes()[:ln] == sc.oracle_flat(base)
    with pytest.raises(AssertionError):  # the reference's `assert cp % z == 0` (stark.py:76)
        pyoracle.mk_stark_proof(units[1], base.inputs[0], base.sp, base.steps, base.ext, p=base.p)


@pytest.mark.parametrize("tile_log", [3, 5])
def test_forced_transform_plans(driver, tmp_path, tile_log):
    """the same proofs when the transforms run as several passes"""
    cases = [c for c in HOST_GRID if c.name == "bn254" and c.shape in ("s8", "s32") and not c.plus_p and c.batch == 1]
    assert len(cases) == 2
    proofs, _ = _prove(driver, tmp_path, "bn254", cases, tile_log)
    for c, got in zip(cases, proofs):
        assert got == sc.oracle_flat(c), c.id


def test_refusals(driver, tmp_path):
    """the driver's restatement of the host checks: an even modulus, BabyBear (7 is a residue), a cubic at ext 2"""
    c = [x for x in HOST_GRID if x.name == "bn254" and x.shape == "s16x4"][0]
    blob = c.witness_wire() + c.input_wire() + c.terms_blob()
    line = b"%d %d %d %d %d 10\n" % (c.steps, c.ext, c.width, c.samples, c.batch)
    assert _call(driver, tmp_path, ["prove"], mod=wire([1 << 64]), cases=line, **{"in": blob}).returncode == 2
    assert _call(driver, tmp_path, ["prove"], mod=wire([sc.BABYBEAR]), cases=line, **{"in": blob}).returncode == 3
    assert _call(driver, tmp_path, ["prove"], mod=wire([c.p]), cases=b"16 2 1 80 1 10\n", **{"in": blob}).returncode == 4


# ---- the batch inversion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "goldilocks", "p43", "f257", "f17"])
@pytest.mark.parametrize("count", [1, 31, 32, 33, 100])
def test_batch_inversion(driver, tmp_path, name, count):
    """ms_batch_inv_item against pow(v, -1, p): zeros map to zero, a chunk that is all zeros, counts around the chunk boundary (32 values
    per item: at 33 item 0 owns two values and item 1 one)"""
    p = MODULI[name]
    vals = [v % p for v in mc.inputs(count, count, p)]
    vals[0] = 0
    if count > 40:
        vals[40] = p - 1
        vals[3] = vals[7] = 0
    out = _call(driver, tmp_path, ["inv"], mod=wire([p]), values=wire(vals))
    assert out.returncode == 0, out.stderr[-3000:]
    assert ints((tmp_path / "out").read_bytes()) == [pow(v, -1, p) if v else 0 for v in vals]


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
def test_fixture_oracle():
    """pyoracle over other moduli restates the live reference's STARK.mk_proof (tests/golden/generate_mod_stark.py)"""
    G = load_golden("mod_stark.json")["cases"]
    assert sorted(G) == sorted(sc.FIXTURE)
    for key, c in sc.FIXTURE.items():
        assert sc.recorded(c) == G[key], key
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "mod_stark.json")) < 16384


def test_fixture_host_walk(driver, tmp_path):
    G = load_golden("mod_stark.json")["cases"]
    for key, c in sc.FIXTURE.items():
        (got,), _ = _prove(driver, tmp_path, c.name, [c])
        assert hashlib.sha256(got).hexdigest() == G[key]["sha256"] and got[:64].hex() == G[key]["head"], key


# ---- the library and the Python call sites -------------------------------------------------------------------------------------------
def test_library_cross_compiles():
    """the two new translation units for gfx950, and the symbols the header declares in the built library"""
    for src in ("modstark.hip", "api_modstark.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("sh_mod_stark_prove", "sh_dev_mod_stark_prove"):
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header


def test_routing_rule(monkeypatch):
    """without a device: STARK over BN254 constructs and mk_proof goes to mod_prove_flat with its modulus, wire values modulo p and the
    terms packed modulo p; the MiMC prime keeps prove_flat; BabyBear (7 is a residue) and an even modulus raise NotImplementedError"""
    from starks_amd import IntegersModP, _lib, stark
    from starks_amd.multivariate_polynomial import multivariates_over
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("routing must not ask for a context"))
    c = sc.FIXTURE["bn254-s8-w2"]
    calls = []

    def fake_mod(modulus, witness_bytes, input_bytes, steps, ext, width, step_polys, batch=1, samples=80):
        calls.append(("mod", modulus, witness_bytes, input_bytes, steps, ext, width, batch, samples))
        assert stark.pack_step_polys(step_polys, width, p=modulus)[:2] == (wire(c.terms()[1]), c.terms()[2])
        return sc.oracle_flat(c)

    def fake_mimc(witness_bytes, input_bytes, steps, ext, width, step_polys, batch=1, samples=80):
        calls.append(("mimc", steps))
        return bytes(stark_len)

    monkeypatch.setattr(stark, "mod_prove_flat", fake_mod)
    monkeypatch.setattr(stark, "prove_flat", fake_mimc)
    monkeypatch.setattr(stark, "proof_len", lambda *a, **k: pytest.fail("routing must not load the library"))
    F = IntegersModP(c.p)
    mv = multivariates_over(F, c.width).factory
    sp = [mv({k: F(v) for k, v in d.items()}) for d in c.sp]
    st = stark.STARK(F, c.steps, c.ext, c.width, sp)
    assert st.modulus == c.p and int(st.G2) == pow(7, (c.p - 1) // 64, c.p)
    w = c.witnesses()[0]
    boundary = [(0, j, F(v)) for j, v in enumerate(c.inputs[0])]
    got = st.mk_proof([[F(v) for v in col] for col in w], boundary)
    assert got == sc.oracle_proofs(c)[0]
    assert calls == [("mod", c.p, c.witness_wire(), c.input_wire(), 8, 8, 2, 1, 80)]
    # negative values are field(v): taken modulo p, not modulo the MiMC prime
    del calls[:]
    st.mk_proof([[v - c.p for v in col] for col in w], [(0, j, v - c.p) for j, v in enumerate(c.inputs[0])])
    assert calls == [("mod", c.p, c.witness_wire(), c.input_wire(), 8, 8, 2, 1, 80)]
    assert st.verify_proof(got, w, boundary)  # the Python mirror, modulo p
    with pytest.raises(NotImplementedError):
        st.verify_proof_native(got, w, boundary)
    # the MiMC prime keeps its own prover
    del calls[:]
    Fm = IntegersModP(sc.MIMC_P)
    mvm = multivariates_over(Fm, 2).factory
    stm = stark.STARK(Fm, 8, 8, 2, [mvm({k: Fm(v) for k, v in d.items()}) for d in sc.MIMC_2])
    stark_len = len(sc.oracle_flat(c))
    stm.mk_proof([[1] * 8, [2] * 8], [(0, 0, 1), (0, 1, 2)])
    assert calls == [("mimc", 8)]
    # not accelerated: 7 of too small an order, an even modulus, a modulus of 2^256 or more
    for p in (sc.BABYBEAR, 1 << 64, 2**256 + 297):
        Fx = IntegersModP(p)
        with pytest.raises(NotImplementedError) as e:
            stark.STARK(Fx, 8, 8, 2, [])
        assert "7" in str(e.value) or "even" in str(e.value) or "2^256" in str(e.value)
