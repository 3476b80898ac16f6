"""The packed-word STARK prover's CPU half: tests/native/mod64stark_host.cpp (hipcc, host code under AddressSanitizer and UBSan) walks
the prover exactly as starks_amd/csrc/api_mod64stark.hip issues it -- the transforms through ntt64_items.cuh, the items of
mod64stark_items.cuh over the grids mod64stark.hip launches, the trees and commit rounds through mod64fri_items.cuh -- and every case of
tests/mod64stark_cases.py equals the exact oracle (oracle/pyoracle.py with p = the modulus) byte for byte; the oracle's verifier accepts
each proof; the top-bit case; the broken witnesses flag; the batch inversion against pow(v, -1, p); the refusals; the library
cross-compiles.  CPU only.
What this half does NOT run: the index sampler (a device-only kernel of the MiMC path: the driver samples with its own host copy of
utils.py's get_pseudorandom_indices) and the host checks of api_mod64stark.hip, which need the HIP runtime; both are covered by
tests/test_gpu_mod64stark.py."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
import mod64stark_cases as m6
import ntt64_cases as nc
from mod64stark_cases import HOST_GRID, MODULI
from oracle import pyoracle

CSRC = os.path.join(ROOT, "starks_amd", "csrc")
SYMBOLS = ("sh_mod64_stark_prove", "sh_dev_mod64_stark_prove")
CHUNK = 16  # mod64stark_items.cuh: M6S_INV_CHUNK


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("m6s") / "mod64stark_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-g", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "mod64stark_host.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, args, **files):
    for name, data in files.items():
        (d / name).write_bytes(data)
    return subprocess.run([driver, args[0], str(d)] + [str(a) for a in args[1:]], capture_output=True, text=True, timeout=600)


def _prove(driver, d, name, cases, tile_log=12, witnesses=None):
    """-> ([flat proofs of each case], [flags of each case]) from one run of the driver; all cases over MODULI[name]"""
    blob, lines = b"", []
    for c in cases:
        lines.append("%d %d %d %d %d %d" % (c.steps, c.ext, c.width, c.samples, c.batch, tile_log))
        blob += c.blob(witnesses)
    out = _call(driver, d, ["prove", MODULI[name]], cases=("\n".join(lines) + "\n").encode(), **{"in": blob})
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    raw, flags, res, fl, k, j = (d / "out").read_bytes(), (d / "flags").read_bytes(), [], [], 0, 0
    for c in cases:
        ln = m6.proof_len(c) * c.batch
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
        assert got == m6.oracle_flat(c), c.id
        assert fl == [0] * c.batch, c.id
        for b, proof in enumerate(m6.oracle_proofs(c)):
            assert m6.oracle_verify(c, proof, b), c.id


def test_grid_covers_what_it_must():
    """a guard on the case table itself (tests/mod64stark_cases.py), not on the code: it keeps a later edit from dropping a case"""
    ids = [c.id for c in m6.GRID]
    assert len(set(ids)) == len(ids) and HOST_GRID == m6.GRID
    assert set(MODULI) == {"goldilocks", "big18", "f65537", "f257", "f17"}
    have = {(c.name, c.steps, c.ext, c.width, c.degree) for c in m6.GRID if c.batch == 1 and c.samples == 80 and not c.plus_p}
    for name in MODULI:
        assert (name, 2, 8, 1, 1) in have
        if name != "f17":
            for shape in ((8, 8, 2, 3), (16, 4, 1, 3), (32, 8, 3, 3), (8, 8, 9, 5)):  # widths 1, 2, 3 and 9
                assert (name,) + shape in have, (name, shape)
    assert [c.shape for c in m6.GRID if c.name == "f17"] == ["s2"]
    assert any(c.name == "f257" and c.n == 257 - 1 for c in m6.GRID)  # the domain is the whole group
    assert MODULI["big18"] > 2**63 and MODULI["goldilocks"] > 2**63  # sums carry out of 64 bits
    assert any(c.name == "goldilocks" and c.shape == "s32" and c.batch == 3 and c.samples == 7 for c in m6.GRID)
    assert any(c.name == "big18" and c.shape == "s8" and c.batch == 3 for c in m6.GRID)
    assert {c.name for c in m6.GRID if c.sp is m6.ZERO_2} == {"f65537", "big18"}
    plus = [c for c in m6.GRID if c.plus_p]
    assert {c.name for c in plus} == {"goldilocks", "big18", "f257", "f65537"}
    for c in plus:  # stored values at or above p, in the witness, the inputs and the coefficients
        assert any(v >= c.p for v in nc.ints(c.witness_words())) and any(v >= c.p for v in nc.ints(c.input_words())), c.id
        assert any(v >= c.p for v in c.terms()[1]), c.id
        assert nc.ints(c.witness_words()) != [v % c.p for v in nc.ints(c.witness_words())]
    for name in ("goldilocks", "big18"):  # only some words fit there
        c = [x for x in plus if x.name == name][0]
        w = nc.ints(c.witness_words())
        assert any(i % 5 == 2 and v < c.p for i, v in enumerate(w)), name
    # zero, one and two commit rounds
    assert {0, 1, 2} <= {len(m6.oracle_proofs(c)[0][3]) - 1 for c in m6.GRID if c.name == "big18"}
    b = m6.BIG18_CONST
    assert b.inputs == [[m6.BIG18 - 1]] and (b.steps, b.ext) == (16, 8) and b.sp is m6.CUBE_1
    units, flags = m6.broken_witnesses()
    assert m6.BREAK_BASE.name == "goldilocks" and len(units) == 1 + m6.BREAK_BASE.width * m6.BREAK_BASE.steps == 17
    assert flags == [0] + [1] * 16
    for c in m6.GRID + [b, m6.BREAK_BASE]:  # G2 has full order over every case of the grid
        assert pow(pow(7, (c.p - 1) // c.n, c.p), c.n // 2, c.p) == c.p - 1, c.id
    for p, n in ((m6.BABYBEAR, 64), (m6.KOALABEAR, 64), (3, 16), (m6.P64_59, 16), (m6.BIG18, 1 << 19)):  # and not over these
        assert pow(pow(7, (p - 1) // n, p), n // 2, p) != p - 1, (p, n)
    # the flat lengths recorded for BIG18 over the five shapes
    assert [m6.proof_len(c) for c in m6.GRID if c.name == "big18" and c.batch == 1 and not c.plus_p and c.shape in m6.SHAPES] == \
        [{"s2": 59456, "s8": 147808, "s16x4": 117088, "s32": 248960, "s8w9": 362848}[s] for s in m6.SHAPES]


def test_top_bit(driver, tmp_path):
    """X' = X^3 from p - 1 over BIG18: the whole trace is p - 1 > 2^63, and every P value in every opened leaf appears as p - 1"""
    c = m6.BIG18_CONST
    assert c.witnesses() == [[[m6.BIG18 - 1] * 16]]
    (got,), (fl,) = _prove(driver, tmp_path, "big18", [c])
    assert got == m6.oracle_flat(c) and fl == [0]
    opened = m6.opened_p_values(got, c)
    assert len(opened) == 4 * c.samples and set(opened) == {m6.BIG18 - 1} and all(v >> 63 for v in opened)
    assert m6.oracle_verify(c, m6.oracle_proofs(c)[0])


def test_broken_witnesses(driver, tmp_path):
    """every single-element break of one small witness in one batch: exactly the broken proofs flag, the valid one keeps its bytes"""
    batch, units, want = m6.break_batch()
    base = m6.BREAK_BASE
    out = _call(driver, tmp_path, ["prove", base.p], cases=b"%d %d %d %d %d 12\n" % (base.steps, base.ext, base.width, 80, len(units)),
                **{"in": batch.blob(units)})
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    assert list((tmp_path / "flags").read_bytes()) == want
    ln = m6.proof_len(base)
    assert (tmp_path / "out").read_bytes()[:ln] == m6.oracle_flat(base)
    with pytest.raises(AssertionError):  # the reference's `assert cp % z == 0` (stark.py:76)
        pyoracle.mk_stark_proof(units[1], base.inputs[0], base.sp, base.steps, base.ext, p=base.p)


@pytest.mark.parametrize("tile_log", [3, 5])
def test_forced_transform_plans(driver, tmp_path, tile_log):
    """the same proofs when the transforms run as several passes"""
    cases = [c for c in HOST_GRID if c.name == "big18" and c.shape in ("s8", "s32") and not c.plus_p and c.batch == 1]
    assert len(cases) == 2
    proofs, _ = _prove(driver, tmp_path, "big18", cases, tile_log)
    for c, got in zip(cases, proofs):
        assert got == m6.oracle_flat(c), c.id


def test_refusals(driver, tmp_path):
    """the driver's restatement of the host checks: an even modulus and one below 3, the moduli over which G2 lacks full order, a cubic
    at ext 2"""
    c = [x for x in HOST_GRID if x.name == "goldilocks" and x.shape == "s16x4"][0]
    line = b"%d %d %d %d %d 12\n" % (c.steps, c.ext, c.width, c.samples, c.batch)
    for p in (1 << 32, 1, 0):
        assert _call(driver, tmp_path, ["prove", p], cases=line, **{"in": c.blob()}).returncode == 2
    for p in (m6.BABYBEAR, m6.KOALABEAR, 3, m6.P64_59):
        assert _call(driver, tmp_path, ["prove", p], cases=line, **{"in": c.blob()}).returncode == 3, p
    assert _call(driver, tmp_path, ["prove", c.p], cases=b"16 2 1 80 1 12\n", **{"in": c.blob()}).returncode == 4
    s2 = [x for x in HOST_GRID if x.name == "f17" and x.shape == "s2"][0]
    assert _call(driver, tmp_path, ["prove", m6.P64_59], cases=b"2 8 1 80 1 12\n", **{"in": s2.blob()}).returncode == 3  # n = 16 > 4


# ---- the batch inversion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
@pytest.mark.parametrize("count", [1, CHUNK - 1, CHUNK, CHUNK + 1, 100])
def test_batch_inversion(driver, tmp_path, name, count):
    """m6s_batch_inv_item against pow(v, -1, p): zeros map to zero, counts around the chunk boundary (16 values per item: at 17 item 0
    owns two values and item 1 one)"""
    p = MODULI[name]
    vals = [v % p for v in nc.inputs(count, count, p)]
    vals[0] = 0
    if count > 40:
        vals[40] = p - 1
        vals[3] = vals[7] = 0
    out = _call(driver, tmp_path, ["inv", p], values=nc.words(vals))
    assert out.returncode == 0, out.stderr[-3000:]
    assert nc.ints((tmp_path / "out").read_bytes()) == [pow(v, -1, p) if v else 0 for v in vals]


def test_chunk_constant():
    text = open(os.path.join(CSRC, "mod64stark_items.cuh")).read()
    assert "constexpr uint32_t M6S_INV_CHUNK = %d;" % CHUNK in text


# ---- the library and the Python call sites -------------------------------------------------------------------------------------------
def test_library_cross_compiles():
    """the two new translation units for gfx950, and the symbols the header declares in the built library"""
    for src in ("mod64stark.hip", "api_mod64stark.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header


def test_python_length_checks(monkeypatch):
    """without a device: mod64_prove_flat and mod64_prove_inputs_flat refuse buffers of the wrong length before asking for a context"""
    from starks_amd import IntegersModP, _lib, stark
    from starks_amd.multivariate_polynomial import multivariates_over
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("a length error must not ask for a context"))
    F = IntegersModP(m6.GOLDILOCKS)
    mv = multivariates_over(F, 2).factory
    sp = [mv({k: F(v) for k, v in d.items()}) for d in m6.MIMC_2]
    with pytest.raises(ValueError):
        stark.mod64_prove_flat(m6.GOLDILOCKS, [1] * 15, [1, 2], 8, 8, 2, sp)
    with pytest.raises(ValueError):
        stark.mod64_prove_flat(m6.GOLDILOCKS, [1] * 16, [1, 2, 3], 8, 8, 2, sp)
    with pytest.raises(ValueError):
        stark.mod64_prove_inputs_flat(m6.GOLDILOCKS, bytes(63), 8, 8, 2, sp)
