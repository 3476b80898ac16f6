"""The STARK verifiers over any prime modulus below 2^256, CPU half: tests/native/modstark_verify_host.cpp (hipcc, host code under
AddressSanitizer and UBSan) runs the host verifier (starks_amd/csrc/modverify.hip, behind sh_mod_stark_verify) and walks the batch
verifier's item decomposition (starks_amd/csrc/modverify_items.cuh: the plan, vb_branch, mv_fri_row, mv_spot, the final-layer items)
over the same plan.  On every proof of tests/modstark_verify_cases.py both decide as the exact oracle decides
(oracle/pyoracle.verify_stark_proof with p = the modulus); the MiMC prime through the generic path equals sh_stark_verify on the golden
flat proofs; the shape verdicts with their wording; the library cross-compiles; the Python call sites.  CPU only.
What this half does NOT run: the device's index sampler (the driver samples with a serial host rewrite) and the kernels themselves:
tests/test_gpu_modstark_verify.py compares every device status with the host verifier's."""
import ctypes
import os
import struct
import subprocess

import pytest

from conftest import GOLDEN, ROOT, load_golden
import modntt_cases as mc
import modstark_cases as sc
import modstark_verify_cases as vc
from modstark_cases import HOST_GRID, MODULI
from modstark_verify_cases import INVALID, OK, REJECTED, ROOT_ORDER, UNSUPPORTED, b32
from oracle import pyoracle as po
from verify_batch_layout import flips, stark_regions

CSRC = os.path.join(ROOT, "starks_amd", "csrc")
FILES = ("mod", "proofs", "inputs", "outputs", "coefs", "exps", "counts")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msv") / "modstark_verify_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-g", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "modstark_verify_host.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _run(driver, d, files, steps, ext, width, samples, batch, timeout=600):
    """-> (the plan's code, its reason, [(host verifier's code, item walk's code)] per proof); files: name -> bytes, None = no file"""
    d.mkdir(exist_ok=True)
    for name in FILES:
        if files.get(name) is None:
            if (d / name).exists():
                (d / name).unlink()
        else:
            (d / name).write_bytes(files[name])
    out = subprocess.run([driver, str(d)] + [str(a) for a in (steps, ext, width, samples, batch)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-3000:])
    lines = out.stdout.split("\n")
    head = lines[0].split(" ", 2)
    assert head[0] == "plan" and len(lines) >= 1 + batch
    return int(head[1]), head[2] if len(head) > 2 else "", [tuple(int(x) for x in lines[1 + b].split()) for b in range(batch)]


def _files(proofs):
    P = proofs[0]
    counts, coefs, exps = P.terms()
    return {"mod": b32(P.p), "proofs": b"".join(q.flat for q in proofs), "inputs": b"".join(mc.wire(q.inputs) for q in proofs),
            "outputs": b"".join(mc.wire(q.outputs) for q in proofs), "coefs": mc.wire(coefs), "exps": exps,
            "counts": struct.pack("<%dI" % P.width, *counts)}


def _decide(driver, d, proofs):
    """the driver on Proofs -> [(host, items)]; proofs of one shape and one set of terms go in one run"""
    groups = {}
    for i, q in enumerate(proofs):
        groups.setdefault(q.shape(), []).append(i)
    got = [None] * len(proofs)
    for k, idx in enumerate(groups.values()):
        P = proofs[idx[0]]
        plan, why, res = _run(driver, d / ("g%d" % k) if len(groups) > 1 else d, _files([proofs[i] for i in idx]), P.steps, P.ext, P.width,
                              P.samples, len(idx))
        assert (plan, why) == (OK, ""), (P.id, plan, why)
        for i, r in zip(idx, res):
            got[i] = r
    return got


def _check(driver, d, proofs, want):
    """both C paths and the oracle give `want` on each proof"""
    assert [q.oracle() for q in proofs] == want, [q.id for q in proofs]
    d.mkdir(exist_ok=True)
    for q, g, w in zip(proofs, _decide(driver, d, proofs), want):
        assert g == (w, w), (q.id, g, w)


# ---- 1. the oracle's proofs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_honest_grid(driver, tmp_path, name):
    """every case of the modulus (n <= 4096): host verifier = item walk = oracle = accept"""
    cases = [c for c in HOST_GRID if c.name == name]
    assert cases
    for k, c in enumerate(cases):
        _check(driver, tmp_path / str(k), vc.honest(c), [OK] * c.batch)


def test_grid_covers_what_it_must():
    ids = {c.id for c in HOST_GRID}
    for want in vc.SINGLE_CHECK_IDS + ["bn254-s2-b1-s80", "f17-s2-b1-s80", "bn254-s8-b3-s80", "goldilocks-s32-b3-s7", "mimc-s32-b1-s80"]:
        assert want in ids, want
    assert len(sc.oracle_proofs(sc._BY_ID["bn254-s2-b1-s80"])[0][3]) == 1  # no FRI round: the final layer alone


# ---- 2. one algebraic check at a time ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", vc.SINGLE_CHECK_IDS)
def test_single_check_rejections(driver, tmp_path, cid):
    """an honest proof verified with another step-polynomial coefficient of the same degree (the transition check alone can reject), with
    input 0 off by one and with the last output off by one (the boundary check alone can reject)"""
    _check(driver, tmp_path, vc.single_check(sc._BY_ID[cid]), [OK, REJECTED, REJECTED, REJECTED])


# ---- 3. bit flips --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", vc.SINGLE_CHECK_IDS + ["bn254-s2-b1-s80"])
def test_bit_flips(driver, tmp_path, cid):
    """one single-bit flip in every region of the layout: each decision is the oracle's, and the host verifier's equals the walk's"""
    P = vc.honest(sc._BY_ID[cid])[0]
    bad = vc.region_flips(P)
    assert len(bad) >= 7
    _check(driver, tmp_path, [P] + bad, [OK] + [REJECTED] * len(bad))  # every byte of a proof is hashed or checked


# ---- 4. unreduced storage, values above the MiMC prime, inputs that are not row 0 --------------------------------------------------------
def test_values_stored_plus_p(driver, tmp_path):
    """inputs, outputs and coefficients stored as v + p are v"""
    for k, cid in enumerate(("bn254-s8-b1-s80", "goldilocks-s16x4-b1-s80", "f257-s32-b1-s80")):
        P = vc.stored_plus_p(vc.honest(sc._BY_ID[cid])[0])
        assert any(v >= P.p for v in P.inputs + P.outputs) and any(v >= P.p for v in P.terms()[1])
        _check(driver, tmp_path / str(k), [P, vc.wrong_input(P)], [OK, REJECTED])


def test_above_the_mimc_prime(driver, tmp_path):
    """opened values p - 1 >= the MiMC prime over P43: accepted over P43, rejected when the MiMC prime is given as the modulus"""
    good, as_mimc = vc.p43_const()
    assert min(sc.opened_p_values(good.flat, sc.P43_CONST)) >= sc.MIMC_P
    _check(driver, tmp_path, [good, as_mimc], [OK, REJECTED])


def test_inputs_that_are_not_row_0(driver, tmp_path):
    for k, cid in enumerate(("bn254-s8-b1-s80", "goldilocks-s16x4-b1-s80")):
        _check(driver, tmp_path / str(k), [vc.not_row0(sc._BY_ID[cid])], [REJECTED])


# ---- 5. the MiMC prime through the generic path ------------------------------------------------------------------------------------------
class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


STARK_CASES = [c for c in load_golden("stark.json") if os.path.exists(os.path.join(GOLDEN, "stark_%s.flat.bin" % c["name"]))]


def golden_mimc_cases(c, per_region=1):
    """-> (terms, [(name, flat, inputs wire, outputs wire)]): the golden flat proof, flipped copies, wrong public values"""
    from starks_amd import stark
    flat = open(os.path.join(GOLDEN, "stark_%s.flat.bin" % c["name"]), "rb").read()
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    coefs, exps, counts, _ = stark.pack_step_polys([_Poly(d) for d in sp], c["width"])
    degree = max(sum(exps[t * c["width"]:(t + 1) * c["width"]]) for t in range(len(coefs) // 32))
    regions, end = stark_regions(c["steps"], c["ext"], c["width"], degree, 80)
    assert end == len(flat)
    outs = [col[-1] for col in po.get_computational_trace(c["inputs"], c["steps"], sp)]
    inb, outb = mc.wire(c["inputs"]), mc.wire(outs)
    cases = [("untouched", flat, inb, outb)] + [(name, bad, inb, outb) for name, bad in flips(flat, regions, per_region, c["flat_len"])]
    cases.append(("wrong_output", flat, inb, mc.wire(outs[:-1] + [outs[-1] + 1])))
    cases.append(("unreduced_input", flat, mc.wire([c["inputs"][0] + sc.MIMC_P] + list(c["inputs"][1:])), outb))
    return (coefs, exps, counts), cases


@pytest.mark.parametrize("c", STARK_CASES, ids=lambda c: c["name"])
def test_mimc_prime_equals_sh_stark_verify(c):
    """sh_mod_stark_verify with modulus = the MiMC prime decides the golden flat proofs and their flipped copies as sh_stark_verify does"""
    from starks_amd import _lib
    L = _lib.lib()
    (coefs, exps, counts), cases = golden_mimc_cases(c, 2)
    want = [L.sh_stark_verify(f, len(f), i, o, c["steps"], c["ext"], c["width"], coefs, exps, counts, 80) for _, f, i, o in cases]
    got = [L.sh_mod_stark_verify(b32(sc.MIMC_P), f, len(f), i, o, c["steps"], c["ext"], c["width"], coefs, exps, counts, 80) for _, f, i, o in cases]
    assert want[0] == OK and want[-1] == OK and want.count(REJECTED) == len(cases) - 2
    assert got == want, [x[0] for x, g, w in zip(cases, got, want) if g != w]


# ---- 6. shape verdicts ---------------------------------------------------------------------------------------------------------------
def test_shape_verdicts(driver, tmp_path):
    """host verifier and plan agree on every refused shape, with the code the header gives and the plan's wording (the text the batch
    entries put behind their name in sh_last_error)"""
    P = vc.honest(sc._BY_ID["bn254-s8-b1-s80"])[0]
    base = _files([P])
    k = [0]

    def verdict(steps=8, ext=8, width=2, samples=80, timeout=600, **files):
        k[0] += 1
        f = dict(base)
        f.update(files)
        plan, why, got = _run(driver, tmp_path / str(k[0]), f, steps, ext, width, samples, 1, timeout)
        return (plan, got[0][0], got[0][1]), why

    assert verdict() == ((OK, OK, OK), "")
    # null pointers: the plan reads the modulus and the term description, the verifiers every buffer
    for name in ("mod", "exps", "counts"):
        assert verdict(**{name: None}) == ((INVALID,) * 3, "null pointer"), name
    for name in ("proofs", "inputs", "outputs", "coefs"):
        assert verdict(**{name: None}) == ((OK, INVALID, INVALID), ""), name
    for bad in (P.p - 1, 1 << 255, 0, 1, 2):  # even, 0, 1
        assert verdict(mod=b32(bad)) == ((INVALID,) * 3, "the modulus must be odd and at least 3"), bad
    one = {"inputs": bytes(32), "outputs": bytes(32)}
    assert verdict(width=0, **one) == ((INVALID,) * 3, "width and samples must be at least 1")
    assert verdict(samples=0) == ((INVALID,) * 3, "width and samples must be at least 1")
    for steps, ext in ((12, 8), (8, 12), (1, 8), (8, 1), (0, 8), (8, 0)):
        assert verdict(steps=steps, ext=ext) == ((INVALID,) * 3, "steps and ext must be powers of two and at least 2"), (steps, ext)
    for steps, ext in ((1 << 12, 1 << 12), (1 << 24, 2), (2, 1 << 24), (1 << 40, 1 << 24)):
        assert verdict(steps=steps, ext=ext) == ((INVALID,) * 3, "steps * ext must be below 2^24 (utils.py:69)"), (steps, ext)
    wide = {"inputs": bytes(320), "outputs": bytes(320)}
    assert verdict(width=10, **wide) == ((UNSUPPORTED,) * 3, "width is limited to 9 (stark.py:106-126)")
    many = "more step-polynomial terms than SHK_STARK_MAX_TERMS (256)"
    assert verdict(counts=struct.pack("<2I", 257, 1)) == ((UNSUPPORTED,) * 3, many)
    assert verdict(counts=struct.pack("<2I", 200, 57)) == ((UNSUPPORTED,) * 3, many)
    assert verdict(counts=struct.pack("<2I", 0, 0), coefs=b"", exps=b"") == ((INVALID,) * 3, "the step polynomials have no terms")
    # G2 = 7^((p - 1) // 64) of the wrong order: 7 is a quadratic residue modulo BabyBear; 17 - 1 has too few factors of two
    order = "G2 = 7^((p - 1) // (steps * ext)) does not have order steps * ext modulo p (G2^(n/2) != -1)"
    assert verdict(mod=b32(sc.BABYBEAR)) == ((ROOT_ORDER,) * 3, order)
    assert verdict(mod=b32(17)) == ((ROOT_ORDER,) * 3, order)
    # a FRI shape the FRI verifier calls invalid: steps * degree = 2040 coefficients on 256 points leave the fourth round 4 points
    big = {"exps": bytes([1, 0, 1, 0, 0, 255]), "coefs": base["coefs"]}
    assert verdict(steps=8, ext=32, **big) == ((INVALID,) * 3, "a round with fewer than 16 points (maxdeg_plus_1 is too large for n)")
    # the length: the plan takes the shape, the batch form answers SH_ERR_INVALID for the mismatch as the host verifier does
    assert verdict(proofs=P.flat[:-32]) == ((OK, INVALID, INVALID), "")
    assert verdict(proofs=P.flat + bytes(32)) == ((OK, INVALID, INVALID), "")
    assert verdict(proofs=P.flat[:64]) == ((OK, INVALID, INVALID), "")
    # a hostile sample count on a 100-byte buffer: refused before anything is derived from it (the sampling would hash 16 GiB); the
    # plan refuses index sets of 2^32 entries or more
    assert verdict(proofs=bytes(100), samples=2**32 - 1, timeout=10) == ((UNSUPPORTED, INVALID, UNSUPPORTED),
                                                                        "more sampled rows per proof than the index sets hold (2^32)")
    Q = vc.honest(sc._BY_ID["bn254-s2-b1-s80"])[0]  # no round: the spot set alone
    assert _run(driver, tmp_path / "s2", dict(_files([Q]), proofs=bytes(100)), 2, 8, 1, 2**32 - 1, 1, 10)[::2] == (OK, [(INVALID, INVALID)])
    from starks_amd import _lib
    L = _lib.lib()
    counts, coefs, exps = P.terms()
    cn = (ctypes.c_uint32 * 2)(*counts)
    args = (mc.wire(P.inputs), mc.wire(P.outputs), 8, 8, 2, mc.wire(coefs), exps, cn)
    assert L.sh_mod_stark_verify(b32(P.p), bytes(100), 100, *args, 2**32 - 1) == INVALID
    assert L.sh_mod_stark_verify(b32(P.p), P.flat, len(P.flat), *args, 80) == OK
    assert L.sh_mod_stark_verify(b32(P.p), P.flat, len(P.flat) - 32, *args, 80) == INVALID
    assert L.sh_mod_stark_verify(b32(P.p), None, 0, *args, 80) == INVALID
    assert L.sh_mod_stark_verify(None, P.flat, len(P.flat), *args, 80) == INVALID


# ---- 7. build and mirrors ------------------------------------------------------------------------------------------------------------
def test_library_cross_compiles():
    """the translation units of the verifiers for gfx950, and the symbols the header declares in the built library"""
    for src in ("modverify.hip", "modverify_dev.hip", "api_modverify.hip", "api_modstark.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("sh_mod_stark_verify", "sh_dev_mod_stark_verify", "sh_mod_stark_verify_batch"):
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header
    assert "There is no C verifier of these proofs" not in header


def _stark_of(c):
    from starks_amd import IntegersModP, stark
    from starks_amd.multivariate_polynomial import multivariates_over
    F = IntegersModP(c.p)
    mv = multivariates_over(F, c.width).factory
    st = stark.STARK(F, c.steps, c.ext, c.width, [mv({k: F(v) for k, v in d.items()}) for d in c.sp], c.samples)
    return st, c.witnesses()[0], [(0, j, F(v)) for j, v in enumerate(c.inputs[0])]


@pytest.mark.parametrize("cid", ["bn254-s8-b1-s80", "goldilocks-s16x4-b1-s80", "mimc-s8-b1-s80"])
def test_python_call_sites(monkeypatch, cid):
    """without a device: STARK.verify_proof_mod_native accepts the oracle's proof over the STARK's own modulus (the MiMC prime included)
    and raises AssertionError on a tampered one; verify_proof_native still refuses other moduli"""
    from starks_amd import _lib, stark
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("the host verifier must not ask for a context"))
    c = sc._BY_ID[cid]
    st, w, boundary = _stark_of(c)
    proof = sc.oracle_proofs(c)[0]
    assert st.verify_proof_mod_native(proof, w, boundary) is True
    tampered = [proof[0], proof[1], [list(b) for b in proof[2]], proof[3]]
    tampered[2][4][1] = bytes(len(tampered[2][4][1]))
    with pytest.raises(AssertionError):
        st.verify_proof_mod_native(tampered, w, boundary)
    with pytest.raises(AssertionError):
        st.verify_proof_mod_native(proof, w, [(0, 0, int(boundary[0][2]) + 1)] + boundary[1:])
    P = vc.honest(c)[0]
    assert stark.mod_verify_flat(c.p, P.flat, mc.wire(P.inputs), mc.wire(P.outputs), c.steps, c.ext, c.width, st.step_polys, c.samples) is True
    if c.p != sc.MIMC_P:
        with pytest.raises(NotImplementedError):
            st.verify_proof_native(proof, w, boundary)
    else:
        assert st.verify_proof_native(proof, w, boundary) is True
