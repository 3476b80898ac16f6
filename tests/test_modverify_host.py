"""The FRI verifiers over any odd modulus below 2^256, CPU half: tests/native/modverify_host.cpp (hipcc, host code under
AddressSanitizer and UBSan) runs the host verifier (starks_amd/csrc/modverify.hip, behind sh_mod_fri_verify) and walks the batch
verifier's item decomposition (starks_amd/csrc/modverify_items.cuh) over the same plan.  On honest proofs of every modulus of
tests/modfri_cases.py, on single-bit flips in every region of the layout and on proofs that only one algebraic check can reject, both
decide as the exact oracle decides (oracle/pyoracle.verify_low_degree_proof with p = the modulus); the shape verdicts; the library
cross-compiles; the Python call sites.  CPU only.
What this half does NOT run: the device's index sampler (the driver samples with a serial host rewrite) and the kernels themselves:
tests/test_gpu_modverify.py compares every device status with the host verifier's."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
import modfri_cases as fc
import modverify_cases as vc
from modfri_cases import HOST_GRID, MODULI, root_of
from modverify_cases import INVALID, OK, REJECTED, ROOT_ORDER, UNSUPPORTED, b32
from verify_batch_layout import flips, fri_regions

CSRC = os.path.join(ROOT, "starks_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mv") / "modverify_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-g", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "native", "modverify_host.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _run(driver, d, files, n, md, exclude, samples, batch, timeout=600):
    """-> (the plan's code, [(host verifier's code, item walk's code)] per proof); files: name -> bytes, None = no file (a null pointer)"""
    d.mkdir(exist_ok=True)
    for name in ("mod", "root", "proofs", "roots"):
        if files.get(name) is None:
            if (d / name).exists():
                (d / name).unlink()
        else:
            (d / name).write_bytes(files[name])
    out = subprocess.run([driver, str(d)] + [str(a) for a in (n, md, exclude, samples, batch)], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-3000:])
    lines = out.stdout.split()
    assert lines[0] == "plan" and len(lines) == 2 + 2 * batch
    return int(lines[1]), [(int(lines[2 + 2 * b]), int(lines[3 + 2 * b])) for b in range(batch)]


def _decide(driver, d, proofs):
    """the driver on Proofs of one shape and modulus -> [(host, items)]"""
    P = proofs[0]
    assert all((q.p, q.n, q.md, q.exclude, q.samples, len(q.flat)) == (P.p, P.n, P.md, P.exclude, P.samples, len(P.flat)) for q in proofs)
    plan, got = _run(driver, d, {"mod": b32(P.p), "root": b32(P.root), "proofs": b"".join(q.flat for q in proofs),
                                 "roots": b"".join(q.merkle_root for q in proofs)}, P.n, P.md, P.exclude, P.samples, len(proofs))
    assert plan == OK
    return got


# ---- 1. honest proofs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_honest_grid(driver, tmp_path, name):
    """every verifiable case of the modulus: host verifier = item walk = oracle = accept"""
    cases = [c for c in HOST_GRID if c.name == name and c.verify and c.n >= 4]
    assert cases
    for k, c in enumerate(cases):
        proofs = vc.honest(c)
        assert _decide(driver, tmp_path / str(k), proofs) == [(OK, OK)] * c.batch, c.id
        assert [P.oracle() for P in proofs] == [OK] * c.batch, c.id


def test_honest_grid_covers_what_it_must():
    ids = {c.id for c in HOST_GRID if c.verify and c.n >= 4}
    for want in ("p43-n64-md32-c1-x0-s40-b1-const", "c2-n256-md128-c128-x0-s40-b1", "f65537-n1024-md256-c256-x8-s40-b1",
                 "bls12_381-n1024-md256-c256-x0-s40-b3", "bn254-n256-md128-c100-x0-s7-b1", "goldilocks-n256-md64-c64-x0-s80-b1"):
        assert want in ids, want
    assert fc.P43 - 1 >= fc.MIMC_P


def test_two_rounds_of_80_and_40_samples(driver, tmp_path):
    """the prover gives the first round `samples` and later rounds 40; the reference's verifier asks every round for `samples` and cannot
    take such a proof (verify=False in the grid).  Both C paths follow the prover and accept it."""
    c = fc._BY_ID["goldilocks-n256-md128-c128-x0-s80-b1"]
    assert not c.verify and c.rounds() == 2
    assert _decide(driver, tmp_path, vc.honest(c)) == [(OK, OK)]


# ---- 2. bit flips --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["bn254-n64-md32-c32-x0-s40-b1", "c2-n256-md128-c128-x0-s40-b1", "f65537-n1024-md256-c256-x8-s40-b1",
                                 "p43-n64-md32-c1-x0-s40-b1-const"])
def test_bit_flips(driver, tmp_path, cid):
    """two single-bit flips in every region of the layout: each decision is the oracle's, and the host verifier's equals the walk's"""
    c = fc._BY_ID[cid]
    P = vc.honest(c)[0]
    regions, end = fri_regions(c.n, c.md, c.samples)
    assert end == len(P.flat)
    bad = [P.with_flat(flat, "-" + name) for name, flat in flips(P.flat, regions, 2, c.n + c.md)]
    want = [q.oracle() for q in [P] + bad]
    assert want == [OK] + [REJECTED] * len(bad)  # every byte of a proof is hashed
    got = _decide(driver, tmp_path, [P] + bad)
    for q, g, w in zip([P] + bad, got, want):
        assert g == (w, w), (q.id, g, w)


# ---- 3. the degree bound alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vc.DEGREE_SHAPES, ids=lambda s: "%s-%d-%d-x%d" % s)
def test_degree_bound_alone_rejects(driver, tmp_path, shape):
    """md + 1 coefficients committed honestly: every branch and row passes, only the final layer's check fails (the composite c2
    included, where a Fermat inversion of the denominators would decide at random)"""
    lo, hi = vc.degree_pair(*shape)
    assert (lo.oracle(), hi.oracle()) == (OK, REJECTED)
    assert _decide(driver, tmp_path, [lo, hi]) == [(OK, OK), (REJECTED, REJECTED)]


# ---- 4. the row check alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vc.FOLD_SHAPES, ids=lambda s: "%s-%d-%d-x%d" % s)
def test_row_check_alone_rejects(driver, tmp_path, shape):
    """the first column folded at special_x + nudge: nudge 1 is rejected by the rows alone, nudges 0 and p are the honest proof (the
    challenge is used modulo p)"""
    proofs = [vc.wrong_fold(*shape, nudge) for nudge in (0, 1, MODULI[shape[0]])]
    want = [OK, REJECTED, OK]
    assert [P.oracle() for P in proofs] == want
    assert _decide(driver, tmp_path, proofs) == [(w, w) for w in want]


# ---- 5. unreduced bytes --------------------------------------------------------------------------------------------------------------
def test_unreduced_values(driver, tmp_path):
    """final-layer values stored as v + p are v; one of them off by 1 breaks the degree bound"""
    good, bad = vc.unreduced(0), vc.unreduced(1)
    assert (good.oracle(), bad.oracle()) == (OK, REJECTED)
    assert _decide(driver, tmp_path, [good, bad]) == [(OK, OK), (REJECTED, REJECTED)]


# ---- 6. shape verdicts ---------------------------------------------------------------------------------------------------------------
def test_shape_verdicts(driver, tmp_path):
    """host verifier and plan agree on every refused shape, with the code the header gives"""
    P = vc.honest(fc._BY_ID["bn254-n64-md32-c32-x0-s40-b1"])[0]
    p, w = P.p, P.root
    k = [0]

    def verdict(mod=b32(p), root=b32(w), proofs=P.flat, roots=P.merkle_root, n=64, md=32, exclude=0, samples=40, timeout=600):
        k[0] += 1
        plan, got = _run(driver, tmp_path / str(k[0]), {"mod": mod, "root": root, "proofs": proofs, "roots": roots}, n, md, exclude, samples, 1,
                         timeout)
        return plan, got[0][0], got[0][1]

    assert verdict() == (OK, OK, OK)
    for bad in (p - 1, 1 << 255, 0, 1, 2):  # even, 0, 1
        assert verdict(mod=b32(bad)) == (INVALID, INVALID, INVALID), bad
    assert verdict(root=b32(p + w)) == (ROOT_ORDER,) * 3                       # a root at or above p
    assert verdict(root=b32(p)) == (ROOT_ORDER,) * 3
    assert verdict(root=b32(root_of("bn254", 32))) == (ROOT_ORDER,) * 3       # a root of order n / 2
    assert verdict(root=b32(root_of("bn254", 128))) == (ROOT_ORDER,) * 3
    assert verdict(n=12) == (INVALID,) * 3
    assert verdict(n=2, root=b32(p - 1)) == (INVALID,) * 3
    assert verdict(samples=0) == (INVALID,) * 3
    assert verdict(exclude=1) == (INVALID,) * 3
    assert verdict(n=8, root=b32(root_of("bn254", 8)), md=32) == (INVALID,) * 3  # a round below 16 points
    assert verdict(md=1 << 10) == (INVALID,) * 3                                # the third round would have 4 points
    assert verdict(n=1 << 27, root=b32(root_of("bn254", 1 << 27)), md=16) == (UNSUPPORTED,) * 3
    # n = 2^26: without a round the plan takes the shape (its final layer is over the batch cap); with a round the column has 2^24 rows,
    # which the sampler refuses (utils.py:69): SH_ERR_INVALID from both, on a short buffer and on one of the shape's full length
    w26 = b32(root_of("bn254", 1 << 26))
    assert verdict(n=1 << 26, root=w26, md=16)[0] == UNSUPPORTED
    assert verdict(n=1 << 26, root=w26, md=32) == (INVALID,) * 3
    full = sum(32 + 40 * 32 * ((lg - 1) + 4 * (lg + 1)) for lg in range(26, 6, -2)) + 32 * 64  # ten rounds, a final layer of 64
    assert full == 1128768
    assert verdict(n=1 << 26, root=w26, md=1 << 24, proofs=bytes(full)) == (INVALID,) * 3
    w24 = b32(root_of("bn254", 1 << 24))
    assert verdict(n=1 << 24, root=w24, md=1 << 22, proofs=bytes(1024))[0] == OK  # the largest domain with rounds
    # the length: the plan takes the shape, the batch form answers SH_ERR_INVALID for the mismatch as the host verifier does
    assert verdict(proofs=P.flat + bytes(32)) == (OK, INVALID, INVALID)
    assert verdict(proofs=P.flat[:-32]) == (OK, INVALID, INVALID)
    # a batch final layer of 2^11 points: the host verifier takes it, the batch forms do not
    top = vc.from_coeffs("bn254", 2048, 16, (3, 1, 4))
    assert verdict(root=b32(top.root), proofs=top.flat, roots=top.merkle_root, n=2048, md=16) == (UNSUPPORTED, OK, UNSUPPORTED)
    at_cap = vc.from_coeffs("bn254", 1024, 16, (3, 1, 4))
    assert verdict(root=b32(at_cap.root), proofs=at_cap.flat, roots=at_cap.merkle_root, n=1024, md=16) == (OK, OK, OK)
    # null pointers
    assert verdict(mod=None) == (INVALID,) * 3
    assert verdict(root=None) == (INVALID,) * 3
    assert verdict(proofs=None) == (OK, INVALID, INVALID)
    assert verdict(roots=None) == (OK, INVALID, INVALID)
    # a hostile sample count on a 100-byte buffer: refused before anything is derived from it (the sampling would hash 16 GiB)
    assert verdict(proofs=bytes(100), samples=2**32 - 1, timeout=10) == (OK, INVALID, INVALID)
    from starks_amd import _lib
    L = _lib.lib()
    assert L.sh_mod_fri_verify(b32(p), bytes(100), 100, P.merkle_root, 64, b32(w), 32, 0, 2**32 - 1) == INVALID
    assert L.sh_mod_fri_verify(b32(p), P.flat, len(P.flat), P.merkle_root, 64, b32(w), 32, 0, 40) == OK
    assert L.sh_mod_fri_verify(b32(p), None, 0, P.merkle_root, 64, b32(w), 32, 0, 40) == INVALID


# ---- 7. build and mirrors ------------------------------------------------------------------------------------------------------------
def test_library_cross_compiles():
    """the new translation units for gfx950, and the symbols the header declares in the built library"""
    for src in ("modverify.hip", "modverify_dev.hip", "api_modverify.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=600)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("sh_mod_fri_verify", "sh_dev_mod_fri_verify", "sh_mod_fri_verify_batch"):
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header
    assert "OUT OF SCOPE: the C and GPU verifiers" not in header


def test_library_host_verifier_is_the_driver_s():
    """sh_mod_fri_verify in the built library (no context, no GPU) decides the hand-made proofs as the oracle does"""
    from starks_amd import _lib, fri
    L = _lib.lib()
    lo, hi = vc.degree_pair("c2", 64, 32, 0)
    for P, want in ((lo, OK), (hi, REJECTED), (vc.wrong_fold("c2", 256, 128, 0, 1), REJECTED), (vc.unreduced(0), OK), (vc.unreduced(1), REJECTED)):
        assert L.sh_mod_fri_verify(b32(P.p), P.flat, len(P.flat), P.merkle_root, P.n, b32(P.root), P.md, P.exclude, P.samples) == want, P.id
        if want == OK:
            assert fri.mod_verify_flat(P.p, P.flat, P.merkle_root, P.n, P.root, P.md, P.exclude, P.samples) is True
        else:
            with pytest.raises(AssertionError):
                fri.mod_verify_flat(P.p, P.flat, P.merkle_root, P.n, P.root, P.md, P.exclude, P.samples)


def test_native_verifier_routes_by_modulus(monkeypatch):
    """without a device: verify_proximity_proof_native sends the MiMC prime to verify_flat and any other odd modulus to mod_verify_flat
    with its modulus; an even modulus and a root whose order is no power of two raise NotImplementedError"""
    from starks_amd import IntegersModP, _lib, fri
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("routing must not ask for a context"))
    calls = []
    monkeypatch.setattr(fri, "mod_verify_flat", lambda modulus, flat, mroot, n, w, md, ex=0, sm=40: calls.append(("mod", modulus, n, int(w), md, ex, sm)) or True)
    monkeypatch.setattr(fri, "verify_flat", lambda flat, mroot, n, w, md, ex=0, sm=40: calls.append(("mimc", n, md, ex, sm)) or True)
    c = fc._BY_ID["bn254-n64-md32-c32-x0-s40-b1"]
    F = IntegersModP(c.p)
    proof = fc.oracle_proofs(c)[0]
    assert fri.SmoothSubgroupFRI(F).verify_proximity_proof_native(proof, fc.merkle_root(c), F(c.root), c.md, 0, 40)
    assert calls == [("mod", c.p, 64, c.root, 32, 0, 40)]
    del calls[:]
    Fm = IntegersModP(fc.MIMC_P)
    wm = root_of("mimc", 64)
    assert fri.SmoothSubgroupFRI(Fm).verify_proximity_proof_native(proof, fc.merkle_root(c), Fm(wm), 32, 8, 40)
    assert calls == [("mimc", 64, 32, 8, 40)]
    del calls[:]
    with pytest.raises(NotImplementedError):
        fri.SmoothSubgroupFRI(IntegersModP(1 << 64)).verify_proximity_proof_native(proof, fc.merkle_root(c), 3, 32)
    F31 = IntegersModP(31)
    with pytest.raises(NotImplementedError):
        fri.SmoothSubgroupFRI(F31).verify_proximity_proof_native(proof, fc.merkle_root(c), F31(15), 32)
    assert calls == []


def test_python_verifier_over_the_composite_modulus():
    """starks_amd.fri.verify_low_degree_proof (pure Python) inverts with pow(den, -1, p): it accepts the honest c2 proofs, where
    den^(p-2) is no inverse, and rejects the degree-too-high one"""
    from starks_amd import fri
    for c in [c for c in HOST_GRID if c.name == "c2" and c.verify and c.n >= 4]:
        for P in vc.honest(c):
            assert fri.verify_low_degree_proof(vc.unpack(P.flat, P.n, P.md), P.merkle_root, P.root, P.md, P.exclude, P.samples, modulus=P.p), c.id
    lo, hi = vc.degree_pair("c2", 64, 32, 0)
    assert fri.verify_low_degree_proof(vc.unpack(lo.flat, 64, 32), lo.merkle_root, lo.root, 32, modulus=lo.p)
    with pytest.raises(AssertionError):
        fri.verify_low_degree_proof(vc.unpack(hi.flat, 64, 32), hi.merkle_root, hi.root, 32, modulus=hi.p)
