"""STARK proofs over any prime modulus below 2^256 (sh_mod_stark_prove, sh_dev_mod_stark_prove: starks_amd/csrc/modstark_items.cuh,
modstark.hip, api_modstark.hip) on the MI355X: the whole grid of tests/modstark_cases.py against the exact oracle (oracle/pyoracle.py
with p = the modulus) and tests/golden/mod_stark.json (the live reference's STARK over IntegersModP(p)), byte for byte; the device form
and its per-proof flags; the Python call sites; the tuned MiMC prover as yardstick through the generic entry; sizes the coefficient
oracle does not reach, checked by the two verifiers; interleaved calls; the errors.  Every refused call is refused on the host."""
import ctypes
import hashlib
import random
import struct

import pytest

from conftest import load_golden
import modntt_cases as mc
import modstark_cases as sc
from modstark_cases import MODULI
from modntt_cases import wire
from oracle import pyoracle

pytestmark = pytest.mark.gpu

OK, INVALID, ROOT_ORDER, TOO_SMALL, UNSUPPORTED, CONSTRAINT = 0, -1, -2, -5, -6, -8


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


def term_args(sp, p):
    """step polynomials as {exponent tuple: coefficient} per dimension -> (coefs, exps, counts) as the C entry takes them"""
    counts, coefs, exps = [], [], bytearray()
    for poly in sp:
        items = sorted(poly.items())
        counts.append(len(items))
        for k, c in items:
            coefs.append(c % p)
            exps += bytes(k)
    return wire(coefs), bytes(exps), (ctypes.c_uint32 * len(sp))(*counts)


def prove_raw(L, p, wit, inp, steps, ext, sp, samples=80, batch=1, terms=None):
    width = len(sp)
    coefs, exps, counts = terms or term_args(sp, p)
    plen = L.sh_stark_proof_len(steps, ext, width, sc.degree_of(sp), samples)
    assert plen
    out = ctypes.create_string_buffer(plen * batch)
    rc = L.sh_mod_stark_prove(_ctx(), b32(p), wit, inp, steps, ext, width, coefs, exps, counts, samples, batch, out, plen * batch)
    assert rc == OK, (rc, L.sh_last_error(_ctx()))
    return out.raw


def prove(L, c):
    """sh_mod_stark_prove on a Case (values and coefficients as the case stores them) -> the batch's flat proofs"""
    counts, coefs, exps = c.terms()
    return prove_raw(L, c.p, c.witness_wire(), c.input_wire(), c.steps, c.ext, c.sp, c.samples, c.batch,
                     (wire(coefs), exps, (ctypes.c_uint32 * c.width)(*counts)))


def mvpolys(F, sp):
    from starks_amd.multivariate_polynomial import multivariates_over
    mv = multivariates_over(F, len(sp)).factory
    return [mv({k: F(v) for k, v in d.items()}) for d in sp]


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(L, name):
    """every case of the modulus through sh_mod_stark_prove equals the oracle's flat proof byte for byte"""
    cases = [c for c in sc.GRID if c.name == name]
    assert cases
    for c in cases:
        assert prove(L, c) == sc.oracle_flat(c), c.id


def test_fixture(L):
    """the live reference's STARK.mk_proof over BN254, Goldilocks and P43 (tests/golden/generate_mod_stark.py)"""
    G = load_golden("mod_stark.json")["cases"]
    for key, c in sc.FIXTURE.items():
        got = prove(L, c)
        assert len(got) == G[key]["len"] and hashlib.sha256(got).hexdigest() == G[key]["sha256"] and got[:64].hex() == G[key]["head"], key


def test_above_the_mimc_prime(L):
    """X' = X^3 from p - 1 over P43: every P value in every opened leaf is p - 1 >= MIMC_P, which a MiMC canonicalisation would change"""
    c = sc.P43_CONST
    got = prove(L, c)
    assert got == sc.oracle_flat(c)
    assert set(sc.opened_p_values(got, c)) == {sc.P43 - 1}


# ---- 2. the device form and the flags ---------------------------------------------------------------------------------------------------
def test_device_form_names_the_broken_proofs(L):
    """a mixed batch through sh_dev_mod_stark_prove: sh_stark_status_batch names exactly the broken proofs, the valid ones keep their
    bytes, and the context proves correctly afterwards"""
    base = sc.BREAK_BASE
    units, want = sc.broken_witnesses()
    units, want = units + [units[0]], want + [0]
    batch, ctx = len(units), _ctx()
    limbs = b"".join(int(v).to_bytes(32, "little") for w in units for col in w for v in col)
    inl = b"".join(int(v).to_bytes(32, "little") for v in base.inputs[0]) * batch
    coefs, exps, counts = term_args(base.sp, base.p)
    plen = sc.proof_len(base)
    dw, di, dp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    for ptr, nbytes in ((dw, len(limbs)), (di, len(inl)), (dp, plen * batch)):
        assert L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)) == OK
    try:
        assert L.sh_stark_status(ctx) in (OK, CONSTRAINT)  # drop what earlier tests may have left
        assert L.sh_dev_upload(ctx, limbs, dw, len(limbs)) == OK and L.sh_dev_upload(ctx, inl, di, len(inl)) == OK
        rc = L.sh_dev_mod_stark_prove(ctx, b32(base.p), dw, di, base.steps, base.ext, base.width, coefs, exps, counts, 80, batch, dp)
        assert rc == OK, (rc, L.sh_last_error(ctx))
        bad = ctypes.create_string_buffer(batch)
        assert L.sh_stark_status_batch(ctx, bad, batch) == CONSTRAINT
        assert list(bad.raw) == want
        assert L.sh_stark_status(ctx) == OK  # the flags are dropped once reported
        out = ctypes.create_string_buffer(plen * batch)
        assert L.sh_dev_download(ctx, dp, out, plen * batch) == OK
        assert out.raw[:plen] == sc.oracle_flat(base) == out.raw[-plen:]
        back = ctypes.create_string_buffer(len(limbs))
        assert L.sh_dev_download(ctx, dw, back, len(limbs)) == OK and back.raw == limbs  # the witness is not modified
    finally:
        assert L.sh_sync(ctx) == OK
        for ptr in (dw, di, dp):
            L.sh_dev_free(ctx, ptr)
    # the host form on a broken witness returns SH_ERR_CONSTRAINT
    out = ctypes.create_string_buffer(plen)
    w1 = wire([v for col in units[1] for v in col])
    assert L.sh_mod_stark_prove(ctx, b32(base.p), w1, base.input_wire(), base.steps, base.ext, base.width, coefs, exps, counts, 80, 1, out,
                                plen) == CONSTRAINT
    c = [x for x in sc.GRID if x.name == "bn254" and x.shape == "s32" and not x.plus_p][0]
    assert prove(L, c) == sc.oracle_flat(c)


# ---- 3. the Python call sites ------------------------------------------------------------------------------------------------------------
def test_python_stark_over_bn254(L):
    from starks_amd import IntegersModP
    from starks_amd.stark import STARK
    c = sc.FIXTURE["bn254-s8-w2"]
    F = IntegersModP(c.p)
    st = STARK(F, c.steps, c.ext, c.width, mvpolys(F, c.sp))
    w = c.witnesses()[0]
    boundary = [(0, j, F(v)) for j, v in enumerate(c.inputs[0])]
    proof = st.mk_proof([[F(v) for v in col] for col in w], boundary)
    assert proof == sc.oracle_proofs(c)[0]
    assert st.verify_proof(proof, w, boundary)
    leaf = proof[2][0][0]
    bad = [proof[0], proof[1], [[bytes([leaf[0] ^ 1]) + leaf[1:]] + proof[2][0][1:]] + proof[2][1:], proof[3]]
    with pytest.raises(AssertionError):
        st.verify_proof(bad, w, boundary)
    with pytest.raises(AssertionError):  # a broken witness: the reference's `assert cp % z == 0`
        st.mk_proof(sc.broken_witnesses()[0][3], boundary)


# ---- 4. the tuned MiMC prover as yardstick ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps,ext,sp,batch", [(1 << 10, 8, sc.MIMC_2, 3), (1 << 13, 8, sc.MIMC_2, 1), (8, 8, sc.QUINTIC_9, 2),
                                                (1 << 12, 8, sc.MIMC_2, 64), (1 << 18, 8, sc.MIMC_2, 1)],
                         ids=["s1024-b3", "s8192-b1", "s8-w9", "s4096-b64", "s262144-b1"])
def test_mimc_prime_through_the_generic_entry(L, steps, ext, sp, batch):
    """the MiMC prime through sh_mod_stark_prove equals sh_stark_prove's bytes (2^13 steps: n * batch is above the serial-tree limit
    2^15, the later rounds below it; 64 x 2^12 and 2^18 steps are the sizes of the timed shapes: 2^19 and more leaf rows and 2^21 and
    more domain points per launch, transforms of two and three passes with the short-input first pass, a batch inversion of 2^17
    chunks)"""
    from starks_amd import IntegersModP, stark
    p, width = sc.MIMC_P, len(sp)
    rnd = random.Random(steps)
    inp = wire([rnd.randrange(p) for _ in range(batch * width)])
    polys = mvpolys(IntegersModP(p), sp)
    if width == 9:
        wit = wire([v for b in range(batch)
                    for col in pyoracle.get_computational_trace(mc.ints(inp)[b * 9:b * 9 + 9], steps, sp, p) for v in col])
    else:
        wit = stark.witness_flat(inp, steps, width, polys, batch)
    want = stark.prove_flat(wit, inp, steps, ext, width, polys, batch)
    assert prove_raw(L, p, wit, inp, steps, ext, sp, 80, batch) == want


# ---- 5. sizes the coefficient oracle does not reach ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "goldilocks"])
def test_4096_steps_verify(L, name):
    """steps 2^12, ext 8: the proof is accepted by the oracle's verifier and by the Python verify_proof"""
    from starks_amd import IntegersModP
    from starks_amd.stark import STARK, unpack_proof
    p, steps, ext, sp = MODULI[name], 1 << 12, 8, sc.MIMC_2
    inputs = [2, 5]
    w = pyoracle.get_computational_trace(inputs, steps, sp, p)
    flat = prove_raw(L, p, wire([v for col in w for v in col]), wire(inputs), steps, ext, sp)
    proof = unpack_proof(flat, steps, ext, 2, 3)
    assert pyoracle.verify_stark_proof(proof, [col[-1] for col in w], inputs, sp, steps, ext, p=p)
    F = IntegersModP(p)
    st = STARK(F, steps, ext, 2, mvpolys(F, sp))
    assert st.verify_proof(proof, w, [(0, j, v) for j, v in enumerate(inputs)])


# ---- 6. interleaved calls ----------------------------------------------------------------------------------------------------------------
def test_interleaved_with_the_mimc_prover(L):
    """sh_stark_prove and sh_mod_stark_prove take turns on one context with the same step polynomials: each keeps its own term image"""
    from starks_amd import IntegersModP, stark
    c = sc.FIXTURE["bn254-s8-w2"]
    polys = mvpolys(IntegersModP(sc.MIMC_P), c.sp)
    wm = wire([v for col in pyoracle.get_computational_trace(c.inputs[0], c.steps, c.sp, sc.MIMC_P) for v in col])
    im = wire(c.inputs[0])
    first_m, first_g = stark.prove_flat(wm, im, c.steps, c.ext, c.width, polys), prove(L, c)
    assert first_g == sc.oracle_flat(c)
    for _ in range(2):
        assert stark.prove_flat(wm, im, c.steps, c.ext, c.width, polys) == first_m
        assert prove(L, c) == first_g
    g = [x for x in sc.GRID if x.name == "goldilocks" and x.shape == "s8"][0]  # the same terms over a third modulus
    assert prove(L, g) == sc.oracle_flat(g) and prove(L, c) == first_g


# ---- 7. the errors -----------------------------------------------------------------------------------------------------------------------
def test_refusals(L):
    """every refusal returns its status with the entry's name in sh_last_error; the buffers are far too small for the refused shapes, so
    a call that got as far as reading them would be seen"""
    ctx, c = _ctx(), sc.FIXTURE["bn254-s8-w2"]
    coefs, exps, counts = term_args(c.sp, c.p)
    cub = term_args(sc.CUBIC_1, c.p)
    wit, inp, plen = c.witness_wire(), c.input_wire(), sc.proof_len(c)
    out = ctypes.create_string_buffer(plen)

    def host(p=c.p, steps=8, ext=8, width=2, terms=(coefs, exps, counts), samples=80, batch=1, cap=plen, w=wit):
        rc = L.sh_mod_stark_prove(ctx, b32(p) if p is not None else None, w, inp, steps, ext, width, terms[0], terms[1], terms[2], samples,
                                  batch, out, cap)
        return rc, L.sh_last_error(ctx).decode()

    assert host()[0] == OK
    table = [
        (dict(p=1 << 64), INVALID), (dict(p=1), INVALID), (dict(p=0), INVALID),
        (dict(p=sc.BABYBEAR), ROOT_ORDER), (dict(p=65537, steps=1 << 10, ext=1 << 7), ROOT_ORDER),  # 2-adicity 16 < 17
        (dict(steps=12), INVALID), (dict(steps=1), INVALID), (dict(ext=1), INVALID), (dict(ext=6), INVALID),
        (dict(width=0), INVALID), (dict(width=10), UNSUPPORTED),
        (dict(steps=1 << 21, ext=8), UNSUPPORTED), (dict(steps=16, ext=2, width=1, terms=cub), UNSUPPORTED),
        (dict(samples=0), INVALID), (dict(batch=0), INVALID), (dict(batch=65536), UNSUPPORTED),
        (dict(cap=plen - 1), TOO_SMALL), (dict(batch=2), TOO_SMALL), (dict(w=None), INVALID), (dict(p=None), INVALID),
    ]
    for kw, want in table:
        rc, text = host(**kw)
        assert rc == want and text.startswith("sh_mod_stark_prove: "), (kw, rc, text)
    d = ctypes.c_void_p()
    assert L.sh_dev_alloc(ctx, 4096, ctypes.byref(d)) == OK
    try:
        for kw, want in ((dict(p=1 << 64), INVALID), (dict(p=sc.BABYBEAR), ROOT_ORDER), (dict(steps=12), INVALID), (dict(batch=0), INVALID),
                         (dict(batch=65536), UNSUPPORTED), (dict(width=10), UNSUPPORTED)):
            a = dict(p=c.p, steps=8, ext=8, width=2, batch=1)
            a.update(kw)
            rc = L.sh_dev_mod_stark_prove(ctx, b32(a["p"]), d, d, a["steps"], a["ext"], a["width"], coefs, exps, counts, 80, a["batch"], d)
            assert rc == want and L.sh_last_error(ctx).decode().startswith("sh_dev_mod_stark_prove: "), (kw, rc)
    finally:
        L.sh_dev_free(ctx, d)
    assert host()[0] == OK and out.raw == sc.oracle_flat(c)
