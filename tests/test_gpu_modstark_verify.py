"""The STARK verifiers over any prime modulus below 2^256 on the MI355X (sh_mod_stark_verify_batch, sh_dev_mod_stark_verify:
starks_amd/csrc/modverify_items.cuh, modverify_dev.hip, api_modverify.hip): the proofs sh_mod_stark_prove writes over the whole grid of
tests/modstark_cases.py are accepted; in mixed batches every status equals the host verifier's (sh_mod_stark_verify, itself pinned to the
exact oracle by tests/test_modstark_verify_host.py) and only the bad proofs are rejected; unreduced storage and values above the MiMC
prime; the device form on witnesses and proofs that never leave the device; the MiMC prime through the generic path against
sh_stark_verify_batch; two moduli on two contexts; the errors, each refused on the host before any launch; the Python call sites."""
import ctypes
import struct

import pytest

import modntt_cases as mc
import modstark_cases as sc
import modstark_verify_cases as vc
from modntt_cases import wire
from modstark_verify_cases import INVALID, OK, REJECTED, ROOT_ORDER, UNSUPPORTED, b32
from oracle import pyoracle
from test_gpu_modfri import Dev, _ctx
from test_gpu_modstark import mvpolys, prove, term_args
from test_modstark_verify_host import STARK_CASES, golden_mimc_cases
from verify_batch_layout import stark_regions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def _terms(P):
    counts, coefs, exps = P.terms()
    return wire(coefs), exps, (ctypes.c_uint32 * P.width)(*counts)


def host(L, P, samples=None):
    return L.sh_mod_stark_verify(b32(P.p), P.flat, len(P.flat), wire(P.inputs), wire(P.outputs), P.steps, P.ext, P.width, *_terms(P),
                                 samples or P.samples)


def batch_verify(L, proofs, ctx=None):
    """sh_mod_stark_verify_batch on vc.Proofs of one shape and one set of terms -> the statuses"""
    P = proofs[0]
    assert all(q.shape() == P.shape() for q in proofs)
    status = (ctypes.c_int32 * len(proofs))()
    rc = L.sh_mod_stark_verify_batch(ctx or _ctx(), b32(P.p), b"".join(q.flat for q in proofs), len(P.flat),
                                     b"".join(wire(q.inputs) for q in proofs), b"".join(wire(q.outputs) for q in proofs), P.steps, P.ext,
                                     P.width, *_terms(P), P.samples, len(proofs), status)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))
    return list(status)


def both(L, proofs):
    return batch_verify(L, proofs), [host(L, q) for q in proofs]


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.MODULI))
def test_grid(L, name):
    """every case of the modulus, proved by sh_mod_stark_prove: every status is SH_OK and equals sh_mod_stark_verify's (s2: no FRI
    round, the final layer against l_root)"""
    cases = [c for c in sc.GRID if c.name == name]
    assert cases and {c.shape for c in cases} >= ({"s2"} if name == "f17" else {"s2", "s8", "s16x4", "s32", "s8w9"})
    for c in cases:
        flat, plen = prove(L, c), sc.proof_len(c)
        proofs = [P.derive("", flat=flat[b * plen:(b + 1) * plen]) for b, P in enumerate(vc.honest(c))]
        assert both(L, proofs) == ([OK] * c.batch,) * 2, c.id


# ---- 2. mixed batches ----------------------------------------------------------------------------------------------------------------
def _own_proofs(L, name, shape, nb, samples):
    """nb honest proofs of the shape, each from its own inputs, proved on the device in one call"""
    steps, ext, sp = sc.SHAPES[shape]
    c = sc.Case(name, shape, steps, ext, sp, batch=nb, samples=samples, tag="-mixed")
    flat = prove(L, c)
    plen = len(flat) // nb
    return [vc.Proof(c.p, steps, ext, sp, samples, flat[b * plen:(b + 1) * plen], c.inputs[b], [col[-1] for col in w], "%s#%d" % (c.id, b))
            for b, w in enumerate(c.witnesses())]


@pytest.mark.parametrize("samples", [80, 7])
@pytest.mark.parametrize("name,shape", [("bn254", "s8"), ("goldilocks", "s32")])
@pytest.mark.parametrize("nb", [65, 3, 1])
def test_mixed_batches(L, name, shape, nb, samples):
    """nb proofs with their own inputs and outputs, every third one with a bit flipped in another region of the layout, then proofs with
    input 0 or the last output off by one beside their honest counterparts; the same batch once more under another step-polynomial
    coefficient, where every proof is rejected.  Every status is the host verifier's and only the bad proofs are rejected.  65 crosses
    the index kernel's 16 proofs per block, 65 x 80 the spot kernel's 64-lane blocks"""
    good = _own_proofs(L, name, shape, nb, samples)
    proofs = []
    for b, P in enumerate(good):
        if b % 3 == 2:
            bad = vc.region_flips(P)
            P = bad[(b // 3) % len(bad)]
        proofs.append(P)
    proofs += [vc.wrong_input(good[0]), good[0], vc.wrong_output(good[-1]), good[-1]]
    want = [REJECTED if b % 3 == 2 else OK for b in range(nb)] + [REJECTED, OK, REJECTED, OK]
    dev, hst = both(L, proofs)
    assert hst == want and dev == hst
    others = [vc.wrong_constant(P) for P in good[:3]]  # the transition check alone
    assert both(L, others) == ([REJECTED] * len(others),) * 2


@pytest.mark.parametrize("cid", vc.SINGLE_CHECK_IDS)
def test_single_check_rejections(L, cid):
    P, const, inp, out = vc.single_check(sc._BY_ID[cid])
    assert both(L, [P, inp, out, P]) == ([OK, REJECTED, REJECTED, OK],) * 2
    assert both(L, [const]) == ([REJECTED],) * 2


# ---- 3. unreduced storage, values above the MiMC prime --------------------------------------------------------------------------------
def test_values_stored_plus_p(L):
    for cid in ("bn254-s8-b1-s80", "goldilocks-s16x4-b1-s80", "f257-s32-b1-s80"):
        P = vc.stored_plus_p(vc.honest(sc._BY_ID[cid])[0])
        assert both(L, [P, vc.wrong_input(P)]) == ([OK, REJECTED],) * 2, cid


def test_above_the_mimc_prime(L):
    good, as_mimc = vc.p43_const()
    assert both(L, [good]) == ([OK], [OK])
    assert both(L, [as_mimc]) == ([REJECTED], [REJECTED])
    assert both(L, [vc.not_row0(sc._BY_ID["bn254-s8-b1-s80"])]) == ([REJECTED], [REJECTED])


# ---- 4. the device form --------------------------------------------------------------------------------------------------------------
def _dev_verify(L, ctx, p, d_proof, d_in, d_out, io_stride, steps, ext, width, terms, samples, batch):
    st = Dev(L, 4 * batch, ctx)
    rc = L.sh_dev_mod_stark_verify(ctx, b32(p), d_proof.ptr, d_in.ptr, d_out, io_stride, steps, ext, width, *terms, samples, batch, st.ptr)
    assert rc == OK, (rc, L.sh_last_error(ctx))
    out = list((ctypes.c_int32 * batch).from_buffer_copy(st.get()))
    st.free()
    return out


@pytest.mark.parametrize("name,lg,batch", [("bn254", 10, 3), ("goldilocks", 14, 2)])
def test_device_form(L, name, lg, batch):
    """sh_dev_mod_stark_prove, then sh_dev_mod_stark_verify on its d_proof with d_inputs = d_witness (row 0 of a trace is its inputs),
    d_outputs = d_witness + (steps - 1) elements and io_stride = steps: nothing is downloaded before the verdict.  Then one flipped bit per proof: all rejected, every status the host
    verifier's"""
    ctx, p, steps, ext, sp = _ctx(), sc.MODULI[name], 1 << lg, 8, sc.MIMC_2
    inputs = [[2 + 3 * b, 5 + b] for b in range(batch)]
    wits = [pyoracle.get_computational_trace(inp, steps, sp, p) for inp in inputs]
    terms = term_args(sp, p)
    plen = L.sh_stark_proof_len(steps, ext, 2, 3, 80)
    dw = Dev(L, 32 * batch * 2 * steps, ctx).put_values([v for w in wits for col in w for v in col])
    di = Dev(L, 32 * batch * 2, ctx).put_values([v for inp in inputs for v in inp])
    dp = Dev(L, plen * batch, ctx)
    assert L.sh_stark_status(ctx) in (OK, -8)  # drop what earlier tests may have left
    rc = L.sh_dev_mod_stark_prove(ctx, b32(p), dw.ptr, di.ptr, steps, ext, 2, *terms, 80, batch, dp.ptr)
    assert rc == OK, (rc, L.sh_last_error(ctx))
    d_out = ctypes.c_void_p(dw.ptr.value + 32 * (steps - 1))
    assert _dev_verify(L, ctx, p, dp, dw, d_out, steps, steps, ext, 2, terms, 80, batch) == [OK] * batch
    assert L.sh_stark_status(ctx) == OK
    flat = dp.get()
    regions, end = stark_regions(steps, ext, 2, 3, 80)
    assert end == plen
    bad = bytearray(flat)
    for b in range(batch):
        a, e = regions[(5 * b + 2) % len(regions)][1:]
        bad[b * plen + (a + e) // 2] ^= 0x10
    assert L.sh_dev_upload(ctx, bytes(bad), dp.ptr, len(bad)) == OK
    dev = _dev_verify(L, ctx, p, dp, dw, d_out, steps, steps, ext, 2, terms, 80, batch)
    hst = [L.sh_mod_stark_verify(b32(p), bytes(bad[b * plen:(b + 1) * plen]), plen, wire(inputs[b]), wire([col[-1] for col in wits[b]]), steps,
                                 ext, 2, *terms, 80) for b in range(batch)]
    assert dev == [REJECTED] * batch and dev == hst
    for d in (dw, di, dp):
        d.free()


# ---- 5. the MiMC prime through the generic path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", STARK_CASES, ids=lambda c: c["name"])
def test_mimc_prime_equals_the_mimc_verifier(L, c):
    """the golden flat proofs and flipped copies of them: sh_mod_stark_verify_batch with modulus = the MiMC prime gives the statuses of
    sh_stark_verify_batch"""
    (coefs, exps, counts), cases = golden_mimc_cases(c, 1)
    nb = len(cases)
    args = (b"".join(x[1] for x in cases), len(cases[0][1]), b"".join(x[2] for x in cases), b"".join(x[3] for x in cases), c["steps"], c["ext"],
            c["width"], coefs, exps, counts, 80, nb)
    want, got = (ctypes.c_int32 * nb)(), (ctypes.c_int32 * nb)()
    assert L.sh_stark_verify_batch(_ctx(), *args, want) == OK
    assert L.sh_mod_stark_verify_batch(_ctx(), b32(sc.MIMC_P), *args, got) == OK, L.sh_last_error(_ctx())
    assert list(got) == list(want) and got[0] == OK and got[nb - 1] == OK and list(got).count(REJECTED) == nb - 2


# ---- 6. two moduli at once -----------------------------------------------------------------------------------------------------------
def test_two_moduli_on_two_contexts(L):
    """BN254 on one context and Goldilocks on another, device forms enqueued back to back with no synchronisation in between: each
    status vector is that of its run alone (a modulus kept in a device global fails here)"""
    from starks_amd import _lib
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    runs = []
    for name, ctx in zip(("bn254", "goldilocks"), ctxs):
        good = vc.honest(sc._BY_ID["%s-s32-b1-s80" % name])[0]
        proofs = [good] + vc.region_flips(good)[:6] + [vc.wrong_input(good), good]
        alone = batch_verify(L, proofs, ctx)
        assert alone == [OK] + [REJECTED] * 7 + [OK]
        nb = len(proofs)
        d_proof, d_in, d_out, d_st = Dev(L, len(good.flat) * nb, ctx), Dev(L, 32 * 3 * nb, ctx), Dev(L, 32 * 3 * nb, ctx), Dev(L, 4 * nb, ctx)
        assert L.sh_dev_upload(ctx, b"".join(q.flat for q in proofs), d_proof.ptr, d_proof.nbytes) == OK
        d_in.put_values([v for q in proofs for v in q.inputs])
        d_out.put_values([v for q in proofs for v in q.outputs])
        runs.append((good, ctx, d_proof, d_in, d_out, d_st, alone))
    for _ in range(4):
        for good, ctx, d_proof, d_in, d_out, d_st, alone in runs:
            assert L.sh_dev_mod_stark_verify(ctx, b32(good.p), d_proof.ptr, d_in.ptr, d_out.ptr, 1, good.steps, good.ext, good.width,
                                             *_terms(good), good.samples, len(alone), d_st.ptr) == OK, L.sh_last_error(ctx)
    for good, ctx, d_proof, d_in, d_out, d_st, alone in runs:
        assert L.sh_sync(ctx) == OK
        assert list((ctypes.c_int32 * len(alone)).from_buffer_copy(d_st.get())) == alone, good.id
        for d in (d_proof, d_in, d_out, d_st):
            d.free()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(L):
    """every refusal comes from the host, before a launch: the counters of sh_ctx_stats do not move, the status buffer is not written,
    and sh_last_error opens with the entry's name and gives the cause"""
    ctx = _ctx()
    P = vc.honest(sc._BY_ID["bn254-s8-b1-s80"])[0]
    flat, inb, outb = P.flat, wire(P.inputs), wire(P.outputs)
    coefs, exps, counts = _terms(P)
    assert batch_verify(L, [P]) == [OK]  # the terms are uploaded: the refusals below find a warm context
    st = Dev(L, 64)
    assert L.sh_dev_upload(ctx, bytes([0x5a]) * 64, st.ptr, 64) == OK
    buf = Dev(L, len(flat) + 64)
    stats0 = (ctypes.c_uint64 * 4)()
    assert L.sh_ctx_stats(ctx, stats0) == OK
    status = (ctypes.c_int32 * 2)(77, 77)

    def call(mod=P.p, steps=8, ext=8, width=2, sm=80, plen=len(flat), proofs=flat, counts=counts, exps=exps):
        rc = L.sh_mod_stark_verify_batch(ctx, b32(mod), proofs, plen, inb, outb, steps, ext, width, coefs, exps, counts, sm, 1, status)
        msg = L.sh_last_error(ctx).decode()
        assert msg.startswith("sh_mod_stark_verify_batch: "), msg
        if plen == len(flat):  # the device form refuses the same shapes
            assert L.sh_dev_mod_stark_verify(ctx, b32(mod), buf.ptr, buf.ptr, buf.ptr, 1, steps, ext, width, coefs, exps, counts, sm, 1,
                                             st.ptr) == rc
            assert L.sh_last_error(ctx).decode() == "sh_dev_mod_stark_verify: " + msg.split(": ", 1)[1]
        return rc, msg

    for bad in (P.p - 1, 0, 1):
        rc, msg = call(mod=bad)
        assert rc == INVALID and "odd" in msg
    rc, msg = call(width=0)
    assert rc == INVALID and "width" in msg
    rc, msg = call(sm=0)
    assert rc == INVALID and "samples" in msg
    for steps, ext in ((12, 8), (8, 12), (1, 8)):
        rc, msg = call(steps=steps, ext=ext)
        assert rc == INVALID and "powers of two" in msg
    rc, msg = call(steps=1 << 12, ext=1 << 12)
    assert rc == INVALID and "2^24" in msg
    rc, msg = call(width=10)
    assert rc == UNSUPPORTED and "width is limited to 9" in msg
    rc, msg = call(counts=(ctypes.c_uint32 * 2)(257, 1))
    assert rc == UNSUPPORTED and "terms" in msg
    rc, msg = call(counts=(ctypes.c_uint32 * 2)(0, 0))
    assert rc == INVALID and "no terms" in msg
    rc, msg = call(mod=sc.BABYBEAR)
    assert rc == ROOT_ORDER and "G2 = 7^((p - 1) // (steps * ext)) does not have order steps * ext modulo p (G2^(n/2) != -1)" in msg
    rc, msg = call(ext=32, exps=bytes([1, 0, 1, 0, 0, 255]))
    assert rc == INVALID and "16 points" in msg
    rc, msg = call(sm=2**32 - 1)
    assert rc == UNSUPPORTED and "sampled rows" in msg
    assert status[0] == 77
    # a proof length that is not the shape's: the statuses are the host verifier's, nothing is launched
    rc, msg = call(plen=len(flat) - 32)
    assert rc == INVALID and "proof_len" in msg and status[0] == INVALID
    status[0] = 77
    # null pointers, a pointer off by 2 bytes, batch 0, io_stride 0
    assert L.sh_mod_stark_verify_batch(ctx, None, flat, len(flat), inb, outb, 8, 8, 2, coefs, exps, counts, 80, 1, status) == INVALID
    assert L.sh_mod_stark_verify_batch(ctx, b32(P.p), flat, len(flat), inb, outb, 8, 8, 2, coefs, exps, counts, 80, 0, status) == INVALID
    assert L.sh_mod_stark_verify_batch(ctx, b32(P.p), flat, len(flat), inb, outb, 8, 8, 2, None, exps, counts, 80, 1, status) == INVALID
    dev = lambda dp, di, do, ds, stride=1: L.sh_dev_mod_stark_verify(ctx, b32(P.p), dp, di, do, stride, 8, 8, 2, coefs, exps, counts, 80, 1, ds)
    assert dev(None, buf.ptr, buf.ptr, st.ptr) == INVALID
    assert dev(buf.ptr, buf.ptr, buf.ptr, st.ptr, 0) == INVALID
    odd = ctypes.c_void_p(buf.ptr.value + 2)
    for args in ((odd, buf.ptr, buf.ptr, st.ptr), (buf.ptr, odd, buf.ptr, st.ptr), (buf.ptr, buf.ptr, odd, st.ptr),
                 (buf.ptr, buf.ptr, buf.ptr, ctypes.c_void_p(st.ptr.value + 2))):
        assert dev(*args) == INVALID
        assert "aligned" in L.sh_last_error(ctx).decode()
    stats1 = (ctypes.c_uint64 * 4)()
    assert L.sh_ctx_stats(ctx, stats1) == OK and list(stats1) == list(stats0)
    assert st.get() == bytes([0x5a]) * 64 and status[0] == 77
    # a valid call afterwards on the same context
    assert batch_verify(L, [P, vc.wrong_input(P)]) == [OK, REJECTED]
    st.free()
    buf.free()


# ---- 8. Python -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "goldilocks"])
def test_python_call_sites(L, name):
    from starks_amd import IntegersModP, _lib, stark
    c = sc._BY_ID["%s-s8-b1-s80" % name]
    F = IntegersModP(c.p)
    st = stark.STARK(F, c.steps, c.ext, c.width, mvpolys(F, c.sp))
    w = c.witnesses()[0]
    boundary = [(0, j, F(v)) for j, v in enumerate(c.inputs[0])]
    proof = st.mk_proof([[F(v) for v in col] for col in w], boundary)
    assert st.verify_proof_mod_native(proof, w, boundary) is True
    flat = stark.pack_proof(proof)
    bad = bytearray(flat)
    bad[len(flat) // 2] ^= 1
    inb, outb = wire(c.inputs[0]), wire([col[-1] for col in w])
    assert stark.mod_verify_flat_batch(c.p, flat + bytes(bad) + flat, inb * 3, outb * 3, c.steps, c.ext, c.width, st.step_polys,
                                       3) == [True, False, True]
    with pytest.raises(AssertionError):
        st.verify_proof_mod_native(stark.unpack_proof(bytes(bad), c.steps, c.ext, c.width, c.degree), w, boundary)
    with pytest.raises(_lib.StarkHipError) as err:
        stark.mod_verify_flat_batch(c.p, flat[:-32], inb, outb, c.steps, c.ext, c.width, st.step_polys, 1)
    assert err.value.status == INVALID
