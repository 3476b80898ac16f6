"""The FRI verifiers over any odd modulus below 2^256 on the MI355X (sh_mod_fri_verify_batch, sh_dev_mod_fri_verify:
starks_amd/csrc/modverify_items.cuh, modverify_dev.hip, api_modverify.hip): the proofs sh_mod_fri_prove writes over the whole grid of
tests/modfri_cases.py are accepted; in mixed batches every status equals the host verifier's (sh_mod_fri_verify, itself pinned to the
exact oracle by tests/test_modverify_host.py) and only the bad proofs are rejected; the device form on proofs and roots that never
leave the device; the MiMC prime through the generic path against sh_fri_verify_batch; larger shapes; two moduli on two contexts; the
Python call sites; the errors, each refused on the host before any launch."""
import ctypes

import pytest

from conftest import load_golden
import modfri_cases as fc
import modntt_cases as mc
import modverify_cases as vc
from modfri_cases import MODULI, root_of
from modverify_cases import INVALID, OK, REJECTED, ROOT_ORDER, UNSUPPORTED, b32
from test_gpu_modfri import Dev, _ctx, prove
from verify_batch_layout import flips, fri_regions

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def host(L, p, flat, mroot, n, w, md, ex=0, sm=40):
    return L.sh_mod_fri_verify(b32(p), flat, len(flat), mroot, n, b32(w), md, ex, sm)


def batch_verify(L, p, proofs, roots, n, w, md, ex=0, sm=40, ctx=None):
    """sh_mod_fri_verify_batch -> the statuses"""
    status = (ctypes.c_int32 * len(proofs))()
    rc = L.sh_mod_fri_verify_batch(ctx or _ctx(), b32(p), b"".join(proofs), len(proofs[0]), b"".join(roots), n, b32(w), md, ex, sm,
                                   len(proofs), status)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))
    return list(status)


def both(L, proofs):
    """vc.Proofs of one shape -> (device statuses, host verifier's statuses)"""
    P = proofs[0]
    dev = batch_verify(L, P.p, [q.flat for q in proofs], [q.merkle_root for q in proofs], P.n, P.root, P.md, P.exclude, P.samples)
    return dev, [host(L, q.p, q.flat, q.merkle_root, q.n, q.root, q.md, q.exclude, q.samples) for q in proofs]


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(L, name):
    """every verifiable case of the modulus, proved by sh_mod_fri_prove: every status is SH_OK and equals sh_mod_fri_verify's"""
    cases = [c for c in fc.GRID if c.name == name and c.verify and c.n >= 4]
    if name == "bn254":
        cases.append(fc.BOTH_TREE_FORMS)
    assert cases
    for c in cases:
        flat = prove(L, c)
        plen = len(flat) // c.batch
        proofs = [flat[b * plen:(b + 1) * plen] for b in range(c.batch)]
        roots = [fc.merkle_root(c, b) for b in range(c.batch)]
        assert batch_verify(L, c.p, proofs, roots, c.n, c.root, c.md, c.exclude, c.samples) == [OK] * c.batch, c.id
        assert [host(L, c.p, f, r, c.n, c.root, c.md, c.exclude, c.samples) for f, r in zip(proofs, roots)] == [OK] * c.batch, c.id


def test_two_rounds_of_80_and_40_samples(L):
    """what the prover emits for samples = 80 over two rounds (80, then 40), which the reference's verifier cannot take"""
    c = fc._BY_ID["goldilocks-n256-md128-c128-x0-s80-b1"]
    assert both(L, [vc.Proof(c.name, c.n, c.md, prove(L, c), fc.merkle_root(c), 0, 80)]) == ([OK], [OK])


# ---- 2. mixed batches ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["bn254-n256-md128-c128-x0-s40-b1", "c2-n256-md128-c128-x0-s40-b1"])
@pytest.mark.parametrize("nb", [65, 3, 1])
def test_mixed_batches(L, cid, nb):
    """nb proofs, every third one with a bit flipped in another region of the layout, then the wrong-fold proof and the degree-too-high
    proof (each with its own root, each beside its honest counterpart): every status is the host verifier's, only the bad ones are
    rejected.  65 crosses the index kernel's 16 proofs per block"""
    c = fc._BY_ID[cid]
    good = vc.Proof(c.name, c.n, c.md, prove(L, c), fc.merkle_root(c))
    regions, end = fri_regions(c.n, c.md, 40)
    assert end == len(good.flat)
    bad = flips(good.flat, regions, 3, nb)
    proofs = [good.with_flat(bad[(b // 3) % len(bad)][1], "") if b % 3 == 2 else good for b in range(nb)]
    proofs += [vc.wrong_fold(c.name, c.n, c.md, 0, 1), vc.wrong_fold(c.name, c.n, c.md, 0, 0)] + list(vc.degree_pair(c.name, c.n, c.md, 0))
    want = [REJECTED if b % 3 == 2 else OK for b in range(nb)] + [REJECTED, OK, OK, REJECTED]
    dev, hst = both(L, proofs)
    assert hst == want and dev == hst


@pytest.mark.parametrize("shape", vc.DEGREE_SHAPES, ids=lambda s: "%s-%d-%d-x%d" % s)
def test_degree_bound_alone_rejects(L, shape):
    """md + 1 coefficients committed honestly: only the final-layer kernel's cross-multiplied check can reject (composite c2 included)"""
    assert both(L, list(vc.degree_pair(*shape)) * 2) == ([OK, REJECTED] * 2,) * 2


def test_unreduced_values(L):
    """final-layer values stored as v + p are v"""
    assert both(L, [vc.unreduced(0), vc.unreduced(1)]) == ([OK, REJECTED],) * 2


# ---- 3. the device form --------------------------------------------------------------------------------------------------------------
def _dev_commit(L, ctx, p, w, n, md, ex, coeffs, batch):
    """[batch][k] coefficients -> (d_proof from sh_dev_mod_fri_prove, d_roots [batch][32] gathered on the device from
    sh_dev_merkelize_plain's trees over sh_dev_mod_ntt's evaluations, everything to free)"""
    k = len(coeffs) // batch
    plen = L.sh_fri_proof_len(n, md, 40)
    src = Dev(L, 32 * len(coeffs), ctx).put_values(coeffs)
    d_proof = Dev(L, plen * batch, ctx)
    assert L.sh_dev_mod_fri_prove(ctx, b32(p), src.ptr, k, n, b32(w), md, ex, 40, batch, d_proof.ptr) == OK, L.sh_last_error(ctx)
    vals = Dev(L, 32 * n * batch, ctx)
    raw = b"".join(b"".join(int(v).to_bytes(32, "little") for v in coeffs[b * k:(b + 1) * k]) + bytes(32 * (n - k)) for b in range(batch))
    assert L.sh_dev_upload(ctx, raw, vals.ptr, len(raw)) == OK
    assert L.sh_dev_mod_ntt(ctx, b32(p), vals.ptr, vals.ptr, n, batch, b32(w), 0) == OK, L.sh_last_error(ctx)
    nodes = Dev(L, 64 * n * batch, ctx)
    assert L.sh_dev_merkelize_plain(ctx, vals.ptr, n, batch, nodes.ptr) == OK
    d_roots = Dev(L, 32 * batch, ctx)
    for b in range(batch):
        assert L.sh_dev_copy(ctx, ctypes.c_void_p(nodes.ptr.value + 64 * n * b + 32), ctypes.c_void_p(d_roots.ptr.value + 32 * b), 32) == OK
    return d_proof, d_roots, [src, vals, nodes]


def _dev_verify(L, ctx, p, w, n, md, ex, d_proof, d_roots, batch):
    st = Dev(L, 4 * batch, ctx)
    rc = L.sh_dev_mod_fri_verify(ctx, b32(p), d_proof.ptr, d_roots.ptr, n, b32(w), md, ex, 40, batch, st.ptr)
    assert rc == OK, (rc, L.sh_last_error(ctx))
    out = list((ctypes.c_int32 * batch).from_buffer_copy(st.get()))
    st.free()
    return out


@pytest.mark.parametrize("name,lg,batch,ex", [("bn254", 10, 3, 8), ("p43", 8, 2, 0), ("bn254", 16, 8, 8), ("bn254", 20, 1, 8)])
def test_device_form_and_larger_shapes(L, name, lg, batch, ex):
    """proofs straight from sh_dev_mod_fri_prove's d_proof and roots from sh_dev_merkelize_plain, never on the host before the verdict;
    then one flipped bit per proof is rejected, and every status equals the host verifier's.  n = 2^16 x 8 and 2^20 x 1 at
    maxdeg_plus_1 = n / 8: five and seven rounds, final layers of 64 points"""
    ctx, p, n = _ctx(), MODULI[name], 1 << lg
    md, w = n // 8, root_of(name, n)
    k = min(md, 200)
    coeffs = [fc.P43 - 1] * (k * batch) if name == "p43" else mc.inputs(lg, k * batch, p)
    coeffs = [v % p for v in coeffs]
    d_proof, d_roots, held = _dev_commit(L, ctx, p, w, n, md, ex, coeffs, batch)
    assert _dev_verify(L, ctx, p, w, n, md, ex, d_proof, d_roots, batch) == [OK] * batch
    flat, roots = d_proof.get(), d_roots.get()
    plen = len(flat) // batch
    assert [host(L, p, flat[b * plen:(b + 1) * plen], roots[32 * b:32 * b + 32], n, w, md, ex) for b in range(batch)] == [OK] * batch
    if lg <= 10:
        assert roots[:32] == mc_root(coeffs[:k], n, p, w)
    # one flip per proof, each in another region
    regions, end = fri_regions(n, md, 40)
    assert end == plen
    bad = bytearray(flat)
    for b in range(batch):
        a, e = regions[(5 * b + 2) % len(regions)][1:]
        bad[b * plen + (a + e) // 2] ^= 0x10
    assert L.sh_dev_upload(ctx, bytes(bad), d_proof.ptr, len(bad)) == OK
    dev = _dev_verify(L, ctx, p, w, n, md, ex, d_proof, d_roots, batch)
    assert dev == [REJECTED] * batch
    assert dev == [host(L, p, bytes(bad[b * plen:(b + 1) * plen]), roots[32 * b:32 * b + 32], n, w, md, ex) for b in range(batch)]
    for d in [d_proof, d_roots] + held:
        d.free()


def mc_root(coeffs, n, p, w):
    from oracle import pyoracle
    return pyoracle.merkelize(mc.transform(coeffs, n, p, w))[1]


def test_errors(L):
    """every refusal comes from the host, before a launch: the counters of sh_ctx_stats do not move, the status buffer is not written,
    and sh_last_error names the cause"""
    ctx = _ctx()
    c = fc._BY_ID["bn254-n64-md32-c32-x0-s40-b1"]
    p, w, flat, root = c.p, c.root, prove(L, c), fc.merkle_root(c)
    st = Dev(L, 64)
    assert L.sh_dev_upload(ctx, bytes([0x5a]) * 64, st.ptr, 64) == OK
    buf = Dev(L, len(flat) + 64)
    stats0 = (ctypes.c_uint64 * 4)()
    assert L.sh_ctx_stats(ctx, stats0) == OK
    status = (ctypes.c_int32 * 2)(77, 77)

    def call(mod=p, root_w=w, n=64, md=32, ex=0, sm=40, plen=len(flat), proofs=flat):
        rc = L.sh_mod_fri_verify_batch(ctx, b32(mod), proofs, plen, root, n, b32(root_w), md, ex, sm, 1, status)
        msg = L.sh_last_error(ctx).decode()
        if plen == len(flat):  # the device form refuses the same shapes
            assert L.sh_dev_mod_fri_verify(ctx, b32(mod), buf.ptr, buf.ptr, n, b32(root_w), md, ex, sm, 1, st.ptr) == rc
        return rc, msg

    for bad in (p - 1, 0, 1):
        rc, msg = call(mod=bad)
        assert rc == INVALID and "odd" in msg
    rc, msg = call(root_w=p + w)
    assert rc == ROOT_ORDER and "below" in msg
    rc, msg = call(root_w=root_of("bn254", 32))
    assert rc == ROOT_ORDER and "order" in msg
    rc, msg = call(n=12)
    assert rc == INVALID and "power of two" in msg
    rc, msg = call(sm=0)
    assert rc == INVALID and "samples" in msg
    rc, msg = call(ex=1)
    assert rc == INVALID and "exclude" in msg
    rc, msg = call(md=1 << 10)
    assert rc == INVALID and "16 points" in msg
    rc, msg = call(n=2048, root_w=root_of("bn254", 2048), md=16)
    assert rc == UNSUPPORTED and "2^10" in msg
    rc, msg = call(n=1 << 26, root_w=root_of("bn254", 1 << 26), md=32)  # a column of 2^24 rows: the host verifier's code
    assert rc == INVALID and "2^24" in msg
    assert L.sh_mod_fri_verify(b32(p), flat, len(flat), root, 1 << 26, b32(root_of("bn254", 1 << 26)), 32, 0, 40) == INVALID
    assert status[0] == 77
    # a proof length that is not the shape's: the statuses are the host verifier's, nothing is launched
    rc, msg = call(plen=len(flat) - 32)
    assert rc == INVALID and "proof_len" in msg and status[0] == INVALID
    status[0] = 77
    rc, msg = call(plen=100, sm=2**32 - 1, proofs=bytes(100))
    assert rc == INVALID and status[0] == INVALID
    # null pointers, a pointer off by 2 bytes, batch 0
    assert L.sh_mod_fri_verify_batch(ctx, None, flat, len(flat), root, 64, b32(w), 32, 0, 40, 1, status) == INVALID
    assert L.sh_mod_fri_verify_batch(ctx, b32(p), flat, len(flat), root, 64, b32(w), 32, 0, 40, 0, status) == INVALID
    assert L.sh_dev_mod_fri_verify(ctx, b32(p), None, buf.ptr, 64, b32(w), 32, 0, 40, 1, st.ptr) == INVALID
    odd = ctypes.c_void_p(buf.ptr.value + 2)
    for args in ((odd, buf.ptr, st.ptr), (buf.ptr, odd, st.ptr), (buf.ptr, buf.ptr, ctypes.c_void_p(st.ptr.value + 2))):
        assert L.sh_dev_mod_fri_verify(ctx, b32(p), args[0], args[1], 64, b32(w), 32, 0, 40, 1, args[2]) == INVALID
        assert "aligned" in L.sh_last_error(ctx).decode()
    stats1 = (ctypes.c_uint64 * 4)()
    assert L.sh_ctx_stats(ctx, stats1) == OK and list(stats1) == list(stats0)
    assert st.get() == bytes([0x5a]) * 64
    # a valid call afterwards on the same context
    assert batch_verify(L, p, [flat], [root], 64, w, 32) == [OK]
    st.free()
    buf.free()


# ---- 4. the MiMC prime through the generic path ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", load_golden("fri.json"), ids=lambda r: r["name"])
def test_mimc_prime_equals_the_mimc_verifier(L, rec):
    """the reference's proofs over the MiMC prime and flipped copies of them: sh_mod_fri_verify_batch with modulus = the MiMC prime gives
    the statuses of sh_fri_verify_batch"""
    from oracle import coracle as co
    from starks_amd import _lib
    from test_coracle import _fri_coeffs, wire
    w = int(rec["w"], 16)
    n = _lib.order_of_root(w)
    md, ex, sm = rec["maxdeg_plus_1"], rec["exclude_multiples_of"], rec["samples"]
    flat = co.fri_prove_flat(wire(_fri_coeffs(rec)), w, md, ex, sm)
    root = bytes.fromhex(rec["eval_root"])
    regions, end = fri_regions(n, md, sm)
    assert end == len(flat)
    proofs = [flat] + [bad for _, bad in flips(flat, regions, 2, rec["flat_len"])] + [flat]
    roots = [root] * (len(proofs) - 1) + [bytes(32)]
    status = (ctypes.c_int32 * len(proofs))()
    assert L.sh_fri_verify_batch(_ctx(), b"".join(proofs), len(flat), b"".join(roots), n, b32(w), md, ex, sm, len(proofs), status) == OK
    got = batch_verify(L, mc.MIMC_P, proofs, roots, n, w, md, ex, sm)
    assert got == list(status) and got[0] == OK and got[1:] == [REJECTED] * (len(proofs) - 1)


# ---- 5. two moduli at once -----------------------------------------------------------------------------------------------------------
def test_two_moduli_on_two_contexts(L):
    """BN254 on one context and Goldilocks on another, device forms enqueued back to back with no synchronisation in between: each
    status vector is that of its run alone (a modulus kept in a device global fails here)"""
    from starks_amd import _lib
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    runs = []
    for name, ctx in zip(("bn254", "goldilocks"), ctxs):
        c = fc._BY_ID["%s-n4096-md1024-c1000-x0-s40-b1" % name]
        good = prove(L, c, ctx)
        regions, _ = fri_regions(c.n, c.md, 40)
        proofs = [good] + [bad for _, bad in flips(good, regions, 1, 7)][:6] + [good]
        want = [OK] + [REJECTED] * (len(proofs) - 2) + [OK]
        d_proof, d_roots, d_st = Dev(L, len(good) * len(proofs), ctx), Dev(L, 32 * len(proofs), ctx), Dev(L, 4 * len(proofs), ctx)
        assert L.sh_dev_upload(ctx, b"".join(proofs), d_proof.ptr, d_proof.nbytes) == OK
        assert L.sh_dev_upload(ctx, fc.merkle_root(c) * len(proofs), d_roots.ptr, d_roots.nbytes) == OK
        runs.append((c, ctx, d_proof, d_roots, d_st, want))
    for _ in range(4):
        for c, ctx, d_proof, d_roots, d_st, want in runs:
            assert L.sh_dev_mod_fri_verify(ctx, b32(c.p), d_proof.ptr, d_roots.ptr, c.n, b32(c.root), c.md, 0, 40, len(want), d_st.ptr) == OK
    for c, ctx, d_proof, d_roots, d_st, want in runs:
        assert L.sh_sync(ctx) == OK
        assert list((ctypes.c_int32 * len(want)).from_buffer_copy(d_st.get())) == want, c.id
        for d in (d_proof, d_roots, d_st):
            d.free()


# ---- 6. Python -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "goldilocks"])
def test_python_call_sites(L, name):
    from starks_amd import IntegersModP, _lib, batch, fri
    c = fc._BY_ID["%s-n256-md128-c128-x0-s40-b1" % name]
    F = IntegersModP(c.p)
    S = fri.SmoothSubgroupFRI(F)
    proof = S.generate_proximity_proof([F(v % c.p) for v in c.coeffs()], F(c.root), c.md)
    m_root = fc.merkle_root(c)
    assert S.verify_proximity_proof_native(proof, m_root, F(c.root), c.md)
    flat = fri.pack_proof(proof)
    bad = bytearray(flat)
    bad[len(flat) // 2] ^= 1
    assert fri.mod_verify_flat_batch(c.p, flat + bytes(bad) + flat, m_root * 3, c.n, c.root, c.md, batch=3) == [True, False, True]
    assert batch.verify_fri_batch([flat, bytes(bad)], [m_root] * 2, c.n, c.root, c.md, modulus=c.p) == [True, False]
    with pytest.raises(AssertionError):
        S.verify_proximity_proof_native(fri.unpack_proof(bytes(bad), c.n, c.md), m_root, F(c.root), c.md)
    with pytest.raises(_lib.StarkHipError) as err:
        fri.mod_verify_flat_batch(c.p, flat[:-32], m_root, c.n, c.root, c.md)
    assert err.value.status == INVALID
