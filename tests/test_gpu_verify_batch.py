"""The batch verifiers on the GPU (sh_stark_verify_batch / sh_fri_verify_batch / sh_dev_stark_verify, csrc/verify_dev.hip): every
status equals what the host verifier (sh_stark_verify / sh_fri_verify, csrc/verify.hip) returns for that proof alone -- on proofs the
GPU prover wrote for the reference's shapes, the kernel variant matrix, the large units and config 5, untouched and with bit flips in
every region of the layout, wrong public values, and batches where only some proofs are bad."""
import ctypes
import hashlib
import random

import pytest

from conftest import load_golden
from oracle import pyoracle as po
from verify_batch_layout import flips, fri_regions, stark_regions

pytestmark = pytest.mark.gpu

P = po.MIMC_P


def _wire(vals):
    return b"".join((int(v) % P).to_bytes(32, "big") for v in vals)


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


def _stark_batch(proofs, ins, outs, steps, ext, width, polys):
    """-> (device statuses, host statuses) of proofs [(flat)] with per-proof [width] wire inputs / outputs."""
    from starks_amd import _lib, stark
    L = _lib.lib()
    coefs, exps, counts, _ = stark.pack_step_polys(polys, width)
    status = (ctypes.c_int32 * len(proofs))()
    rc = L.sh_stark_verify_batch(_lib.ctx(), b"".join(proofs), len(proofs[0]), b"".join(ins), b"".join(outs), steps, ext, width, coefs,
                                 exps, counts, 80, len(proofs), status)
    assert rc == 0, rc
    host = [L.sh_stark_verify(p, len(p), i, o, steps, ext, width, coefs, exps, counts, 80) for p, i, o in zip(proofs, ins, outs)]
    return list(status), host


def _degree(polys, width):
    from starks_amd import stark
    coefs, exps, _, _ = stark.pack_step_polys(polys, width)
    return max(sum(exps[t * width:(t + 1) * width]) for t in range(len(coefs) // 32))


def _mixed(flat, regions, seed, inb, outb, outs_wrong):
    """untouched copies, one flip per region, a wrong output: (proofs, ins, outs)"""
    cases = [(flat, inb, outb)] + [(bad, inb, outb) for _, bad in flips(flat, regions, 1, seed)]
    cases += [(flat, inb, outs_wrong), (flat, inb, outb)]
    return [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]


@pytest.mark.parametrize("c", load_golden("stark.json"), ids=lambda c: c["name"])
def test_stark_reference_shapes(c):
    from starks_amd import stark
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    steps, ext, width = c["steps"], c["ext"], c["width"]
    polys = [_Poly(d) for d in sp]
    w = po.get_computational_trace(c["inputs"], steps, sp)
    flat = stark.prove_flat(b"".join(_wire(col) for col in w), _wire(c["inputs"]), steps, ext, width, polys)
    assert hashlib.sha256(flat).hexdigest() == c["flat_sha"]
    regions, end = stark_regions(steps, ext, width, _degree(polys, width), 80)
    assert end == len(flat)
    outs = [col[-1] for col in w]
    wrong = list(outs)
    wrong[0] += 1
    proofs, ins, outb = _mixed(flat, regions, c["flat_len"], _wire(c["inputs"]), _wire(outs), _wire(wrong))
    dev, host = _stark_batch(proofs, ins, outb, steps, ext, width, polys)
    assert dev == host
    assert host[0] == 0 and host[-1] == 0 and host.count(-9) >= len(host) - 3
    assert stark.verify_flat_batch(b"".join(proofs[:2]), ins[0] * 2, outb[0] * 2, steps, ext, width, polys, 2) == [True, host[1] == 0]


def _variant_cases():
    return load_golden("stark_variants.json")["cases"]


@pytest.mark.parametrize("c", _variant_cases(), ids=lambda c: c["name"])
def test_stark_variant_matrix(c):
    """Every unit of a variant batch proved in one launch, then verified in one batch with every fifth proof flipped somewhere."""
    import stark_variants as sv
    from starks_amd import stark
    steps, ext, width, nb = c["steps"], c["ext"], c["width"], c["batch"]
    sp = sv.step_polys(c)
    polys = [_Poly(d) for d in sp]
    ins = [sv.unit_inputs(c, u) for u in range(nb)]
    traces = [sv.trace(i, steps, sp) for i in ins]
    flat = stark.prove_flat(b"".join(b"".join(_wire(col) for col in t) for t in traces), b"".join(_wire(i) for i in ins), steps, ext,
                            width, polys, batch=nb)
    plen = c["proof_bytes"]
    proofs = [flat[u * plen:(u + 1) * plen] for u in range(nb)]
    assert hashlib.sha256(proofs[-1]).hexdigest() == c["unit_sha256"][-1]
    regions, _ = stark_regions(steps, ext, width, _degree(polys, width), 80)
    rng = random.Random(nb)
    for u in range(0, nb, 5):
        a, b = regions[rng.randrange(len(regions))][1:]
        bad = bytearray(proofs[u])
        bad[rng.randrange(a, b)] ^= 1 << rng.randrange(8)
        proofs[u] = bytes(bad)
    dev, host = _stark_batch(proofs, [_wire(i) for i in ins], [_wire([col[-1] for col in t]) for t in traces], steps, ext, width, polys)
    assert dev == host
    assert all(host[u] == 0 for u in range(nb) if u % 5)


@pytest.mark.parametrize("logsteps", [12, 14, 16, 18, 20])
def test_stark_large_units(logsteps):
    from starks_amd import batch, stark
    from starks_amd.modp import IntegersModP
    from starks_amd.multivariate_polynomial import generate_Xi_s
    c = [c for c in load_golden("stark_large.json")["cases"] if c["logsteps"] == logsteps][0]
    steps, ext = c["steps"], c["ext"]
    X1, X2 = generate_Xi_s(IntegersModP(P), 2)
    polys = [X1, X1 + X2**3]
    wit, inputs = batch.mimc_stark_unit(c["unit"], steps)
    flat = stark.prove_flat(b"".join(_wire(col) for col in wit), _wire(inputs), steps, ext, 2, polys)
    assert hashlib.sha256(flat).hexdigest() == c["proof_sha256"]
    regions, end = stark_regions(steps, ext, 2, 3, 80)
    assert end == len(flat)
    wrong = [wit[0][-1], wit[1][-1] + 1]
    proofs, ins, outs = _mixed(flat, regions, logsteps, _wire(inputs), _wire([col[-1] for col in wit]), _wire(wrong))
    dev, host = _stark_batch(proofs, ins, outs, steps, ext, 2, polys)
    assert dev == host and host[0] == 0 and host.count(-9) >= len(host) - 3


def _fri_batch(proofs, roots, n, w, md, ex, sm):
    from starks_amd import _lib
    L = _lib.lib()
    wb = w.to_bytes(32, "big")
    status = (ctypes.c_int32 * len(proofs))()
    rc = L.sh_fri_verify_batch(_lib.ctx(), b"".join(proofs), len(proofs[0]), b"".join(roots), n, wb, md, ex, sm, len(proofs), status)
    assert rc == 0, rc
    return list(status), [L.sh_fri_verify(p, len(p), r, n, wb, md, ex, sm) for p, r in zip(proofs, roots)]


@pytest.mark.parametrize("rec", load_golden("fri.json"), ids=lambda r: r["name"])
def test_fri_reference_proofs(rec):
    from oracle import coracle as co
    from starks_amd import _lib, fri
    from test_coracle import _fri_coeffs, wire
    w = int(rec["w"], 16)
    n = _lib.order_of_root(w)
    md, ex, sm = rec["maxdeg_plus_1"], rec["exclude_multiples_of"], rec["samples"]
    flat = co.fri_prove_flat(wire(_fri_coeffs(rec)), w, md, ex, sm)
    assert hashlib.sha256(flat).hexdigest() == rec["flat_sha"]
    root = bytes.fromhex(rec["eval_root"])
    regions, end = fri_regions(n, md, sm)
    assert end == len(flat)
    proofs = [flat] + [bad for _, bad in flips(flat, regions, 2, rec["flat_len"])] + [flat, flat]
    roots = [root] * (len(proofs) - 1) + [hashlib.sha256(root).digest()]
    dev, host = _fri_batch(proofs, roots, n, w, md, ex, sm)
    assert dev == host and host[0] == 0 and host[-2] == 0 and host[-1] == -9
    assert fri.verify_flat_batch(flat * 2, root + bytes(32), n, w, md, ex, batch=2, samples=sm) == [True, False]


@pytest.mark.parametrize("logsteps", [14, 16, 18, 20])
def test_fri_large_commits(logsteps):
    from starks_amd import _lib
    c = [c for c in load_golden("fri_large.json")["cases"] if c["logsteps"] == logsteps][0]
    L, ctx = _lib.lib(), _lib.ctx()
    steps, n = c["steps"], c["domain"]
    w = int(c["w"], 16)
    md, ex, sm = c["maxdeg_plus_1"], c["exclude_multiples_of"], c["samples"]
    plen = int(L.sh_fri_proof_len(n, md, sm))
    dc, dp, dn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert L.sh_dev_alloc(ctx, 32 * n, ctypes.byref(dc)) == 0 and L.sh_dev_alloc(ctx, plen, ctypes.byref(dp)) == 0
    assert L.sh_dev_alloc(ctx, 64 * n, ctypes.byref(dn)) == 0
    try:
        assert L.sh_dev_fill_seeded(ctx, dc, steps, c["seed"]) == 0
        assert L.sh_dev_fri_prove_coeffs(ctx, dc, steps, n, w.to_bytes(32, "big"), md, ex, sm, 1, dp) == 0
        flat = ctypes.create_string_buffer(plen)
        assert L.sh_dev_download(ctx, dp, flat, plen) == 0
        assert hashlib.sha256(flat.raw).hexdigest() == c["proof_sha256"]
        # the committed root: the tree over the polynomial's evaluations on the domain
        assert L.sh_dev_upload(ctx, bytes(32 * (n - steps)), ctypes.c_void_p(dc.value + 32 * steps), 32 * (n - steps)) == 0
        assert L.sh_dev_ntt(ctx, dc, dc, n, 1, w.to_bytes(32, "big"), 0) == 0
        assert L.sh_dev_merkelize(ctx, dc, n, 1, dn) == 0
        root = ctypes.create_string_buffer(32)
        assert L.sh_dev_download(ctx, ctypes.c_void_p(dn.value + 32), root, 32) == 0
    finally:
        for p in (dc, dp, dn):
            L.sh_dev_free(ctx, p)
    regions, end = fri_regions(n, md, sm)
    assert end == plen
    proofs = [flat.raw] + [bad for _, bad in flips(flat.raw, regions, 1, logsteps)]
    dev, host = _fri_batch(proofs, [root.raw] * len(proofs), n, w, md, ex, sm)
    assert dev == host and host[0] == 0 and host.count(-9) >= len(host) - 1


def _mimc_polys():
    from starks_amd.modp import IntegersModP
    from starks_amd.multivariate_polynomial import generate_Xi_s
    X1, X2 = generate_Xi_s(IntegersModP(P), 2)
    return [X1, X1 + X2**3]


@pytest.mark.parametrize("nb", [65, 3, 1])
def test_only_the_bad_proofs_of_a_batch_are_rejected(nb):
    """65 distinct units: flipped bits at 0, 31, 32 and 64, a wrong input at 5, a wrong output at 40; everything else is accepted."""
    from starks_amd import batch, stark
    steps, ext = 64, 8
    polys = _mimc_polys()
    units = [batch.mimc_stark_unit(j, steps) for j in range(nb)]
    flat = stark.prove_flat(b"".join(b"".join(_wire(col) for col in w) for w, _ in units), b"".join(_wire(i) for _, i in units), steps,
                            ext, 2, polys, batch=nb)
    plen = len(flat) // nb
    proofs = [bytearray(flat[u * plen:(u + 1) * plen]) for u in range(nb)]
    ins = [_wire(i) for _, i in units]
    outs = [_wire([col[-1] for col in w]) for w, _ in units]
    rng = random.Random(nb)
    bad = {u for u in (0, 31, 32, 64) if u < nb}
    for u in bad:
        proofs[u][rng.randrange(plen)] ^= 1 << rng.randrange(8)
    if nb > 40:
        ins[5] = _wire([units[5][1][0] + 1, units[5][1][1]])
        outs[40] = _wire([units[40][0][0][-1], units[40][0][1][-1] + 1])
        bad |= {5, 40}
    got = stark.verify_flat_batch(b"".join(bytes(p) for p in proofs), b"".join(ins), b"".join(outs), steps, ext, 2, polys, nb)
    assert [u for u in range(nb) if not got[u]] == sorted(bad)
    dev, host = _stark_batch([bytes(p) for p in proofs], ins, outs, steps, ext, 2, polys)
    assert dev == host


@pytest.mark.parametrize("second", [False, True], ids=["ctx1", "ctx2"])
def test_config5_512_units_verified_on_the_device(second):
    """BASELINE config 5 at size: 512 units of 2^16 steps proved as 2 x 256 by StarkUnitProver and verified on the device behind the
    prover (no synchronisation between the two): all accepted, every status equal to the host verifier's; then 4 device-side copies,
    one flipped bit each, are rejected."""
    from starks_amd import _lib, batch
    steps, chunk = 1 << 16, 256
    pr = batch.StarkUnitProver(steps, 8, chunk, second_context=second)
    L, ctx = pr.L, pr.ctx
    polys = _mimc_polys()
    from starks_amd import stark
    coefs, exps, counts, _ = stark.pack_step_polys(polys, 2)
    try:
        for first in (0, chunk):
            pr.generate(first, chunk)
            pr.prove(chunk)
            status = pr.verify(chunk)
            pr.status()
            assert status == [0] * chunk
            proofs = pr.download(chunk)
            for u, p in enumerate(proofs):
                w, i = batch.mimc_stark_unit(first + u, steps)
                assert L.sh_stark_verify(p, len(p), _wire(i), _wire([col[-1] for col in w]), steps, 8, 2, coefs, exps, counts, 80) == status[u]
        # 4 flipped copies on the device, verified against the witness of units 256..259 still on the device
        plen = pr.plen
        rng = random.Random(5)
        dq, ds = ctypes.c_void_p(), ctypes.c_void_p()
        _lib.check(L.sh_dev_alloc(ctx, 4 * plen, ctypes.byref(dq)), "alloc")
        _lib.check(L.sh_dev_alloc(ctx, 16, ctypes.byref(ds)), "alloc")
        try:
            _lib.check(L.sh_dev_copy(ctx, pr.dp, dq, 4 * plen), "copy")
            for u in range(4):
                off = u * plen + rng.randrange(plen)
                byte = ctypes.create_string_buffer(1)
                _lib.check(L.sh_dev_download(ctx, ctypes.c_void_p(dq.value + off), byte, 1), "dl")
                _lib.check(L.sh_dev_upload(ctx, bytes([byte.raw[0] ^ (1 << rng.randrange(8))]), ctypes.c_void_p(dq.value + off), 1), "ul")
            last = ctypes.c_void_p(pr.dw.value + 32 * (steps - 1))
            _lib.check(L.sh_dev_stark_verify(ctx, dq, pr.dw, last, steps, steps, 8, 2, coefs, exps, counts, 80, 4, ds), "verify")
            st = (ctypes.c_int32 * 4)()
            _lib.check(L.sh_dev_download(ctx, ds, st, 16), "dl")
            assert list(st) == [-9] * 4
        finally:
            L.sh_dev_free(ctx, dq)
            L.sh_dev_free(ctx, ds)
    finally:
        pr.close()


def test_shape_errors_return_the_host_verifiers_code_and_launch_nothing():
    from starks_amd import _lib, stark
    L, ctx = _lib.lib(), _lib.ctx()
    polys = _mimc_polys()
    coefs, exps, counts, _ = stark.pack_step_polys(polys, 2)
    st = (ctypes.c_int32 * 2)(7, 7)
    one = bytes(64)

    def sv(proofs, plen, steps, ext, width=2, cf=coefs, ex=exps, cn=counts, batch=1):
        return L.sh_stark_verify_batch(ctx, proofs, plen, one * 2, one * 2, steps, ext, width, cf, ex, cn, 80, batch, st)

    def hv(proof, steps, ext, width=2, cf=coefs, ex=exps, cn=counts):
        return L.sh_stark_verify(proof, len(proof), one, one, steps, ext, width, cf, ex, cn, 80)

    assert sv(bytes(64), 64, 24, 8) == hv(bytes(64), 24, 8) == -1                          # steps not a power of two
    assert sv(bytes(64), 64, 1 << 21, 8) == hv(bytes(64), 1 << 21, 8) == -1                # ext * steps >= 2^24
    c10 = (ctypes.c_uint32 * 10)(*([1] * 10))
    assert sv(bytes(64), 64, 64, 8, 10, bytes(320), bytes(100), c10) == -6                # width 10
    assert hv(bytes(64), 64, 8, 10, bytes(320), bytes(100), c10) == -6
    assert list(st) == [7, 7]                                                             # nothing written
    # a wrong proof_len: every status is the host verifier's, the call says SH_ERR_INVALID
    good = stark.proof_len(64, 8, 2, 3)
    assert sv(bytes(2 * (good - 32)), good - 32, 64, 8, batch=2) == -1
    assert list(st) == [hv(bytes(good - 32), 64, 8)] * 2
    # FRI: a root of the wrong order, and a final layer over the cap (2^11 points with no round)
    w = pow(7, (P - 1) // 1024, P).to_bytes(32, "big")
    fst = (ctypes.c_int32 * 1)(7)
    assert L.sh_fri_verify_batch(ctx, bytes(32 * 2048), 32 * 2048, bytes(32), 2048, w, 16, 0, 40, 1, fst) == -2
    assert L.sh_fri_verify(bytes(32 * 2048), 32 * 2048, bytes(32), 2048, w, 16, 0, 40) == -2
    w11 = pow(7, (P - 1) // 2048, P).to_bytes(32, "big")
    assert L.sh_fri_verify_batch(ctx, bytes(32 * 2048), 32 * 2048, bytes(32), 2048, w11, 16, 0, 40, 1, fst) == -6
    assert list(fst) == [7]
    with pytest.raises(_lib.StarkHipError):
        stark.verify_flat_batch(bytes(64), one, one, 24, 8, 2, polys, 1)
    # device buffers that are not 4-byte aligned are refused before anything is launched
    d = ctypes.c_void_p()
    _lib.check(L.sh_dev_alloc(ctx, 4096, ctypes.byref(d)), "alloc")
    try:
        odd = ctypes.c_void_p(d.value + 1)
        assert L.sh_dev_stark_verify(ctx, odd, d, d, 1, 64, 8, 2, coefs, exps, counts, 80, 1, d) == -1
        assert L.sh_dev_stark_verify(ctx, d, d, d, 1, 64, 8, 2, coefs, exps, counts, 80, 1, odd) == -1
        assert L.sh_dev_fri_verify(ctx, odd, d, 1024, pow(7, (P - 1) // 1024, P).to_bytes(32, "big"), 256, 0, 40, 1, d) == -1
        assert L.sh_sync(ctx) == 0
    finally:
        L.sh_dev_free(ctx, d)


def test_algebraic_checks_alone_reject():
    """Batches where every Merkle branch and root verifies, so that only one algebraic check can reject: the final layer's degree bound
    (fri_deg512 against maxdeg_plus_1 = 300, the same layout), a FRI row (the first column folded at special_x + 1, the rest honest for
    that column) and the transition constraint (mimc_w2_s8 proved on the device, verified against step polynomials with one coefficient
    off by 1).  Each is mixed with its honest counterpart; the host verifier rejects exactly the bad ones and the device agrees."""
    from oracle import coracle as co
    from starks_amd import _lib, stark
    from test_coracle import _fri_coeffs, wire
    from verify_batch_layout import wrong_fold_fri
    rec = [r for r in load_golden("fri.json") if r["name"] == "fri_deg512"][0]
    w = int(rec["w"], 16)
    n = _lib.order_of_root(w)
    flat = co.fri_prove_flat(wire(_fri_coeffs(rec)), w, 512, 0, 40)
    root = bytes.fromhex(rec["eval_root"])
    for md, want in ((512, 0), (300, -9)):
        dev, host = _fri_batch([flat] * 3, [root] * 3, n, w, md, 0, 40)
        assert host == [want] * 3 and dev == host
    n2 = 1024
    w2 = pow(7, (P - 1) // n2, P)
    coeffs = [pow(3, i, P) for i in range(200)]
    good, groot = wrong_fold_fri(coeffs, n2, w2, 256, 8, 40, 0)
    bad, broot = wrong_fold_fri(coeffs, n2, w2, 256, 8, 40, 1)
    dev, host = _fri_batch([good, bad, good, bad], [groot, broot, groot, broot], n2, w2, 256, 8, 40)
    assert host == [0, -9, 0, -9] and dev == host
    c = [c for c in load_golden("stark.json") if c["name"] == "mimc_w2_s8"][0]
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    wit = po.get_computational_trace(c["inputs"], c["steps"], sp)
    sflat = stark.prove_flat(b"".join(_wire(col) for col in wit), _wire(c["inputs"]), 8, 8, 2, [_Poly(d) for d in sp])
    other = [dict(d) for d in sp]
    k0 = sorted(other[-1])[-1]
    other[-1][k0] = (other[-1][k0] + 1) % P
    for polys, want in ((sp, 0), (other, -9)):
        dev, host = _stark_batch([sflat] * 3, [_wire(c["inputs"])] * 3, [_wire([col[-1] for col in wit])] * 3, 8, 8, 2,
                                 [_Poly(d) for d in polys])
        assert host == [want] * 3 and dev == host
