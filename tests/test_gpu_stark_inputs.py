"""GPU half of the STARK input harness (tests/stark_input_cases.py), through the C ABI, exact bytes and exact flags everywhere:

A. the prover (sh_stark_prove, sh_dev_stark_prove after sh_dev_from_wire and after a raw sh_dev_upload of limbs) and the batch verifier
   (sh_dev_stark_verify) on witnesses, inputs, outputs and step-polynomial coefficients stored as x + p: every unit's proof is the
   oracle's proof of the residues (oracle/fastoracle.py at test time; tests/golden/stark_inputs.json for the narrow / middle / wide
   batches), every constraint flag is 0, every verifier status is the host verifier's.
B. the witness check of stark_trace_points_kernel<W>, W = 1..9: one unit per broken (column, step, kind) in one launch, flags equal to
   the predicate on Python ints unit for unit, valid neighbours untouched; the flat-index arithmetic at 2^12 steps; the flag buffer's
   growth; a witness whose row 0 is not the inputs."""
import ctypes
import hashlib
import time

import pytest

import stark_input_cases as sc
import stark_variants as sv

pytestmark = pytest.mark.gpu

P, R = sc.P, sc.R
SAMPLES = 80


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


@pytest.fixture(scope="module")
def sa():
    from starks_amd import _lib, stark

    class NS:
        pass

    ns = NS()
    ns.lib, ns.stark, ns.L = _lib, stark, _lib.lib()
    ns.ctx = _lib.ctx()  # fails loudly when the extension or the GPU is missing
    return ns


class Dev(object):
    """Device buffers of one test, freed at its end."""

    def __init__(self, sa, ctx=None):
        self.sa, self.ctx, self.ptrs = sa, ctx or sa.ctx, []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self.sa.lib.check(self.sa.L.sh_dev_alloc(self.ctx, nbytes, ctypes.byref(p)), "sh_dev_alloc")
        self.ptrs.append(p)
        return p

    def from_wire(self, wire_bytes):  # keeps values >= p as they are
        p = self.alloc(len(wire_bytes))
        self.sa.lib.check(self.sa.L.sh_dev_from_wire(self.ctx, wire_bytes, p, len(wire_bytes) // 32), "sh_dev_from_wire")
        return p

    def upload(self, raw):
        p = self.alloc(len(raw))
        self.sa.lib.check(self.sa.L.sh_dev_upload(self.ctx, raw, p, len(raw)), "sh_dev_upload")
        return p

    def download(self, p, nbytes):
        out = ctypes.create_string_buffer(nbytes)
        self.sa.lib.check(self.sa.L.sh_dev_download(self.ctx, p, out, nbytes), "sh_dev_download")
        return out.raw

    def close(self):
        for p in self.ptrs:
            self.sa.L.sh_dev_free(self.ctx, p)
        self.ptrs = []


@pytest.fixture
def dev(sa):
    d = Dev(sa)
    yield d
    d.close()


class Shape(object):
    """One system and shape: the packed terms and the proof length."""

    def __init__(self, sa, sp, steps, ext, raw_terms=None):
        self.width, self.steps, self.ext = len(sp), steps, ext
        if raw_terms is None:
            self.coefs, self.exps, self.counts, self.degree = sa.stark.pack_step_polys([_Poly(d) for d in sp], self.width)
        else:
            self.coefs, self.exps, counts = sc.pack_terms_raw(raw_terms, self.width)
            self.counts = (ctypes.c_uint32 * self.width)(*counts)
            self.degree = max(sum(ex) for terms in raw_terms for ex, _ in terms)
        self.plen = sa.stark.proof_len(steps, ext, self.width, self.degree, SAMPLES)
        assert self.plen
        self.terms = (self.coefs, self.exps, self.counts)


def prove_host(sa, sh, wit_wire, in_wire, nb):
    """sh_stark_prove -> (status, [proof bytes per unit])"""
    out = ctypes.create_string_buffer(sh.plen * nb)
    rc = sa.L.sh_stark_prove(sa.ctx, wit_wire, in_wire, sh.steps, sh.ext, sh.width, *sh.terms, SAMPLES, nb, out, len(out))
    raw = out.raw
    return rc, [raw[u * sh.plen:(u + 1) * sh.plen] for u in range(nb)]


def prove_dev(sa, dev, sh, dw, di, nb, ctx=None):
    """sh_dev_stark_prove on device buffers -> [proof bytes per unit]; the flags are left for the caller to read."""
    dp = dev.alloc(sh.plen * nb)
    sa.lib.check(sa.L.sh_dev_stark_prove(ctx or sa.ctx, dw, di, sh.steps, sh.ext, sh.width, *sh.terms, SAMPLES, nb, dp), "sh_dev_stark_prove")
    raw = dev.download(dp, sh.plen * nb)
    return [raw[u * sh.plen:(u + 1) * sh.plen] for u in range(nb)]


def status_batch(sa, nb, ctx=None):
    flags = ctypes.create_string_buffer(nb)
    rc = sa.L.sh_stark_status_batch(ctx or sa.ctx, flags, nb)
    return rc, list(flags.raw)


def differing(got, want):
    return [u for u in range(len(want)) if got[u] != want[u]]


_expected = {}


def expected(case):
    """The oracle's proof of every unit's residues, computed once per case and never changed."""
    if case["name"] not in _expected:
        tr = sc.traces(case)
        _expected[case["name"]] = tuple(sc.oracle_unit(tr[u], case["inputs"][u], case["sp"], case["steps"], case["ext"])
                                        for u in range(case["batch"]))
    return _expected[case["name"]]


# ---- A. representatives ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.repr_cases(), ids=lambda c: c["name"])
def test_prover_gives_the_residues_proof_for_every_representative(sa, dev, case):
    want = expected(case)
    tr = sc.traces(case)
    nb = case["batch"]
    sh = Shape(sa, case["sp"], case["steps"], case["ext"])
    assert len(want[0]) == sh.plen
    for pattern in case["patterns"]:
        wit, ins = sc.stored(case, tr, pattern)
        w, i = sc.flat(wit), sc.flat(ins)
        rc, got = prove_host(sa, sh, sc.wire(w), sc.wire(i), nb)
        assert rc == 0 and not differing(got, want), ("sh_stark_prove", case["name"], pattern, rc, differing(got, want))
        assert status_batch(sa, nb) == (0, [0] * nb)
        got = prove_dev(sa, dev, sh, dev.from_wire(sc.wire(w)), dev.from_wire(sc.wire(i)), nb)
        assert status_batch(sa, nb) == (0, [0] * nb), ("from_wire", case["name"], pattern)
        assert not differing(got, want), ("from_wire", case["name"], pattern, differing(got, want))
        dw = dev.upload(sc.limbs(w))
        assert dev.download(dw, 32 * len(w)) == sc.limbs(w)  # the device really holds the unreduced limbs
        got = prove_dev(sa, dev, sh, dw, dev.upload(sc.limbs(i)), nb)
        assert status_batch(sa, nb) == (0, [0] * nb), ("upload", case["name"], pattern)
        assert not differing(got, want), ("upload", case["name"], pattern, differing(got, want))
        assert dev.download(dw, 32 * len(w)) == sc.limbs(w)  # d_witness is read only
        dev.close()


def test_prover_takes_unreduced_step_polynomial_coefficients(sa, dev):
    c = sc.COEF_CASE
    nb, steps, width = len(c["inputs"]), c["steps"], c["width"]
    tr = [sv.trace(inp, steps, c["residues"]) for inp in c["inputs"]]
    want = [sc.oracle_unit(tr[u], c["inputs"][u], c["residues"], steps, c["ext"]) for u in range(nb)]
    sh = Shape(sa, c["residues"], steps, c["ext"], raw_terms=c["raw"])
    assert sh.coefs != Shape(sa, c["residues"], steps, c["ext"]).coefs and sh.degree == 3
    in_wire = sc.wire(sc.flat(c["inputs"]))  # one of them is 2^256 - 1
    rc, got = prove_host(sa, sh, sc.wire(sc.flat(tr)), in_wire, nb)
    assert rc == 0 and not differing(got, want), (rc, differing(got, want))
    # sh_dev_stark_witness -> sh_dev_stark_prove with the same raw terms
    di = dev.from_wire(in_wire)
    dw = dev.alloc(32 * nb * width * steps)
    sa.lib.check(sa.L.sh_dev_stark_witness(sa.ctx, di, steps, width, *sh.terms, nb, dw), "sh_dev_stark_witness")
    got = prove_dev(sa, dev, sh, dw, di, nb)
    assert status_batch(sa, nb) == (0, [0] * nb)
    assert not differing(got, want), differing(got, want)
    assert dev.download(dw, 32 * nb * width * steps) == sc.limbs(sc.flat(tr)), "the generated witness is the residues' trace, canonical"
    # and the host verifier reads the same unreduced terms and inputs
    for u in range(nb):
        outs = sc.wire(col[-1] for col in tr[u])
        assert sa.L.sh_stark_verify(want[u], sh.plen, in_wire[32 * width * u:32 * width * (u + 1)], outs, steps, c["ext"], width,
                                    *sh.terms, SAMPLES) == 0


@pytest.mark.parametrize("case", sc.regime_cases(), ids=lambda c: c["name"])
def test_every_kernel_regime_on_canonical_and_unreduced_limbs(sa, dev, case):
    """narrow / middle / wide launches of the quotient and lincomb kernels, width 2 and width 3 (generic lincomb): the canonical form
    and the form with every eligible element stored as x + p, against the committed per-unit hashes of the oracle's proofs."""
    fx, = [r for r in sc.load_fixture()["regimes"] if r["name"] == case["name"]]
    (q, w), (lc, lw) = sv.regimes(case)
    assert q == lc == case["regime"]
    nb, steps = case["batch"], case["steps"]
    sh = Shape(sa, case["sp"], steps, case["ext"])
    ins = [sc.regime_inputs(case, u) for u in range(nb)]
    vals = [v for inp in ins for col in sv.trace(inp, steps, case["sp"]) for v in col]
    lifted = [v + P if v < R else v for v in vals]
    in_vals = sc.flat(ins)
    in_lifted = [v + P if v < R else v for v in in_vals]
    assert sum(v >= P for v in lifted) >= nb * steps

    def check(got, path):
        bad = [u for u in range(nb) if hashlib.sha256(got[u]).hexdigest() != fx["unit_sha256"][u]]
        assert not bad, "%s, %s: units %s of %d differ from the oracle" % (path, case["name"], bad[:16], nb)

    rc, got = prove_host(sa, sh, sc.wire(vals), sc.wire(in_vals), nb)
    assert rc == 0
    check(got, "canonical")
    rc, got = prove_host(sa, sh, sc.wire(lifted), sc.wire(in_lifted), nb)
    assert rc == 0
    check(got, "unreduced wire form")
    got = prove_dev(sa, dev, sh, dev.upload(sc.limbs(lifted)), dev.upload(sc.limbs(in_lifted)), nb)
    assert status_batch(sa, nb) == (0, [0] * nb)
    check(got, "unreduced limbs")


def _dev_verify(sa, dev, sh, proofs, d_in, d_out, io_stride):
    nb = len(proofs)
    dp = dev.upload(b"".join(proofs))
    ds = dev.alloc(4 * nb)
    sa.lib.check(sa.L.sh_dev_stark_verify(sa.ctx, dp, d_in, d_out, io_stride, sh.steps, sh.ext, sh.width, *sh.terms, SAMPLES, nb, ds),
                 "sh_dev_stark_verify")
    st = (ctypes.c_int32 * nb).from_buffer_copy(dev.download(ds, 4 * nb))
    return list(st)


@pytest.mark.parametrize("case", sc.repr_cases(), ids=lambda c: c["name"])
def test_batch_verifier_reads_unreduced_boundary_values(sa, dev, case):
    """sh_dev_stark_verify with d_inputs / d_outputs in unreduced limb form, packed (io_stride = 1) and read from an unreduced device
    witness (io_stride = steps): every status is sh_stark_verify's on the same values as unreduced wire bytes, and that is SH_OK; one
    proof with a wrong output is SH_ERR_REJECTED in both."""
    proofs = list(expected(case))
    tr = sc.traces(case)
    nb, steps, width = case["batch"], case["steps"], case["width"]
    sh = Shape(sa, case["sp"], steps, case["ext"])

    def host(ins, outs):
        return [sa.L.sh_stark_verify(proofs[u], sh.plen, sc.wire(ins[u]), sc.wire(outs[u]), steps, case["ext"], width, *sh.terms, SAMPLES)
                for u in range(nb)]

    for pattern in case["patterns"]:
        wit, ins = sc.stored(case, tr, pattern)
        outs = [[col[-1] for col in unit] for unit in wit]
        want = host(ins, outs)
        assert want == [0] * nb, (case["name"], pattern, want)
        assert _dev_verify(sa, dev, sh, proofs, dev.upload(sc.limbs(sc.flat(ins))), dev.upload(sc.limbs(sc.flat(outs))), 1) == want, pattern
        # row 0 of the witness holds the inputs' residues (in the representative the pattern chose for row 0)
        dw = dev.upload(sc.limbs(sc.flat(wit)))
        last = ctypes.c_void_p(dw.value + 32 * (steps - 1))
        assert _dev_verify(sa, dev, sh, proofs, dw, last, steps) == want, pattern
        # a wrong output in unit 1, kept in the representative class the pattern allows
        wrong = [[list(col) for col in unit] for unit in wit]
        v = (wrong[1][0][-1] + 1) % P
        wrong[1][0][-1] = v + P if v < R and pattern != "canonical" else v
        wouts = [[col[-1] for col in unit] for unit in wrong]
        want = host(ins, wouts)
        assert want == [0] + [sc.REJECTED] + [0] * (nb - 2)
        assert _dev_verify(sa, dev, sh, proofs, dev.upload(sc.limbs(sc.flat(ins))), dev.upload(sc.limbs(sc.flat(wouts))), 1) == want
        dw = dev.upload(sc.limbs(sc.flat(wrong)))
        assert _dev_verify(sa, dev, sh, proofs, dw, ctypes.c_void_p(dw.value + 32 * (steps - 1)), steps) == want
        dev.close()


# ---- B. the witness check ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", list(range(1, 10)))
def test_witness_check_flags_exactly_the_broken_units(sa, dev, width):
    t0 = time.time()
    g = sc.witness_grid(width)
    units, steps, ext, sp = g["units"], g["steps"], g["ext"], g["sp"]
    nb = len(units)
    sh = Shape(sa, sp, steps, ext)
    want_flags = [int(u["bad"]) for u in units]
    assert 0 < sum(want_flags) < nb
    wit = sc.wire(v for u in units for col in u["witness"] for v in col)
    ins = sc.wire(v for u in units for v in u["inputs"])
    valid = [i for i, u in enumerate(units) if not u["bad"]]
    oracle = {i: sc.oracle_unit(units[i]["residues"], units[i]["inputs"], sp, steps, ext) for i in valid}
    sa.L.sh_stark_status(sa.ctx)  # whatever an earlier test left unchecked is not this launch's
    t1 = time.time()
    got = prove_dev(sa, dev, sh, dev.from_wire(wit), dev.from_wire(ins), nb)
    rc, flags = status_batch(sa, nb)
    print("grid_w%d: %d units, %d flagged, %d expected; cases and oracle %.2f s, first launch %.2f s"
          % (width, nb, sum(flags), sum(want_flags), t1 - t0, time.time() - t1))
    assert flags == want_flags, [(i, units[i]["kind"], units[i]["c"], units[i]["k"]) for i in range(nb) if flags[i] != want_flags[i]][:16]
    assert rc == sc.CONSTRAINT
    assert status_batch(sa, nb) == (0, [0] * nb), "the flags are cleared by the call that reports them"
    assert not [i for i in valid if got[i] != oracle[i]], "a valid unit beside broken ones differs from the oracle"
    # the host-buffer form: -8 for the launch, the valid units' bytes all the same
    rc, got = prove_host(sa, sh, wit, ins, nb)
    assert rc == sc.CONSTRAINT and not [i for i in valid if got[i] != oracle[i]]
    # the valid units alone (the "+ p" ones among them): 0, exactly when no unit is bad
    vw = sc.wire(v for i in valid for col in units[i]["witness"] for v in col)
    vi = sc.wire(v for i in valid for v in units[i]["inputs"])
    got = prove_dev(sa, dev, sh, dev.from_wire(vw), dev.from_wire(vi), len(valid))
    assert status_batch(sa, nb) == (0, [0] * nb)
    assert got == [oracle[i] for i in valid]
    rc, got = prove_host(sa, sh, vw, vi, len(valid))
    assert rc == 0 and got == [oracle[i] for i in valid]


def test_a_broken_wrap_transition_is_no_violation(sa, dev):
    c = sc.WRAP_CASE
    tr = sc.traces(c)
    nb = len(tr)
    sh = Shape(sa, c["sp"], c["steps"], c["ext"])
    want = [sc.oracle_unit(tr[u], c["inputs"][u], c["sp"], c["steps"], c["ext"]) for u in range(nb)]
    rc, got = prove_host(sa, sh, sc.wire(sc.flat(tr)), sc.wire(sc.flat(c["inputs"])), nb)
    assert rc == 0 and got == want
    got = prove_dev(sa, dev, sh, dev.from_wire(sc.wire(sc.flat(tr))), dev.from_wire(sc.wire(sc.flat(c["inputs"]))), nb)
    assert status_batch(sa, nb) == (0, [0] * nb) and got == want


def test_witness_check_at_2_12_steps_first_and_last_transition(sa, dev):
    c = sc.SIZE_CASE
    ws = sc.size_case_units()
    sh = Shape(sa, c["sp"], c["steps"], c["ext"])
    wit, ins = sc.wire(sc.flat(ws)), sc.wire(sc.flat(c["inputs"]))
    sa.L.sh_stark_status(sa.ctx)
    got = prove_dev(sa, dev, sh, dev.from_wire(wit), dev.from_wire(ins), 3)
    assert status_batch(sa, 3) == (sc.CONSTRAINT, [1, 0, 1])
    assert status_batch(sa, 3) == (0, [0, 0, 0])
    assert hashlib.sha256(got[1]).hexdigest() == sc.load_fixture()["size_case"]["unit1_sha256"]
    # each broken transition alone, so neither flag hides the other
    for u in (0, 2):
        one = sc.wire(sc.flat([ws[u], ws[1], ws[1]]))
        prove_dev(sa, dev, sh, dev.from_wire(one), dev.from_wire(sc.wire(c["inputs"][u] + c["inputs"][1] * 2)), 3)
        assert status_batch(sa, 3) == (sc.CONSTRAINT, [1, 0, 0]), u


def test_raised_flags_survive_the_growth_of_the_flag_buffer(sa):
    """sh_dev_stark_prove of 3 units with unit 1 broken, unchecked, then a valid batch of 200 on a fresh context (whose flag buffer
    holds 64 units after the first call and has to grow): the next sh_stark_status_batch still names unit 1, and only it."""
    sp, steps, ext = sc.CONST_CUBE_2, 8, 8
    sh = Shape(sa, sp, steps, ext)
    ctx = ctypes.c_void_p()
    sa.lib.check(sa.L.sh_ctx_create(sa.lib.default_device(), ctypes.byref(ctx)), "sh_ctx_create")
    d = Dev(sa, ctx)
    try:
        ins = [[5 + u, 1000 + 7 * u] for u in range(200)]
        tr = [sv.trace(i, steps, sp) for i in ins]
        small = [[list(col) for col in w] for w in tr[:3]]
        small[1][1][4] = (small[1][1][4] + 1) % P
        prove_dev(sa, d, sh, d.from_wire(sc.wire(sc.flat(small))), d.from_wire(sc.wire(sc.flat(ins[:3]))), 3, ctx=ctx)
        got = prove_dev(sa, d, sh, d.from_wire(sc.wire(sc.flat(tr))), d.from_wire(sc.wire(sc.flat(ins))), 200, ctx=ctx)
        assert status_batch(sa, 200, ctx=ctx) == (sc.CONSTRAINT, [0, 1] + [0] * 198)
        assert status_batch(sa, 200, ctx=ctx) == (0, [0] * 200)
        for u in (0, 1, 64, 199):
            assert got[u] == sc.oracle_unit(tr[u], ins[u], sp, steps, ext), u
    finally:
        d.close()
        sa.L.sh_ctx_destroy(ctx)


def test_row_0_that_is_not_the_inputs_proves_with_status_ok_and_is_rejected_by_both_verifiers(sa, dev):
    """The reference asserts nothing about witness[dim][0] against the boundary inputs (its prover's only asserts are stark.py:71 and :75)
    and emits a proof its own verifier rejects.  Here: the prover's status is SH_OK (the constraint check reads the witness alone), and
    sh_stark_verify and sh_dev_stark_verify both reject what it produced.  Nothing is claimed about the proof bytes."""
    sp, steps, ext = sc.CONST_CUBE_2, 32, 8
    sh = Shape(sa, sp, steps, ext)
    ins = [[42, 3], [42, 3], [7, 9]]
    given = [[42, 3], [42, 4], [8, 9]]  # unit 0 honest; unit 1: the cubed column's input is wrong; unit 2: the constant's
    tr = [sv.trace(i, steps, sp) for i in ins]
    rc, proofs = prove_host(sa, sh, sc.wire(sc.flat(tr)), sc.wire(sc.flat(given)), 3)
    print("sh_stark_prove with row 0 != inputs: status %d" % rc)
    assert rc == 0
    assert status_batch(sa, 3) == (0, [0, 0, 0])
    outs = [[col[-1] for col in w] for w in tr]
    host = [sa.L.sh_stark_verify(proofs[u], sh.plen, sc.wire(given[u]), sc.wire(outs[u]), steps, ext, 2, *sh.terms, SAMPLES) for u in range(3)]
    assert host == [0, sc.REJECTED, sc.REJECTED]
    assert _dev_verify(sa, dev, sh, proofs, dev.upload(sc.limbs(sc.flat(given))), dev.upload(sc.limbs(sc.flat(outs))), 1) == host
    assert proofs[0] == sc.oracle_unit(tr[0], ins[0], sp, steps, ext)
