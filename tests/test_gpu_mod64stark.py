"""STARK proofs over any prime modulus below 2^64 on packed 64-bit words (sh_mod64_stark_prove, sh_dev_mod64_stark_prove:
starks_amd/csrc/mod64stark_items.cuh, mod64stark.hip, api_mod64stark.hip) on the MI355X: the whole grid of tests/mod64stark_cases.py
against the exact oracle (oracle/pyoracle.py with p = the modulus), byte for byte; the device form and its per-proof flags; the generic
prover sh_dev_mod_stark_prove as yardstick at sizes that leave the serial tree form and reach multi-workgroup transforms; the generic
verifiers on packed proofs; two contexts; packed and generic calls alternating on one context; the Python call sites; the errors.
Every refused call is refused on the host."""
import ctypes
import random

import pytest

import mod64stark_cases as m6
import modntt_cases as mc
import ntt64_cases as nc
from mod64stark_cases import MODULI
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
    """step polynomials as {exponent tuple: coefficient} per dimension -> (coefs, exps, counts) as the C entries take them"""
    counts, coefs, exps = [], [], bytearray()
    for poly in sp:
        items = sorted(poly.items())
        counts.append(len(items))
        for k, c in items:
            coefs.append(c % p)
            exps += bytes(k)
    return wire(coefs), bytes(exps), (ctypes.c_uint32 * len(sp))(*counts)


def case_terms(c):
    counts, coefs, exps = c.terms()  # as the case stores them: plus-p coefficients included
    return wire(coefs), exps, (ctypes.c_uint32 * c.width)(*counts)


def plen_of(L, steps, ext, sp, samples=80):
    plen = L.sh_stark_proof_len(steps, ext, len(sp), m6.sc.degree_of(sp), samples)
    assert plen
    return plen


def prove_raw(L, p, wit_words, in_words, steps, ext, sp, samples=80, batch=1, terms=None, ctx=None):
    """sh_mod64_stark_prove -> the batch's flat proofs"""
    coefs, exps, counts = terms or term_args(sp, p)
    plen = plen_of(L, steps, ext, sp, samples)
    out = ctypes.create_string_buffer(plen * batch)
    ctx = ctx or _ctx()
    rc = L.sh_mod64_stark_prove(ctx, p, wit_words, in_words, steps, ext, len(sp), coefs, exps, counts, samples, batch, out, plen * batch)
    assert rc == OK, (rc, L.sh_last_error(ctx))
    return out.raw


def prove(L, c, ctx=None):
    return prove_raw(L, c.p, c.witness_words(), c.input_words(), c.steps, c.ext, c.sp, c.samples, c.batch, case_terms(c), ctx)


def generic_prove(L, c):
    """sh_mod_stark_prove on the same stored values"""
    coefs, exps, counts = case_terms(c)
    plen = plen_of(L, c.steps, c.ext, c.sp, c.samples)
    out = ctypes.create_string_buffer(plen * c.batch)
    rc = L.sh_mod_stark_prove(_ctx(), b32(c.p), c.witness_wire(), c.input_wire(), c.steps, c.ext, c.width, coefs, exps, counts, c.samples,
                              c.batch, out, plen * c.batch)
    assert rc == OK, (rc, L.sh_last_error(_ctx()))
    return out.raw


class Dev(object):
    """device buffers of one context, freed together"""

    def __init__(self, L, ctx):
        self.L, self.ctx, self.ptrs = L, ctx, []

    def alloc(self, nbytes, data=None):
        p = ctypes.c_void_p()
        assert self.L.sh_dev_alloc(self.ctx, nbytes, ctypes.byref(p)) == OK
        self.ptrs.append(p)
        if data is not None:
            assert len(data) == nbytes and self.L.sh_dev_upload(self.ctx, data, p, nbytes) == OK
        return p

    def get(self, p, nbytes):
        out = ctypes.create_string_buffer(nbytes)
        assert self.L.sh_dev_download(self.ctx, p, out, nbytes) == OK
        return out.raw

    def free(self):
        assert self.L.sh_sync(self.ctx) == OK
        for p in self.ptrs:
            self.L.sh_dev_free(self.ctx, p)
        self.ptrs = []


def dev_prove(L, dev, p, wit_words, in_words, steps, ext, sp, samples, batch, terms):
    """sh_dev_mod64_stark_prove on uploaded words -> (d_proof, bytes per batch); nothing is synchronised here"""
    plen = plen_of(L, steps, ext, sp, samples)
    dw, di, dp = dev.alloc(len(wit_words), wit_words), dev.alloc(len(in_words), in_words), dev.alloc(plen * batch)
    rc = L.sh_dev_mod64_stark_prove(dev.ctx, p, dw, di, steps, ext, len(sp), terms[0], terms[1], terms[2], samples, batch, dp)
    assert rc == OK, (rc, L.sh_last_error(dev.ctx))
    return dp, plen * batch


def mvpolys(p, sp):
    from starks_amd import IntegersModP
    from starks_amd.multivariate_polynomial import multivariates_over
    F = IntegersModP(p)
    mv = multivariates_over(F, len(sp)).factory
    return [mv({k: F(v) for k, v in d.items()}) for d in sp]


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(L, name):
    """every case of the modulus through sh_mod64_stark_prove equals the oracle's flat proof byte for byte"""
    cases = [c for c in m6.GRID if c.name == name]
    assert cases
    for c in cases:
        assert prove(L, c) == m6.oracle_flat(c), c.id


def test_top_bit(L):
    """X' = X^3 from p - 1 over BIG18: every P value in every opened leaf is p - 1, a word with its top bit set"""
    c = m6.BIG18_CONST
    got = prove(L, c)
    assert got == m6.oracle_flat(c)
    opened = m6.opened_p_values(got, c)
    assert set(opened) == {m6.BIG18 - 1} and all(v >> 63 for v in opened)


# ---- 2. the device form and the flags ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["goldilocks-s32-b3-s7", "big18-s8-b3-s80", "f257-s32-b1-s80-plusp", "big18-s8w9-b1-s80"])
def test_device_form_equals_host_form(L, cid):
    c = m6._BY_ID[cid]
    dev = Dev(L, _ctx())
    try:
        dp, nbytes = dev_prove(L, dev, c.p, c.witness_words(), c.input_words(), c.steps, c.ext, c.sp, c.samples, c.batch, case_terms(c))
        assert L.sh_stark_status(dev.ctx) == OK
        got = dev.get(dp, nbytes)
    finally:
        dev.free()
    assert got == prove(L, c) == m6.oracle_flat(c)


def test_device_form_names_the_broken_proofs(L):
    """a mixed batch through sh_dev_mod64_stark_prove: sh_stark_status_batch names exactly the broken proofs, the valid ones keep their
    bytes, the witness is not modified, the host-buffer form returns SH_ERR_CONSTRAINT, and the context proves correctly afterwards"""
    base = m6.BREAK_BASE
    units, want = m6.broken_witnesses()
    units, want = units + [units[0]], want + [0]
    batch, ctx = len(units), _ctx()
    words = nc.words([v for w in units for col in w for v in col])
    inw = nc.words(base.inputs[0]) * batch
    terms = term_args(base.sp, base.p)
    plen = m6.proof_len(base)
    dev = Dev(L, ctx)
    try:
        assert L.sh_stark_status(ctx) in (OK, CONSTRAINT)  # drop what earlier tests may have left
        dw, di, dp = dev.alloc(len(words), words), dev.alloc(len(inw), inw), dev.alloc(plen * batch)
        rc = L.sh_dev_mod64_stark_prove(ctx, base.p, dw, di, base.steps, base.ext, base.width, terms[0], terms[1], terms[2], 80, batch, dp)
        assert rc == OK, (rc, L.sh_last_error(ctx))
        bad = ctypes.create_string_buffer(batch)
        assert L.sh_stark_status_batch(ctx, bad, batch) == CONSTRAINT
        assert list(bad.raw) == want
        assert L.sh_stark_status(ctx) == OK  # the flags are dropped once reported
        out = dev.get(dp, plen * batch)
        assert out[:plen] == m6.oracle_flat(base) == out[-plen:]
        assert dev.get(dw, len(words)) == words  # the witness is not modified
    finally:
        dev.free()
    out = ctypes.create_string_buffer(plen)
    w1 = nc.words([v for col in units[1] for v in col])
    assert L.sh_mod64_stark_prove(ctx, base.p, w1, base.input_words(), base.steps, base.ext, base.width, terms[0], terms[1], terms[2], 80, 1,
                                  out, plen) == CONSTRAINT
    c = m6._BY_ID["goldilocks-s32-b1-s80"]
    assert prove(L, c) == m6.oracle_flat(c)


# ---- 3. the generic prover as yardstick -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["goldilocks", "big18"])
@pytest.mark.parametrize("steps,ext,sp,batch", [(1 << 10, 8, m6.MIMC_2, 3), (1 << 13, 8, m6.MIMC_2, 1), (8, 8, m6.QUINTIC_9, 2)],
                         ids=["s1024-b3", "s8192-b1", "s8-w9"])
def test_equals_the_generic_device_prover(L, name, steps, ext, sp, batch):
    """sh_dev_mod64_stark_prove equals sh_dev_mod_stark_prove byte for byte on the same values (the existing suite pins the latter to the
    oracle): 3 x 2^13 and 2^16 domain points leave the serial tree form (the latter in the wide form) and reach transforms of several
    workgroups and two passes; width 9 in a batch"""
    p, width, ctx = MODULI[name], len(sp), _ctx()
    rnd = random.Random("%s-%d" % (name, steps))
    inputs = [[rnd.randrange(p) for _ in range(width)] for _ in range(batch)]
    vals = [v for inp in inputs for col in pyoracle.get_computational_trace(inp, steps, sp, p) for v in col]
    flat_in = [v for inp in inputs for v in inp]
    terms = term_args(sp, p)
    plen = plen_of(L, steps, ext, sp)
    dev = Dev(L, ctx)
    try:
        assert L.sh_stark_status(ctx) in (OK, CONSTRAINT)
        gw, gi, gp = dev.alloc(32 * len(vals), nc.limbs(vals)), dev.alloc(32 * len(flat_in), nc.limbs(flat_in)), dev.alloc(plen * batch)
        rc = L.sh_dev_mod_stark_prove(ctx, b32(p), gw, gi, steps, ext, width, terms[0], terms[1], terms[2], 80, batch, gp)
        assert rc == OK, (rc, L.sh_last_error(ctx))
        pp, nbytes = dev_prove(L, dev, p, nc.words(vals), nc.words(flat_in), steps, ext, sp, 80, batch, terms)
        assert L.sh_stark_status(ctx) == OK
        want, got = dev.get(gp, plen * batch), dev.get(pp, nbytes)
    finally:
        dev.free()
    assert nbytes == plen * batch and got == want


# ---- 4. the generic verifiers take the packed proofs ---------------------------------------------------------------------------------------
def test_generic_verifiers_accept(L):
    """every proof of a batched case is accepted by sh_mod_stark_verify and sh_mod_stark_verify_batch; one flipped byte is rejected"""
    from starks_amd import stark
    c = m6._BY_ID["big18-s8-b3-s80"]
    flat, plen = prove(L, c), m6.proof_len(c)
    polys = mvpolys(c.p, c.sp)
    wits = c.witnesses()
    ins = [wire(inp) for inp in c.inputs]
    outs = [wire([col[-1] for col in w]) for w in wits]
    for b in range(c.batch):
        assert stark.mod_verify_flat(c.p, flat[b * plen:(b + 1) * plen], ins[b], outs[b], c.steps, c.ext, c.width, polys)
    assert stark.mod_verify_flat_batch(c.p, flat, b"".join(ins), b"".join(outs), c.steps, c.ext, c.width, polys, c.batch) == [True] * 3
    k = plen + 64 + 5  # inside the first opened leaf of proof 1
    broken = flat[:k] + bytes([flat[k] ^ 1]) + flat[k + 1:]
    with pytest.raises(AssertionError):
        stark.mod_verify_flat(c.p, broken[plen:2 * plen], ins[1], outs[1], c.steps, c.ext, c.width, polys)
    assert stark.mod_verify_flat_batch(c.p, broken, b"".join(ins), b"".join(outs), c.steps, c.ext, c.width, polys, c.batch) == \
        [True, False, True]


# ---- 5. contexts and interleaving ---------------------------------------------------------------------------------------------------------
def test_two_moduli_on_two_contexts(L):
    """Goldilocks on one context and BIG18 on another, enqueued back to back with no synchronisation in between: each proof equals the
    bytes of its run alone (a modulus kept in a device global fails here)"""
    from starks_amd import _lib
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    cases = [m6._BY_ID["goldilocks-s32-b1-s80"], m6._BY_ID["big18-s32-b1-s80"]]
    want = [m6.oracle_flat(c) for c in cases]
    assert [prove(L, c, ctx) for c, ctx in zip(cases, ctxs)] == want
    devs = [Dev(L, ctx) for ctx in ctxs]
    try:
        held = []
        for _ in range(4):
            for c, dev in zip(cases, devs):
                held.append(dev_prove(L, dev, c.p, c.witness_words(), c.input_words(), c.steps, c.ext, c.sp, c.samples, c.batch,
                                      case_terms(c)))
        for ctx in ctxs:
            assert L.sh_sync(ctx) == OK and L.sh_stark_status(ctx) == OK
        for k, (dp, nbytes) in enumerate(held):
            assert devs[k % 2].get(dp, nbytes) == want[k % 2], k
    finally:
        for dev in devs:
            dev.free()


def test_alternating_with_the_generic_prover(L):
    """packed and generic provers take turns on one context over the same system: both keep producing the oracle's bytes (each has
    its own term image), and a second system over another modulus in between disturbs neither"""
    c = m6._BY_ID["goldilocks-s8-b1-s80"]
    want = m6.oracle_flat(c)
    for _ in range(3):
        assert prove(L, c) == want
        assert generic_prove(L, c) == want
    g = m6._BY_ID["big18-s32-b1-s80"]
    assert prove(L, g) == m6.oracle_flat(g) and generic_prove(L, c) == want
    assert generic_prove(L, g) == m6.oracle_flat(g) and prove(L, c) == want


# ---- 6. the Python call sites ------------------------------------------------------------------------------------------------------------
def test_python_call_sites(L):
    from starks_amd import stark
    c = m6._BY_ID["big18-s8-b3-s80"]
    polys = mvpolys(c.p, c.sp)
    want = stark.mod_prove_flat(c.p, c.witness_wire(), c.input_wire(), c.steps, c.ext, c.width, polys, c.batch)
    assert want == m6.oracle_flat(c)
    assert stark.mod64_prove_flat(c.p, c.witness_words(), c.input_words(), c.steps, c.ext, c.width, polys, c.batch) == want
    ints = [v for inp in c.inputs for v in inp]
    assert stark.mod64_prove_flat(c.p, [v for w in c.witnesses() for col in w for v in col], ints, c.steps, c.ext, c.width, polys,
                                  c.batch) == want
    proofs, outputs = stark.mod64_prove_inputs_flat(c.p, c.input_wire(), c.steps, c.ext, c.width, polys, c.batch)
    assert (proofs, outputs) == stark.mod_prove_inputs_flat(c.p, c.input_wire(), c.steps, c.ext, c.width, polys, c.batch)
    assert proofs == want and outputs == wire([col[-1] for w in c.witnesses() for col in w])
    with pytest.raises(ValueError):
        stark.mod64_prove_flat(c.p, c.witness_words()[8:], c.input_words(), c.steps, c.ext, c.width, polys, c.batch)
    with pytest.raises(AssertionError):  # a broken witness: the reference's `assert cp % z == 0`
        b = m6.BREAK_BASE
        stark.mod64_prove_flat(b.p, [v for col in m6.broken_witnesses()[0][3] for v in col], b.inputs[0], b.steps, b.ext, b.width,
                               mvpolys(b.p, b.sp))


# ---- 7. the errors -----------------------------------------------------------------------------------------------------------------------
def test_refusals(L):
    """every refusal returns its status with the entry's name in sh_last_error; the buffers are far too small for the refused shapes, so
    a call that got as far as reading them would be seen; after each refusal the context still proves"""
    ctx, c = _ctx(), m6.BREAK_BASE
    coefs, exps, counts = term_args(c.sp, c.p)
    cub = term_args(m6.CUBIC_1, c.p)
    none = (coefs, exps, (ctypes.c_uint32 * 2)(0, 0))
    many = (bytes(32 * 257), bytes(2 * 257), (ctypes.c_uint32 * 2)(257, 0))
    wit, inp, plen = c.witness_words(), c.input_words(), m6.proof_len(c)
    out = ctypes.create_string_buffer(plen)
    want_bytes = m6.oracle_flat(c)

    def host(p=c.p, steps=8, ext=8, width=2, terms=(coefs, exps, counts), samples=80, batch=1, cap=plen, w=wit, i=inp, o=out):
        rc = L.sh_mod64_stark_prove(ctx, p, w, i, steps, ext, width, terms[0], terms[1], terms[2], samples, batch, o, cap)
        return rc, L.sh_last_error(ctx).decode()

    assert host()[0] == OK and out.raw == want_bytes
    table = [
        (dict(p=1 << 32), INVALID), (dict(p=1), INVALID), (dict(p=0), INVALID),
        (dict(w=None), INVALID), (dict(i=None), INVALID), (dict(o=None), INVALID), (dict(terms=(None, exps, counts)), INVALID),
        (dict(terms=(coefs, None, counts)), INVALID), (dict(terms=(coefs, exps, None)), INVALID),
        (dict(width=0), INVALID), (dict(batch=0), INVALID), (dict(terms=none), INVALID),
        (dict(width=10), UNSUPPORTED), (dict(batch=65536), UNSUPPORTED), (dict(terms=many), UNSUPPORTED),
        (dict(steps=12), INVALID), (dict(steps=1), INVALID), (dict(ext=1), INVALID), (dict(ext=6), INVALID), (dict(samples=0), INVALID),
        (dict(steps=1 << 21, ext=8), UNSUPPORTED), (dict(steps=16, ext=2, width=1, terms=cub), UNSUPPORTED),
        (dict(p=m6.BABYBEAR), ROOT_ORDER), (dict(p=m6.KOALABEAR), ROOT_ORDER), (dict(p=3), ROOT_ORDER),
        (dict(p=m6.P64_59, steps=2, ext=8), ROOT_ORDER), (dict(p=m6.BIG18, steps=1 << 16, ext=8), ROOT_ORDER),
        (dict(p=65537, steps=1 << 10, ext=1 << 7), ROOT_ORDER),  # 2-adicity 16 < 17
        (dict(cap=plen - 1), TOO_SMALL), (dict(batch=2), TOO_SMALL),
        (dict(samples=1 << 26, batch=65535), UNSUPPORTED),  # the gather-size limit: 2^39 32-byte values or more
    ]
    for kw, want in table:
        rc, text = host(**kw)
        assert rc == want and text.startswith("sh_mod64_stark_prove: "), (kw, rc, text)
        assert host()[0] == OK and out.raw == want_bytes, kw
    d = ctypes.c_void_p()
    assert L.sh_dev_alloc(ctx, 4096, ctypes.byref(d)) == OK
    try:
        for kw, want in ((dict(p=1 << 32), INVALID), (dict(p=m6.BABYBEAR), ROOT_ORDER), (dict(steps=12), INVALID), (dict(batch=0), INVALID),
                         (dict(batch=65536), UNSUPPORTED), (dict(width=10), UNSUPPORTED), (dict(wit=None), INVALID)):
            a = dict(p=c.p, steps=8, ext=8, width=2, batch=1, wit=d)
            a.update(kw)
            rc = L.sh_dev_mod64_stark_prove(ctx, a["p"], a["wit"], d, a["steps"], a["ext"], a["width"], coefs, exps, counts, 80, a["batch"], d)
            assert rc == want and L.sh_last_error(ctx).decode().startswith("sh_dev_mod64_stark_prove: "), (kw, rc)
    finally:
        L.sh_dev_free(ctx, d)
    assert host()[0] == OK and out.raw == want_bytes
