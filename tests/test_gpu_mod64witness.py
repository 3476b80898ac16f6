"""STARK witnesses generated on the MI355X on packed 64-bit words over any odd modulus below 2^64 (sh_mod64_stark_witness,
sh_dev_mod64_stark_witness: starks_amd/csrc/mod64witness_items.cuh, mod64witness.hip, api_mod64stark.hip): the whole grid of
tests/mod64witness_cases.py against the exact oracle (oracle/pyoracle.py with p = the modulus, pinned to the reference by
tests/golden/mod64_witness.json), word for word, in the host and the device form; the generic generator followed by
sh_dev_mod64_from_limbs as yardstick; partial waves, slice boundaries and a trace that crosses default slices; every group x slice
decomposition and the other store form in child processes; the device-resident chain generate -> prove -> verify on words; two
contexts with different moduli at once; interleaving with the other two generators; the errors."""
import ctypes
import json
import os
import re
import subprocess
import sys
import threading

import pytest

import mod64stark_cases as m6
import mod64witness_cases as wc
import stark_variants as sv
from conftest import ROOT, load_golden
from modntt_cases import wire

pytestmark = pytest.mark.gpu

OK, INVALID, TOO_SMALL, UNSUPPORTED = 0, -1, -5, -6
with open(os.path.join(ROOT, "starks_amd", "csrc", "mod64witness_items.cuh")) as _fh:
    SLICE_PRODUCTS = 1 << int(re.search(r"M6W_SLICE_PRODUCTS = 1u << (\d+);", _fh.read()).group(1))


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


def _polys(sp):
    return [_Poly(d) for d in sp]


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


def _args(c):
    coefs, exps, counts = c.terms()
    return coefs, exps, (ctypes.c_uint32 * c.width)(*counts)


class Dev(object):
    """device buffers of one test, freed together"""

    def __init__(self, L, ctx=None):
        self.L, self.ctx, self.ptrs = L, ctx or _ctx(), []

    def alloc(self, nbytes, data=None):
        p = ctypes.c_void_p()
        assert self.L.sh_dev_alloc(self.ctx, max(nbytes, 8), ctypes.byref(p)) == OK
        self.ptrs.append(p)
        if data is not None:
            assert self.L.sh_dev_upload(self.ctx, data, p, len(data)) == OK
        return p

    def get(self, p, nbytes):
        out = ctypes.create_string_buffer(nbytes)
        assert self.L.sh_dev_download(self.ctx, p, out, nbytes) == OK
        return out.raw

    def free(self):
        assert self.L.sh_sync(self.ctx) == OK
        for p in self.ptrs:
            self.L.sh_dev_free(self.ctx, p)


def host_form(L, c, ctx=None):
    """sh_mod64_stark_witness on a Case, words and coefficients as the case stores them -> the witness words"""
    ctx = ctx or _ctx()
    coefs, exps, counts = _args(c)
    count = c.batch * c.width * c.steps
    out = ctypes.create_string_buffer(8 * count)
    rc = L.sh_mod64_stark_witness(ctx, c.p, c.input_words(), c.steps, c.width, coefs, exps, counts, c.batch, out, count)
    assert rc == OK, (c.id, rc, L.sh_last_error(ctx))
    return out.raw


def device_form(L, c, yardstick=False):
    """sh_dev_mod64_stark_witness from uploaded words -> the downloaded words; with `yardstick` also sh_dev_mod_stark_witness on the
    zero-extended inputs followed by sh_dev_mod64_from_limbs -> (words, yardstick words)"""
    ctx = _ctx()
    coefs, exps, counts = _args(c)
    count = c.batch * c.width * c.steps
    d = Dev(L)
    try:
        di, dw = d.alloc(8 * c.batch * c.width, c.input_words()), d.alloc(8 * count)
        rc = L.sh_dev_mod64_stark_witness(ctx, c.p, di, c.steps, c.width, coefs, exps, counts, c.batch, dw)
        assert rc == OK, (c.id, rc, L.sh_last_error(ctx))
        got = d.get(dw, 8 * count)
        if not yardstick:
            return got
        dl, dwl, dww = d.alloc(32 * c.batch * c.width, c.input_limbs()), d.alloc(32 * count), d.alloc(8 * count)
        rc = L.sh_dev_mod_stark_witness(ctx, b32(c.p), dl, c.steps, c.width, coefs, exps, counts, c.batch, dwl)
        assert rc == OK, (c.id, rc, L.sh_last_error(ctx))
        assert L.sh_dev_mod64_from_limbs(ctx, c.p, dwl, dww, count) == OK, L.sh_last_error(ctx)
        return got, d.get(dww, 8 * count)
    finally:
        d.free()


# ---- 1, 2. the grid, both forms; the generic generator as yardstick ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wc.MODULI))
def test_grid_host_form(L, name):
    cases = [c for c in wc.GRID if c.name == name]
    assert cases
    for c in cases:
        assert host_form(L, c) == wc.want_words(c), c.id


@pytest.mark.parametrize("name", sorted(wc.MODULI))
def test_grid_device_form(L, name):
    """the device form equals the oracle, and sh_dev_mod_stark_witness on the zero-extended inputs followed by sh_dev_mod64_from_limbs
    gives the same words (every modulus of the grid is below 2^64)"""
    for c in [c for c in wc.GRID if c.name == name]:
        got, generic = device_form(L, c, yardstick=True)
        assert got == wc.want_words(c), c.id
        assert generic == got, c.id


def test_fixture(L):
    G = load_golden("mod64_witness.json")["cases"]
    for key, (name, sp, steps, inputs) in wc.FIXTURE.items():
        got = host_form(L, wc.Case(name, "fixture-" + key, sp, steps, [inputs]))
        assert wc.sha(got) == G[key]["sha256"] and wc.ints(got)[steps - 1::steps] == G[key]["last"], key


# ---- 3. partial waves, G > 1, groups that exit whole ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 65, 130])
def test_batches(L, nb):
    v = [x for x in load_golden("stark_variants.json")["cases"] if x["name"] == "w5_middle"][0]
    p = wc.GOLDILOCKS
    c = wc.Case("goldilocks", "w5_middle-b%d" % nb, sv.step_polys(v), 40, [[x % p for x in sv.unit_inputs(v, u)] for u in range(nb)])
    want = b"".join(wc.trace_words(p, u, 40, c.sp) for u in c.inputs)
    assert host_form(L, c) == want


# ---- 4. decompositions and slice boundaries in child processes, one at a time --------------------------------------------------------------
_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %(root)r)
from starks_amd import stark
out = []
for p, inputs, steps, width, sp in json.loads(sys.stdin.read()):
    class Q(object):
        pass
    polys = []
    for d in sp:
        q = Q()
        q.coefficients = {tuple(k): v for k, v in d}
        polys.append(q)
    out.append(hashlib.sha256(stark.mod64_witness_flat(p, inputs, steps, width, polys, batch=len(inputs) // width)).hexdigest())
print(json.dumps(out))
"""


def _job(p, ins, steps, sp):
    return (p, [v for u in ins for v in u], steps, len(sp), [[[list(k), v % p] for k, v in sorted(d.items())] for d in sp])


def _decomposition_jobs():
    """two fixture systems, the width-3 system one step shorter than, as long as and one step longer than the slices 3 and 64 (inputs
    at or above p among them), and three units of the 256-term system at 70 steps; over goldilocks, big18 and 2^64 - 1"""
    gl, big, ones = wc.GOLDILOCKS, wc.BIG18, wc.ALL_ONES
    jobs = [_job(big, [[2, 5]], 64, wc.MIMC_2), _job(gl, [[3, 4, 5]], 64, wc.MIXED_3)]
    for i, steps in enumerate((2, 3, 4, 63, 64, 65)):
        jobs.append(_job((gl, big, ones)[i % 3], [[5, 6, 7], [ones, 0, ones - 1]], steps, wc.MIXED_3))
    jobs.append(_job(gl, [[v % gl for v in u] for u in wc.W9_INPUTS], 70, wc.W9_256))
    jobs.append(_job(ones, [[v % ones for v in u] for u in wc.W9_INPUTS], 70, wc.W9_256))
    return jobs


def _want_sha(jobs):
    return [wc.sha(b"".join(wc.trace_words(p, ins[u * w:(u + 1) * w], steps, [{tuple(k): v for k, v in d} for d in sp])
                            for u in range(len(ins) // w))) for p, ins, steps, w, sp in jobs]


def _child(env_extra, jobs):
    env = dict(os.environ)
    for k in ("STARKHIP_WITNESS_GROUP", "STARKHIP_WITNESS_SLICE", "STARKHIP_WITNESS_STORE"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}], input=json.dumps(jobs), capture_output=True, text=True, env=env,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def default_run(L):
    """the default run's SHA-256 per job, in this process; it equals the oracle's"""
    from starks_amd import stark
    jobs = _decomposition_jobs()
    got = [wc.sha(stark.mod64_witness_flat(p, ins, steps, w, _polys([{tuple(k): v for k, v in d} for d in sp]), batch=len(ins) // w))
           for p, ins, steps, w, sp in jobs]
    assert got == _want_sha(jobs)
    return jobs, got


@pytest.mark.parametrize("sl", [3, 64])
def test_traces_around_a_slice(default_run, sl):
    """traces of slice - 1, slice and slice + 1 steps under a forced slice (the job list holds 2, 3, 4, 63, 64 and 65 steps)"""
    jobs, want = default_run
    assert _child({"STARKHIP_WITNESS_SLICE": str(sl)}, jobs) == want


@pytest.mark.parametrize("g,sl", [(1, 1), (2, 3), (4, 64), (8, 1), (16, 3), (16, 64)])
def test_alternate_decompositions(default_run, g, sl):
    jobs, want = default_run
    assert _child({"STARKHIP_WITNESS_GROUP": str(g), "STARKHIP_WITNESS_SLICE": str(sl)}, jobs) == want


def test_the_other_store_form(default_run):
    """both values of STARKHIP_WITNESS_STORE give the same words, also with a dispatch per step in groups of 4"""
    jobs, want = default_run
    for form in ("inline", "pass"):
        assert _child({"STARKHIP_WITNESS_STORE": form}, jobs) == want, form
        assert _child({"STARKHIP_WITNESS_STORE": form, "STARKHIP_WITNESS_SLICE": "1", "STARKHIP_WITNESS_GROUP": "4"}, jobs) == want, form


@pytest.mark.parametrize("group", ["1", "2"])
def test_heavy_steps(L, group):
    """HEAVY (256 terms, exponents 255) over BIG18 under groups 1 and 2: the longest step a system can have, launched in the slices the
    budget allows (one step per dispatch where a step exceeds it); the trace ends and equals the oracle"""
    c = wc.HEAVY_CASE
    job = [_job(c.p, c.inputs, c.steps, c.sp)]
    assert _child({"STARKHIP_WITNESS_GROUP": group}, job) == [wc.sha(wc.want_words(c))]


# ---- 5. one long trace -----------------------------------------------------------------------------------------------------------------------
def test_long_mimc_trace_crosses_default_slices(L):
    """3 units of MiMC over two default slice boundaries: a default slice is M6W_SLICE_PRODUCTS // 2 steps"""
    p, steps = wc.GOLDILOCKS, 2 * (SLICE_PRODUCTS // 2) + 5
    c = wc.Case("goldilocks", "mimc2-long", wc.MIMC_2, steps, [[42 + u, 3 + u] for u in range(3)])
    assert host_form(L, c) == b"".join(wc.trace_words(p, u, steps, wc.MIMC_2) for u in c.inputs)


# ---- 6. generate -> prove -> verify on words --------------------------------------------------------------------------------------------------
def _verify(L, c, flat, input_words, plen):
    """sh_dev_mod_stark_verify on the proofs, inputs and outputs read from the regenerated witness through sh_dev_mod64_to_limbs"""
    ctx = _ctx()
    counts, coefs, exps = c.terms()
    coefs, counts = wire(coefs), (ctypes.c_uint32 * c.width)(*counts)
    count = c.batch * c.width * c.steps
    d = Dev(L)
    try:
        di, dw, dl = d.alloc(8 * c.batch * c.width, input_words), d.alloc(8 * count), d.alloc(32 * count)
        dp, ds = d.alloc(len(flat), flat), d.alloc(4 * c.batch)
        assert L.sh_dev_mod64_stark_witness(ctx, c.p, di, c.steps, c.width, coefs, exps, counts, c.batch, dw) == OK, L.sh_last_error(ctx)
        assert L.sh_dev_mod64_to_limbs(ctx, dw, dl, count) == OK, L.sh_last_error(ctx)
        last = ctypes.c_void_p(dl.value + 32 * (c.steps - 1))
        assert L.sh_dev_mod_stark_verify(ctx, b32(c.p), dp, dl, last, c.steps, c.steps, c.ext, c.width, coefs, exps, counts, c.samples,
                                         c.batch, ds) == OK, L.sh_last_error(ctx)
        return list((ctypes.c_int32 * c.batch).from_buffer_copy(d.get(ds, 4 * c.batch)))
    finally:
        d.free()


@pytest.mark.parametrize("name", sorted(m6.MODULI))
def test_chain_grid(L, name):
    """every small grid case of the packed prover from its input words alone: the flat proofs equal the oracle's and
    mod64_prove_inputs_flat's on the same values, the outputs are the traces' last rows, the device verifier accepts each proof, and
    sh_stark_status is SH_OK"""
    from starks_amd import stark
    assert L.sh_stark_status(_ctx()) in (OK, -8)  # drop what earlier tests may have left
    cases = [c for c in m6.GRID if c.name == name and c.n <= 256 and c.batch <= 3]
    assert cases
    for c in cases:
        want = m6.oracle_flat(c)
        flat, outs = stark.mod64_prove_input_words_flat(c.p, c.input_words(), c.steps, c.ext, c.width, _polys(c.sp), batch=c.batch,
                                                        samples=c.samples)
        assert flat == want, c.id
        last = [col[-1] for w in c.witnesses() for col in w]
        assert outs == wc.words(last), c.id
        assert L.sh_stark_status(_ctx()) == OK, c.id
        flat2, outs2 = stark.mod64_prove_inputs_flat(c.p, c.input_wire(), c.steps, c.ext, c.width, _polys(c.sp), batch=c.batch,
                                                     samples=c.samples)
        assert flat2 == flat and outs2 == wire(last), c.id
        assert _verify(L, c, flat, c.input_words(), len(flat) // c.batch) == [0] * c.batch, c.id
        assert L.sh_stark_status(_ctx()) == OK, c.id


# ---- 7. two contexts, two moduli, two host threads ---------------------------------------------------------------------------------------------
def test_two_contexts_at_once(L):
    from starks_amd import _lib
    gl, big = wc.GOLDILOCKS, wc.BIG18
    five = [sv.unit_inputs([x for x in load_golden("stark_variants.json")["cases"] if x["name"] == "w9_256_terms"][0], u) for u in range(5)]
    a = wc.Case("goldilocks", "w9-two-ctx", wc.W9_256, 300, [[v % gl for v in u] for u in five])
    b = wc.Case("big18", "mimc-two-ctx", wc.MIMC_2, 5000, [[42, 3 + u] for u in range(40)])
    jobs = [(_lib.ctx(), a), (_lib.second_ctx(), b)]
    alone = [host_form(L, c, ctx) for ctx, c in jobs]
    together = [None, None]

    def run(i):
        ctx, c = jobs[i]
        for _ in range(3):
            out = host_form(L, c, ctx)
            together[i] = out if together[i] is None or together[i] == out else b""
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert together == alone
    assert alone[1][:16 * 5000] == wc.trace_words(big, [42, 3], 5000, wc.MIMC_2)
    assert alone[0][:8 * 9 * 300] == wc.trace_words(gl, a.inputs[0], 300, wc.W9_256)


# ---- 8. interleaved with the other two generators ------------------------------------------------------------------------------------------------
def test_interleaved_with_the_other_generators(L):
    """sh_stark_witness, sh_mod_stark_witness and sh_mod64_stark_witness take turns on one context with the same step polynomials:
    three separate term images"""
    from starks_amd import stark
    gl = wc.GOLDILOCKS
    raw = wire([42, 3])
    want_m = b"".join(wire(col) for col in sv.trace([42, 3], 200, wc.MIMC_2))
    want_g = wire(wc.ints(wc.trace_words(gl, [42, 3], 200, wc.MIMC_2)))
    want_w = wc.trace_words(gl, [42, 3], 200, wc.MIMC_2)
    want_b = wc.trace_words(wc.BIG18, [42, 3], 200, wc.MIMC_2)
    assert want_m != want_g and want_w != want_b
    for _ in range(3):
        assert stark.witness_flat(raw, 200, 2, _polys(wc.MIMC_2)) == want_m
        assert stark.mod64_witness_flat(gl, [42, 3], 200, 2, _polys(wc.MIMC_2)) == want_w
        assert stark.mod_witness_flat(gl, raw, 200, 2, _polys(wc.MIMC_2)) == want_g
        assert stark.mod64_witness_flat(wc.BIG18, [42, 3], 200, 2, _polys(wc.MIMC_2)) == want_b
    assert stark.mod64_witness_flat(gl, [42, 3], 200, 2, _polys(wc.MIMC_2)) == want_w


# ---- 9. the errors --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(L):
    """every refusal is made on the host, returns its status and names the entry in sh_last_error; the buffers are far too small for the
    refused shapes, so a call that got as far as using them would be seen"""
    ctx, gl = _ctx(), wc.GOLDILOCKS
    c = wc.Case("goldilocks", "mimc2-errors", wc.MIMC_2, 10, [[42, 3]])
    trace = wc.trace_words(gl, [42, 3], 10, wc.MIMC_2)
    coefs, exps, counts = _args(c)
    inp = c.input_words()
    out = ctypes.create_string_buffer(16 * 10)
    zero = (ctypes.c_uint32 * 2)(0, 0)
    ten = (ctypes.c_uint32 * 10)(*([1] * 10))
    many = (ctypes.c_uint32 * 2)(200, 57)
    table = [
        (dict(inp=None), INVALID), (dict(coefs=None), INVALID), (dict(exps=None), INVALID), (dict(counts=None), INVALID),
        (dict(out=None), INVALID),
        (dict(p=gl + 1), INVALID), (dict(p=2), INVALID), (dict(p=1), INVALID), (dict(p=0), INVALID),
        (dict(steps=0), INVALID), (dict(width=0), INVALID), (dict(batch=0), INVALID), (dict(counts=zero), INVALID),
        (dict(width=10, counts=ten, coefs=coefs * 5, exps=bytes(100), inp=inp * 5), UNSUPPORTED),
        (dict(counts=many, coefs=bytes(32 * 257), exps=bytes(2 * 257)), UNSUPPORTED),
        (dict(batch=1 << 31), UNSUPPORTED), (dict(steps=1 << 62), UNSUPPORTED),
    ]

    def host(p=gl, inp=inp, steps=10, width=2, coefs=coefs, exps=exps, counts=counts, batch=1, out=out, cap=20):
        rc = L.sh_mod64_stark_witness(ctx, p, inp, steps, width, coefs, exps, counts, batch, out, cap)
        return rc, L.sh_last_error(ctx).decode()

    assert L.sh_mod64_stark_witness(None, gl, inp, 10, 2, coefs, exps, counts, 1, out, 20) == INVALID
    for kw, want in table + [(dict(cap=19), TOO_SMALL), (dict(batch=2), TOO_SMALL)]:
        rc, text = host(**kw)
        assert rc == want and text.startswith("sh_mod64_stark_witness: "), (kw, rc, text)
    d = ctypes.c_void_p()
    assert L.sh_dev_alloc(ctx, 16 * 11, ctypes.byref(d)) == OK
    try:
        w = ctypes.c_void_p(d.value + 16)

        def dev(p=gl, inp=d, steps=10, width=2, coefs=coefs, exps=exps, counts=counts, batch=1, out=w):
            rc = L.sh_dev_mod64_stark_witness(ctx, p, inp, steps, width, coefs, exps, counts, batch, out)
            return rc, L.sh_last_error(ctx).decode()

        assert L.sh_dev_mod64_stark_witness(None, gl, d, 10, 2, coefs, exps, counts, 1, w) == INVALID
        overlap = [(dict(out=ctypes.c_void_p(d.value + 8)), INVALID), (dict(out=d), INVALID),
                   (dict(inp=ctypes.c_void_p(d.value + 16 * 10)), INVALID)]
        for kw, want in table + overlap:
            kw = {k: v for k, v in kw.items() if not (k == "inp" and v is not None and not isinstance(v, ctypes.c_void_p))}
            rc, text = dev(**kw)
            assert rc == want and text.startswith("sh_dev_mod64_stark_witness: "), (kw, rc, text)
        assert L.sh_dev_upload(ctx, inp, d, len(inp)) == OK
        rc, text = dev()
        assert rc == OK, text
        got = ctypes.create_string_buffer(16 * 10)
        assert L.sh_dev_download(ctx, w, got, len(got)) == OK
        assert got.raw == trace
    finally:
        assert L.sh_sync(ctx) == OK
        L.sh_dev_free(ctx, d)
    assert host()[0] == OK and out.raw == trace
