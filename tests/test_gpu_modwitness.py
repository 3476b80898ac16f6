"""STARK witnesses generated on the MI355X over any odd modulus below 2^256 (sh_mod_stark_witness, sh_dev_mod_stark_witness:
starks_amd/csrc/modwitness_items.cuh, modwitness.hip, api_modstark.hip): the whole grid of tests/modwitness_cases.py against the exact
oracle (oracle/pyoracle.py with p = the modulus, pinned to the reference by tests/golden/mod_witness.json), byte for byte, in the host
and the device form; the tuned MiMC generator as yardstick through the generic entry; partial waves, slice boundaries and a trace that
crosses default slices; every group x slice decomposition in child processes; the device-resident chain generate -> prove -> verify;
two contexts with different moduli at once; interleaving with the MiMC generator; the errors; the Python call sites."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading

import pytest

import modstark_cases as sc
import modwitness_cases as wc
import stark_variants as sv
from conftest import ROOT, load_golden
from modntt_cases import wire

pytestmark = pytest.mark.gpu

OK, INVALID, TOO_SMALL, UNSUPPORTED = 0, -1, -5, -6


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


def host_form(L, c, ctx=None):
    """sh_mod_stark_witness on a Case, values and coefficients as the case stores them -> wire bytes"""
    ctx = ctx or _ctx()
    coefs, exps, counts = _args(c)
    out = ctypes.create_string_buffer(32 * c.batch * c.width * c.steps)
    rc = L.sh_mod_stark_witness(ctx, b32(c.p), c.input_wire(), c.steps, c.width, coefs, exps, counts, c.batch, out, len(out))
    assert rc == OK, (c.id, rc, L.sh_last_error(ctx))
    return out.raw


def device_form(L, c):
    """sh_dev_mod_stark_witness from uploaded limbs -> the downloaded limb bytes"""
    ctx = _ctx()
    coefs, exps, counts = _args(c)
    limbs = c.input_limbs()
    nbytes = 32 * c.batch * c.width * c.steps
    di, dw = ctypes.c_void_p(), ctypes.c_void_p()
    try:
        assert L.sh_dev_alloc(ctx, len(limbs), ctypes.byref(di)) == OK and L.sh_dev_alloc(ctx, nbytes, ctypes.byref(dw)) == OK
        assert L.sh_dev_upload(ctx, limbs, di, len(limbs)) == OK
        rc = L.sh_dev_mod_stark_witness(ctx, b32(c.p), di, c.steps, c.width, coefs, exps, counts, c.batch, dw)
        assert rc == OK, (c.id, rc, L.sh_last_error(ctx))
        out = ctypes.create_string_buffer(nbytes)
        assert L.sh_dev_download(ctx, dw, out, nbytes) == OK
    finally:
        for ptr in (di, dw):
            if ptr.value:
                L.sh_dev_free(ctx, ptr)
    return out.raw


# ---- 1, 2. the grid, both forms ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(wc.MODULI))
def test_grid_host_form(L, name):
    cases = [c for c in wc.GRID if c.name == name]
    assert cases
    for c in cases:
        assert host_form(L, c) == wc.want_wire(c), c.id


@pytest.mark.parametrize("name", sorted(wc.MODULI))
def test_grid_device_form(L, name):
    for c in [c for c in wc.GRID if c.name == name]:
        assert device_form(L, c) == wc.want_limbs(c), c.id


# ---- 3. the tuned generator as yardstick ---------------------------------------------------------------------------------------------------
def test_mimc_prime_equals_the_tuned_generator(L):
    from starks_amd import stark
    p = wc.MIMC_P
    jobs = [(wc.MIMC_2, [[42, 3], [p - 1, p - 2]], 1000), (wc.W9_256, wc.W9_INPUTS, 70), (wc.MIXED_3, [[1, 2, 3]], 65)]
    jobs += [(sp, ins, 100) for _, sp, ins in wc.edge_systems(p)]
    for sp, ins, steps in jobs:
        raw = wire([v for u in ins for v in u])
        assert (stark.mod_witness_flat(p, raw, steps, len(sp), _polys(sp), batch=len(ins))
                == stark.witness_flat(raw, steps, len(sp), _polys(sp), batch=len(ins)))


# ---- 4. partial waves, G > 1, groups that exit whole ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 65, 130])
def test_batches(L, nb):
    v = [x for x in load_golden("stark_variants.json")["cases"] if x["name"] == "w5_middle"][0]
    p = wc.MODULI["bn254"]
    c = wc.Case("bn254", "w5_middle-b%d" % nb, sv.step_polys(v), 40, [[x % p for x in sv.unit_inputs(v, u)] for u in range(nb)])
    want = b"".join(wc.trace_wire(p, u, 40, c.sp) for u in c.inputs)
    assert host_form(L, c) == want


# ---- 5, 7. decompositions and slice boundaries in child processes --------------------------------------------------------------------------
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
    raw = bytes.fromhex(inputs)
    out.append(hashlib.sha256(stark.mod_witness_flat(p, raw, steps, width, polys, batch=len(raw) // (32 * width))).hexdigest())
print(json.dumps(out))
"""


def _job(p, ins, steps, sp):
    return (p, wire([v % p for u in ins for v in u]).hex(), steps, len(sp), [[[list(k), v % p] for k, v in sorted(d.items())] for d in sp])


def _decomposition_jobs():
    """two fixture systems, the width-3 system one step shorter than, as long as and one step longer than the slices 3 and 64, and three
    units of the 256-term system at 70 steps; over bn254, goldilocks and 2^256 - 1"""
    bn, gl, ones = wc.MODULI["bn254"], wc.MODULI["goldilocks"], wc.ALL_ONES
    jobs = [_job(bn, [[2, 5]], 64, wc.MIMC_2), _job(gl, [[3, 4, 5]], 64, wc.MIXED_3)]
    for i, steps in enumerate((2, 3, 4, 63, 64, 65)):
        jobs.append(_job((bn, gl, ones)[i % 3], [[5, 6, 7], [ones - 1, 0, 3]], steps, wc.MIXED_3))
    jobs.append(_job(bn, wc.W9_INPUTS, 70, wc.W9_256))
    jobs.append(_job(ones, wc.W9_INPUTS, 70, wc.W9_256))
    return jobs


def _want_sha(jobs):
    return [wc.sha(b"".join(wc.trace_wire(p, [int.from_bytes(bytes.fromhex(ins)[32 * (u * w + j):32 * (u * w + j + 1)], "big") for j in range(w)],
                                          steps, [{tuple(k): v for k, v in d} for d in sp])
                            for u in range(len(ins) // (64 * w)))) for p, ins, steps, w, sp in jobs]


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
    got = []
    for p, ins, steps, w, sp in jobs:
        raw = bytes.fromhex(ins)
        got.append(wc.sha(stark.mod_witness_flat(p, raw, steps, w, _polys([{tuple(k): v for k, v in d} for d in sp]), batch=len(raw) // (32 * w))))
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


def test_store_on_the_kernels_store_path(default_run):
    """STARKHIP_WITNESS_STORE=inline (conversion in the kernel, none in a closing pass) gives the same bytes, also with a dispatch per step"""
    jobs, want = default_run
    assert _child({"STARKHIP_WITNESS_STORE": "inline"}, jobs) == want
    assert _child({"STARKHIP_WITNESS_STORE": "inline", "STARKHIP_WITNESS_SLICE": "1", "STARKHIP_WITNESS_GROUP": "4"}, jobs) == want


@pytest.mark.parametrize("group", ["1", "2"])
def test_steps_longer_than_a_dispatch_budget(L, group):
    """HEAVY (256 terms, exponents 255) under groups 1 and 2: a step exceeds a dispatch's budget, the trace is launched one step per
    dispatch, ends, and equals the oracle"""
    c = wc.HEAVY_CASE
    job = [_job(c.p, c.inputs, c.steps, c.sp)]
    assert _child({"STARKHIP_WITNESS_GROUP": group}, job) == [wc.sha(wc.want_wire(c))]


# ---- 6. one long trace ----------------------------------------------------------------------------------------------------------------------
def test_long_mimc_trace_crosses_default_slices(L):
    p = wc.MODULI["bn254"]
    c = wc.Case("bn254", "mimc2-long", wc.MIMC_2, 5000, [[42 + u, 3 + u] for u in range(40)])
    assert host_form(L, c) == b"".join(wc.trace_wire(p, u, 5000, wc.MIMC_2) for u in c.inputs)


# ---- 8. generate -> prove -> verify without leaving the device -------------------------------------------------------------------------------
def _chain(L, c):
    """sh_dev_mod_stark_witness -> sh_dev_mod_stark_prove -> sh_dev_mod_stark_verify reading inputs and outputs from the generated witness
    -> (flat proofs, per-proof status, sh_stark_status)"""
    ctx = _ctx()
    counts, coefs, exps = c.terms()
    coefs, counts = wire(coefs), (ctypes.c_uint32 * c.width)(*counts)
    plen = L.sh_stark_proof_len(c.steps, c.ext, c.width, c.degree, c.samples)
    limbs = b"".join(int(v).to_bytes(32, "little") for inp in c.inputs for v in inp)
    di, dw, dp, ds = (ctypes.c_void_p() for _ in range(4))
    try:
        for ptr, nbytes in ((di, len(limbs)), (dw, 32 * c.batch * c.width * c.steps), (dp, plen * c.batch), (ds, 4 * c.batch)):
            assert L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)) == OK
        assert L.sh_dev_upload(ctx, limbs, di, len(limbs)) == OK
        pb = b32(c.p)
        assert L.sh_dev_mod_stark_witness(ctx, pb, di, c.steps, c.width, coefs, exps, counts, c.batch, dw) == OK, L.sh_last_error(ctx)
        assert L.sh_dev_mod_stark_prove(ctx, pb, dw, di, c.steps, c.ext, c.width, coefs, exps, counts, c.samples, c.batch, dp) == OK, L.sh_last_error(ctx)
        last = ctypes.c_void_p(dw.value + 32 * (c.steps - 1))
        assert L.sh_dev_mod_stark_verify(ctx, pb, dp, dw, last, c.steps, c.steps, c.ext, c.width, coefs, exps, counts, c.samples, c.batch,
                                         ds) == OK, L.sh_last_error(ctx)
        flat = ctypes.create_string_buffer(plen * c.batch)
        st = (ctypes.c_int32 * c.batch)()
        assert L.sh_dev_download(ctx, dp, flat, len(flat)) == OK and L.sh_dev_download(ctx, ds, st, 4 * c.batch) == OK
        status = L.sh_stark_status(ctx)
    finally:
        assert L.sh_sync(ctx) == OK
        for ptr in (di, dw, dp, ds):
            if ptr.value:
                L.sh_dev_free(ctx, ptr)
    return flat.raw, list(st), status


def test_prove_inputs_fixture(L):
    """mod_prove_inputs_flat on the three cases of tests/golden/mod_stark.json (the live reference's proofs)"""
    from starks_amd import stark
    G = load_golden("mod_stark.json")["cases"]
    for key, c in sc.FIXTURE.items():
        flat, outs = stark.mod_prove_inputs_flat(c.p, c.input_wire(), c.steps, c.ext, c.width, _polys(c.sp), samples=c.samples)
        g = G[key]
        assert len(flat) == g["len"] and hashlib.sha256(flat).hexdigest() == g["sha256"], key
        assert flat[:32].hex() == g["m_root"] and flat[32:64].hex() == g["l_root"], key
        assert outs == wire([col[-1] for col in c.witnesses()[0]]), key
        got, st, status = _chain(L, c)
        assert got == flat and st == [0] and status == OK, key


@pytest.mark.parametrize("name", sorted(sc.MODULI))
def test_prove_inputs_grid(L, name):
    """every small grid case of the generic prover from its inputs alone equals the oracle's flat proofs; the device verifier, reading
    the boundary values straight from the generated witness (io_stride = steps), accepts each; sh_stark_status is SH_OK"""
    from starks_amd import stark
    assert L.sh_stark_status(_ctx()) in (OK, -8)  # drop what earlier tests may have left
    cases = [c for c in sc.GRID if c.name == name and c.n <= 256 and c.batch <= 3]
    assert cases
    for c in cases:
        want = sc.oracle_flat(c)
        flat, outs = stark.mod_prove_inputs_flat(c.p, c.input_wire(), c.steps, c.ext, c.width, _polys(c.sp), batch=c.batch, samples=c.samples)
        assert flat == want, c.id
        assert outs == wire([col[-1] for w in c.witnesses() for col in w]), c.id
        got, st, status = _chain(L, c)
        assert got == want and st == [0] * c.batch and status == OK, c.id


# ---- 9. two contexts, two moduli, two host threads --------------------------------------------------------------------------------------------
def test_two_contexts_at_once(L):
    from starks_amd import _lib
    bn, gl = wc.MODULI["bn254"], wc.MODULI["goldilocks"]
    five = [sv.unit_inputs([x for x in load_golden("stark_variants.json")["cases"] if x["name"] == "w9_256_terms"][0], u) for u in range(5)]
    a = wc.Case("bn254", "w9-two-ctx", wc.W9_256, 300, [[v % bn for v in u] for u in five])
    b = wc.Case("goldilocks", "mimc-two-ctx", wc.MIMC_2, 5000, [[42, 3 + u] for u in range(40)])
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
    assert alone[1][:64 * 5000] == wc.trace_wire(gl, [42, 3], 5000, wc.MIMC_2)
    assert alone[0][:32 * 9 * 300] == wc.trace_wire(bn, a.inputs[0], 300, wc.W9_256)


# ---- 10. interleaved with the MiMC generator ----------------------------------------------------------------------------------------------------
def test_interleaved_with_the_mimc_generator(L):
    """sh_stark_witness and sh_mod_stark_witness take turns on one context with the same step polynomials: two separate term images"""
    from starks_amd import stark
    bn = wc.MODULI["bn254"]
    raw = wire([42, 3])
    want_m = b"".join(wire(col) for col in sv.trace([42, 3], 200, wc.MIMC_2))
    want_g = wc.trace_wire(bn, [42, 3], 200, wc.MIMC_2)
    assert want_m != want_g
    for _ in range(3):
        assert stark.witness_flat(raw, 200, 2, _polys(wc.MIMC_2)) == want_m
        assert stark.mod_witness_flat(bn, raw, 200, 2, _polys(wc.MIMC_2)) == want_g
    assert stark.mod_witness_flat(wc.MODULI["goldilocks"], raw, 200, 2, _polys(wc.MIMC_2)) == wc.trace_wire(wc.MODULI["goldilocks"], [42, 3], 200, wc.MIMC_2)
    assert stark.witness_flat(raw, 200, 2, _polys(wc.MIMC_2)) == want_m


# ---- 11. the errors ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(L):
    """every refusal is made on the host, returns its status and names the entry in sh_last_error; the buffers are far too small for the
    refused shapes, so a call that got as far as using them would be seen"""
    ctx, bn = _ctx(), wc.MODULI["bn254"]
    c = wc.Case("bn254", "mimc2-errors", wc.MIMC_2, 10, [[42, 3]])
    trace = wc.trace_wire(bn, [42, 3], 10, wc.MIMC_2)
    coefs, exps, counts = _args(c)
    inp = c.input_wire()
    out = ctypes.create_string_buffer(64 * 10)
    zero = (ctypes.c_uint32 * 2)(0, 0)
    ten = (ctypes.c_uint32 * 10)(*([1] * 10))
    many = (ctypes.c_uint32 * 2)(200, 57)
    table = [
        (dict(p=None), INVALID), (dict(inp=None), INVALID), (dict(coefs=None), INVALID), (dict(exps=None), INVALID),
        (dict(counts=None), INVALID), (dict(out=None), INVALID),
        (dict(p=bn + 1), INVALID), (dict(p=1 << 64), INVALID), (dict(p=1), INVALID), (dict(p=0), INVALID),
        (dict(steps=0), INVALID), (dict(width=0), INVALID), (dict(batch=0), INVALID), (dict(counts=zero), INVALID),
        (dict(width=10, counts=ten, coefs=coefs * 5, exps=bytes(100), inp=inp * 5), UNSUPPORTED),
        (dict(counts=many, coefs=bytes(32 * 257), exps=bytes(2 * 257)), UNSUPPORTED),
        (dict(batch=1 << 31), UNSUPPORTED), (dict(steps=1 << 60), UNSUPPORTED),
    ]

    def host(p=bn, inp=inp, steps=10, width=2, coefs=coefs, exps=exps, counts=counts, batch=1, out=out, cap=len(out)):
        rc = L.sh_mod_stark_witness(ctx, b32(p) if p is not None else None, inp, steps, width, coefs, exps, counts, batch, out, cap)
        return rc, L.sh_last_error(ctx).decode()

    assert L.sh_mod_stark_witness(None, b32(bn), inp, 10, 2, coefs, exps, counts, 1, out, len(out)) == INVALID
    for kw, want in table + [(dict(cap=len(out) - 1), TOO_SMALL), (dict(batch=2), TOO_SMALL)]:
        rc, text = host(**kw)
        assert rc == want and text.startswith("sh_mod_stark_witness: "), (kw, rc, text)
    d = ctypes.c_void_p()
    assert L.sh_dev_alloc(ctx, 64 * 11, ctypes.byref(d)) == OK
    try:
        w = ctypes.c_void_p(d.value + 64)

        def dev(p=bn, inp=d, steps=10, width=2, coefs=coefs, exps=exps, counts=counts, batch=1, out=w):
            rc = L.sh_dev_mod_stark_witness(ctx, b32(p) if p is not None else None, inp, steps, width, coefs, exps, counts, batch, out)
            return rc, L.sh_last_error(ctx).decode()

        assert L.sh_dev_mod_stark_witness(None, b32(bn), d, 10, 2, coefs, exps, counts, 1, w) == INVALID
        overlap = [(dict(out=ctypes.c_void_p(d.value + 32)), INVALID), (dict(out=d), INVALID),
                   (dict(inp=ctypes.c_void_p(d.value + 64 * 10)), INVALID)]
        for kw, want in table + overlap:
            kw = {k: v for k, v in kw.items() if not (k == "inp" and v is not None and not isinstance(v, ctypes.c_void_p))}
            rc, text = dev(**kw)
            assert rc == want and text.startswith("sh_dev_mod_stark_witness: "), (kw, rc, text)
        limbs = c.input_limbs()
        assert L.sh_dev_upload(ctx, limbs, d, len(limbs)) == OK
        rc, text = dev()
        assert rc == OK, text
        got = ctypes.create_string_buffer(64 * 10)
        assert L.sh_dev_download(ctx, w, got, len(got)) == OK
        assert got.raw == b"".join(trace[i:i + 32][::-1] for i in range(0, len(trace), 32))
    finally:
        assert L.sh_sync(ctx) == OK
        L.sh_dev_free(ctx, d)
    assert host()[0] == OK and out.raw == trace


# ---- 12. the Python call site -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bn254", "mimc"])
def test_air_device_witness(L, name):
    from starks_amd import IntegersModP, air
    from starks_amd.multivariate_polynomial import multivariates_over
    F = IntegersModP(wc.MODULI[name])
    mv = multivariates_over(F, 2).factory
    polys = [mv({k: F(v) for k, v in d.items()}) for d in wc.MIMC_2]
    want = air.AIR(F, 2, [2, 5], 64, polys, 8).generate_witness()
    got = air.device_witness(F, [2, 5], 64, polys)
    assert len(got) == 2 and [[int(x) for x in col] for col in got] == [[int(x) for x in col] for col in want]
    if name == "bn254":
        g = load_golden("mod_witness.json")["cases"]["bn254-mimc2"]
        assert hashlib.sha256(b"".join(bytes(col.wire()) for col in got)).hexdigest() == g["sha256"]
