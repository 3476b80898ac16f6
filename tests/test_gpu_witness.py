"""Witnesses generated on the GPU from any AIR's step polynomials (sh_dev_stark_witness / sh_stark_witness, csrc/witness.hip): equal to the
reference's traces, and proved from the device without leaving it (stark.prove_inputs_flat) to the fixture proofs' bytes."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import threading

import pytest

import stark_variants as sv
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

P = sv.P
MIMC = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


def _polys(sp):
    return [_Poly(d) for d in sp]


def _wire(vals):
    return b"".join((int(v) % P).to_bytes(32, "big") for v in vals)


def _trace_bytes(inputs, steps, sp):
    return b"".join(_wire(col) for col in sv.trace(inputs, steps, sp))


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def _case_polys(c):
    return [{tuple(k): v for k, v in d} for d in c["step_polys"]]


@pytest.mark.parametrize("c", load_golden("stark.json"), ids=lambda c: c["name"])
def test_reference_cases(L, c):
    from starks_amd import stark
    sp, steps, width = _case_polys(c), c["steps"], c["width"]
    want = b"".join(bytes.fromhex(v) for col in c["witness"] for v in col)
    assert stark.witness_flat(_wire(c["inputs"]), steps, width, _polys(sp)) == want
    flat, outs = stark.prove_inputs_flat(_wire(c["inputs"]), steps, c["ext"], width, _polys(sp))
    assert len(flat) == c["flat_len"] and hashlib.sha256(flat).hexdigest() == c["flat_sha"]
    assert outs == b"".join(bytes.fromhex(col[-1]) for col in c["witness"])
    assert stark.verify_flat(flat, _wire(c["inputs"]), outs, steps, c["ext"], width, _polys(sp))


@pytest.mark.parametrize("c", load_golden("stark_variants.json")["cases"], ids=lambda c: c["name"])
def test_variant_matrix(L, c):
    """Every unit of every batch generated on the device and proved there (sh_dev_stark_witness -> sh_dev_stark_prove) equals its fixture
    hash; the first and last unit's witness equals the Python trace."""
    from starks_amd import stark
    steps, ext, width, nb = c["steps"], c["ext"], c["width"], c["batch"]
    sp = sv.step_polys(c)
    ins = [sv.unit_inputs(c, u) for u in range(nb)]
    flat, outs = stark.prove_inputs_flat(b"".join(_wire(i) for i in ins), steps, ext, width, _polys(sp), batch=nb)
    plen = c["proof_bytes"]
    bad = [u for u in range(nb) if hashlib.sha256(flat[u * plen:(u + 1) * plen]).hexdigest() != c["unit_sha256"][u]]
    assert not bad, (c["name"], bad[:16])
    ends = [ins[0], ins[-1]]
    got = stark.witness_flat(b"".join(_wire(i) for i in ends), steps, width, _polys(sp), batch=2)
    want = b"".join(_trace_bytes(i, steps, sp) for i in ends)
    assert got == want
    last = 32 * width * steps
    assert outs[:32 * width] == b"".join(got[(d + 1) * 32 * steps - 32:(d + 1) * 32 * steps] for d in range(width))
    assert outs[-32 * width:] == b"".join(got[last + (d + 1) * 32 * steps - 32:last + (d + 1) * 32 * steps] for d in range(width))


def test_config5_units_at_size(L):
    """The eight config-5 fixture units at 2^16 steps, proved from their inputs in one batch."""
    from starks_amd import stark
    cases = load_golden("stark_units.json")["cases"]
    steps, ext = cases[0]["steps"], cases[0]["ext"]
    flat, outs = stark.prove_inputs_flat(b"".join(_wire(c["inputs"]) for c in cases), steps, ext, 2, _polys(MIMC), batch=len(cases))
    plen = cases[0]["proof_bytes"]
    for i, c in enumerate(cases):
        proof = flat[i * plen:(i + 1) * plen]
        assert outs[64 * i:64 * i + 64] == b"".join(bytes.fromhex(v) for v in c["outputs"]), c["unit"]
        assert proof[:32].hex() == c["m_root"] and hashlib.sha256(proof).hexdigest() == c["proof_sha256"], c["unit"]


@pytest.mark.parametrize("c", load_golden("stark_large.json")["cases"], ids=lambda c: "steps_2^%d" % c["logsteps"])
def test_large_traces(L, c):
    from starks_amd import stark
    flat, outs = stark.prove_inputs_flat(_wire(c["inputs"]), c["steps"], c["ext"], 2, _polys(_case_polys(c)))
    assert outs == b"".join(bytes.fromhex(v) for v in c["outputs"])
    assert flat[:32].hex() == c["m_root"] and flat[32:64].hex() == c["l_root"]
    assert hashlib.sha256(flat).hexdigest() == c["proof_sha256"]


def test_mimc_512_units_equal_the_dedicated_generator_and_verify(L):
    """512 units at 2^16 steps through the generic entry equal sh_dev_fill_mimc_units byte for byte (compared in chunks), and the batch
    verifier accepts all 512 proofs of them, reading the boundary values from the witness (io_stride = steps)."""
    from starks_amd import _lib, stark
    ctx = _lib.ctx()
    steps, ext, units, chunk = 1 << 16, 8, 512, 64
    coefs, exps, counts, degree = stark.pack_step_polys(_polys(MIMC), 2)
    plen = stark.proof_len(steps, ext, 2, degree)
    wb = 64 * steps * units
    bufs = [ctypes.c_void_p() for _ in range(5)]
    try:
        for ptr, nb in zip(bufs, (wb, wb, 64 * units, plen * chunk, 4 * chunk)):
            _lib.check(L.sh_dev_alloc(ctx, nb, ctypes.byref(ptr)), "alloc")
        dref, dgen, di, dp, ds = bufs
        _lib.check(L.sh_dev_fill_mimc_units(ctx, dref, di, steps, 0, units, 42), "fill")
        _lib.check(L.sh_dev_stark_witness(ctx, di, steps, 2, coefs, exps, counts, units, dgen), "witness")
        a = ctypes.create_string_buffer(64 * steps * chunk)
        b = ctypes.create_string_buffer(64 * steps * chunk)
        for u in range(0, units, chunk):
            off = 64 * steps * u
            _lib.check(L.sh_dev_download(ctx, ctypes.c_void_p(dref.value + off), a, len(a)), "dl")
            _lib.check(L.sh_dev_download(ctx, ctypes.c_void_p(dgen.value + off), b, len(b)), "dl")
            assert a.raw == b.raw, "units %d .. %d differ" % (u, u + chunk - 1)
        for u in range(0, units, chunk):
            w = ctypes.c_void_p(dgen.value + 64 * steps * u)
            inp = ctypes.c_void_p(di.value + 64 * u)
            _lib.check(L.sh_dev_stark_prove(ctx, w, inp, steps, ext, 2, coefs, exps, counts, 80, chunk, dp), "prove")
            last = ctypes.c_void_p(w.value + 32 * (steps - 1))
            _lib.check(L.sh_dev_stark_verify(ctx, dp, w, last, steps, steps, ext, 2, coefs, exps, counts, 80, chunk, ds), "verify")
            st = (ctypes.c_int32 * chunk)()
            _lib.check(L.sh_dev_download(ctx, ds, st, 4 * chunk), "dl")
            assert list(st) == [0] * chunk, u
        assert L.sh_stark_status(ctx) == 0
    finally:
        for ptr in bufs:
            if ptr.value:
                L.sh_dev_free(ctx, ptr)


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
from starks_amd import stark, _lib
out = []
for inputs, steps, width, sp in json.loads(sys.stdin.read()):
    class Q(object):
        pass
    polys = []
    for d in sp:
        q = Q()
        q.coefficients = {tuple(k): v for k, v in d}
        polys.append(q)
    out.append(hashlib.sha256(stark.witness_flat(bytes.fromhex(inputs), steps, width, polys, batch=len(inputs) // (64 * width))).hexdigest())
print(json.dumps(out))
"""


def _alternate_jobs():
    cases = load_golden("stark.json")[:2]
    mixed = [c for c in load_golden("stark.json") if c["name"] == "mixed_w3_s16"][0]
    w9 = [c for c in load_golden("stark_variants.json")["cases"] if c["name"] == "w9_256_terms"][0]
    jobs = [(_wire(c["inputs"]).hex(), c["steps"], c["width"], c["step_polys"]) for c in cases]
    for s in (3, 64):
        for steps in (s - 1, s, s + 1):
            jobs.append((_wire(mixed["inputs"] + [5, 6, 7]).hex(), steps, 3, mixed["step_polys"]))
    jobs.append((b"".join(_wire(sv.unit_inputs(w9, u)) for u in range(3)).hex(), 70, 9, w9["step_polys"]))
    return jobs


def _child(env_extra, jobs):
    env = dict(os.environ)
    env.pop("STARKHIP_WITNESS_GROUP", None)
    env.pop("STARKHIP_WITNESS_SLICE", None)
    env.update(env_extra)
    code = _CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    out = subprocess.run([sys.executable, "-c", code], input=json.dumps(jobs), capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_alternate_decompositions(L):
    """STARKHIP_WITNESS_GROUP x STARKHIP_WITNESS_SLICE in child processes give the default run's bytes, including traces one step
    shorter than, as long as, and one step longer than a slice."""
    from starks_amd import stark
    jobs = _alternate_jobs()
    want = []
    for inputs, steps, width, sp in jobs:
        raw = bytes.fromhex(inputs)
        want.append(hashlib.sha256(stark.witness_flat(raw, steps, width, _polys([{tuple(k): v for k, v in d} for d in sp]),
                                                      batch=len(raw) // (32 * width))).hexdigest())
    for g in (1, 2, 4, 8, 16):
        for s in (1, 3, 64):
            assert _child({"STARKHIP_WITNESS_GROUP": str(g), "STARKHIP_WITNESS_SLICE": str(s)}, jobs) == want, (g, s)


# 256 terms, every exponent 255, coefficient 2: one step is about 34600 products on one lane, more than a dispatch's budget
HEAVY = [{tuple((t * 7 + v) % 256 if v == t % 9 else 255 for v in range(9)): 2 for t in range(c, 256, 9)} for c in range(9)]


def test_steps_longer_than_a_dispatch_budget(L):
    """Under STARKHIP_WITNESS_GROUP = 1 and 2 a step of this system exceeds a dispatch's budget: the trace is still launched one step per
    dispatch, ends, and equals the Python trace."""
    ins = list(range(2, 11))
    want = hashlib.sha256(_trace_bytes(ins, 3, HEAVY)).hexdigest()
    job = [(_wire(ins).hex(), 3, 9, [[[list(k), v] for k, v in d.items()] for d in HEAVY])]
    for g in ("1", "2"):
        assert _child({"STARKHIP_WITNESS_GROUP": g}, job) == [want], g


EDGES = [
    ("zero_polynomial", 2, [{}, {(1, 1): 1}], [[5, 7], [0, 1]]),
    ("coefficients_0_and_p_minus_1", 2, [{(1, 0): P - 1, (0, 1): 0}, {(1, 1): P - 1, (0, 0): 3}], [[5, 7], [P - 1, 2]]),
    ("exponent_255", 2, [{(255, 0): 1}, {(3, 255): 2, (0, 0): 1}], [[3, 5], [P - 2, 1]]),
    ("fib_from_zero", 2, [{(0, 1): 1}, {(0, 1): 1, (1, 0): 1}], [[0, 1], [0, 0]]),
]


@pytest.mark.parametrize("name,width,sp,ins", EDGES, ids=[e[0] for e in EDGES])
def test_edge_systems(L, name, width, sp, ins):
    from starks_amd import stark
    for steps in (1, 3, 1000):
        got = stark.witness_flat(b"".join(_wire(i) for i in ins), steps, width, _polys(sp), batch=len(ins))
        assert got == b"".join(_trace_bytes(i, steps, sp) for i in ins), (name, steps)
    raw = (42 + P).to_bytes(32, "big") + (P + 3).to_bytes(32, "big")  # unreduced inputs
    assert stark.witness_flat(raw, 100, 2, _polys(MIMC)) == _trace_bytes([42, 3], 100, MIMC)


@pytest.mark.parametrize("nb", [1, 65, 130])
def test_batches(L, nb):
    from starks_amd import stark
    c = [x for x in load_golden("stark_variants.json")["cases"] if x["name"] == "w5_middle"][0]
    sp = sv.step_polys(c)
    ins = [sv.unit_inputs(c, u) for u in range(nb)]
    got = stark.witness_flat(b"".join(_wire(i) for i in ins), 40, 5, _polys(sp), batch=nb)
    assert got == b"".join(_trace_bytes(i, 40, sp) for i in ins)


def test_two_contexts_at_once(L):
    from starks_amd import _lib, stark
    c = [x for x in load_golden("stark_variants.json")["cases"] if x["name"] == "w9_256_terms"][0]
    coefs, exps, counts, _ = stark.pack_step_polys(_polys(sv.step_polys(c)), 9)
    mcoefs, mexps, mcounts, _ = stark.pack_step_polys(_polys(MIMC), 2)
    jobs = [(_lib.ctx(), b"".join(_wire(sv.unit_inputs(c, u)) for u in range(5)), 300, 9, coefs, exps, counts, 5),
            (_lib.second_ctx(), b"".join(_wire([42, 3 + u]) for u in range(40)), 5000, 2, mcoefs, mexps, mcounts, 40)]
    alone = []
    for ctx, inp, steps, width, cf, ex, cn, nb in jobs:
        out = ctypes.create_string_buffer(32 * nb * width * steps)
        _lib.check(L.sh_stark_witness(ctx, inp, steps, width, cf, ex, cn, nb, out, len(out)), "witness")
        alone.append(out.raw)
    together = [None, None]

    def run(i):
        ctx, inp, steps, width, cf, ex, cn, nb = jobs[i]
        out = ctypes.create_string_buffer(32 * nb * width * steps)
        for _ in range(3):
            assert L.sh_stark_witness(ctx, inp, steps, width, cf, ex, cn, nb, out, len(out)) == 0
            together[i] = out.raw if together[i] is None or together[i] == out.raw else b""
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert together == alone
    assert alone[1][:64 * 5000] == _trace_bytes([42, 3], 5000, MIMC)


def test_errors_leave_the_context_usable(L):
    from starks_amd import _lib, stark
    ctx = _lib.ctx()
    coefs, exps, counts, _ = stark.pack_step_polys(_polys(MIMC), 2)
    inp = _wire([42, 3])
    out = ctypes.create_string_buffer(64 * 10)
    n = len(out)
    INVALID, TOO_SMALL, UNSUPPORTED = -1, -5, -6
    assert L.sh_stark_witness(None, inp, 10, 2, coefs, exps, counts, 1, out, n) == INVALID
    assert L.sh_stark_witness(ctx, None, 10, 2, coefs, exps, counts, 1, out, n) == INVALID
    assert L.sh_stark_witness(ctx, inp, 10, 2, None, exps, counts, 1, out, n) == INVALID
    assert L.sh_stark_witness(ctx, inp, 10, 2, coefs, None, counts, 1, out, n) == INVALID
    assert L.sh_stark_witness(ctx, inp, 10, 2, coefs, exps, None, 1, out, n) == INVALID
    assert L.sh_stark_witness(ctx, inp, 10, 2, coefs, exps, counts, 1, None, n) == INVALID
    assert L.sh_stark_witness(ctx, inp, 0, 2, coefs, exps, counts, 1, out, n) == INVALID
    assert L.sh_stark_witness(ctx, inp, 10, 2, coefs, exps, counts, 0, out, n) == INVALID
    assert L.sh_stark_witness(ctx, inp, 10, 0, coefs, exps, counts, 1, out, n) == INVALID
    zero = (ctypes.c_uint32 * 2)(0, 0)
    assert L.sh_stark_witness(ctx, inp, 10, 2, coefs, exps, zero, 1, out, n) == INVALID
    ten = (ctypes.c_uint32 * 10)(*([1] * 10))
    assert L.sh_stark_witness(ctx, inp * 5, 10, 10, coefs * 5, bytes(100), ten, 1, out, n) == UNSUPPORTED
    many = (ctypes.c_uint32 * 2)(200, 57)
    assert L.sh_stark_witness(ctx, inp, 10, 2, bytes(32 * 257), bytes(2 * 257), many, 1, out, n) == UNSUPPORTED
    assert L.sh_stark_witness(ctx, inp, 10, 2, coefs, exps, counts, 1, out, n - 1) == TOO_SMALL
    # the device form: the same codes, and overlapping buffers
    d = ctypes.c_void_p()
    _lib.check(L.sh_dev_alloc(ctx, 64 * 11, ctypes.byref(d)), "alloc")
    try:
        w = ctypes.c_void_p(d.value + 64)
        assert L.sh_dev_stark_witness(ctx, None, 10, 2, coefs, exps, counts, 1, w) == INVALID
        assert L.sh_dev_stark_witness(ctx, d, 10, 2, coefs, exps, counts, 1, None) == INVALID
        assert L.sh_dev_stark_witness(ctx, d, 0, 2, coefs, exps, counts, 1, w) == INVALID
        assert L.sh_dev_stark_witness(ctx, d, 10, 2, coefs, exps, zero, 1, w) == INVALID
        assert L.sh_dev_stark_witness(ctx, d, 10, 10, coefs * 5, bytes(100), ten, 1, w) == UNSUPPORTED
        assert L.sh_dev_stark_witness(ctx, d, 10, 2, bytes(32 * 257), bytes(2 * 257), many, 1, w) == UNSUPPORTED
        assert L.sh_dev_stark_witness(ctx, d, 10, 2, coefs, exps, counts, 1, ctypes.c_void_p(d.value + 32)) == INVALID  # overlap
        _lib.check(L.sh_dev_from_wire(ctx, inp, d, 2), "up")
        _lib.check(L.sh_dev_stark_witness(ctx, d, 10, 2, coefs, exps, counts, 1, w), "witness")
        got = ctypes.create_string_buffer(64 * 10)
        _lib.check(L.sh_dev_to_wire(ctx, w, got, 20), "dl")
        assert got.raw == _trace_bytes([42, 3], 10, MIMC)
    finally:
        L.sh_dev_free(ctx, d)
    assert L.sh_stark_witness(ctx, inp, 10, 2, coefs, exps, counts, 1, out, n) == 0
    assert out.raw == _trace_bytes([42, 3], 10, MIMC)
