"""The device witness generator's per-lane step and plan (starks_amd/csrc/witness_items.cuh) run on the host in the kernel's decomposition
(tests/native/witness_host.cpp, hipcc): for groups of 1 .. 16 lanes and several dispatch slices, the witness equals the reference's
traces byte for byte -- the witness arrays of tests/golden/stark.json, the units of the variant matrix, and edge systems.  CPU only."""
import os
import subprocess

import pytest

import stark_variants as sv
from conftest import ROOT, load_golden

P = sv.P
GROUPS = (1, 2, 4, 8, 16)


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


def _wire(vals):
    return b"".join((int(v) % P).to_bytes(32, "big") for v in vals)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wh") / "witness_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "witness_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _generate(driver, d, sp, width, steps, input_bytes, batch, group=0, slice_=0):
    """-> ((group, slice, cost) of the plan, witness bytes [batch][width][steps])"""
    from starks_amd import stark
    coefs, exps, counts, _ = stark.pack_step_polys([_Poly(x) for x in sp], width)
    for name, data in (("inputs", input_bytes), ("coefs", coefs), ("exps", exps), ("counts", bytes(counts))):
        (d / name).write_bytes(data)
    out = subprocess.run([driver, str(d), str(width), str(steps), str(batch), str(group), str(slice_)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    plan = tuple(int(x) for x in out.stdout.split())
    return plan, (d / "witness").read_bytes()


def _want(inputs, steps, sp):
    return b"".join(_wire(col) for col in sv.trace(inputs, steps, sp))


STARK_CASES = load_golden("stark.json")


@pytest.mark.parametrize("c", STARK_CASES, ids=lambda c: c["name"])
def test_reference_witness_arrays(c, driver, tmp_path):
    """Every group size and several slices (1 = a dispatch per step) against the reference's own witness (AIR.generate_witness)."""
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    want = b"".join(bytes.fromhex(v) for col in c["witness"] for v in col)
    assert want == _want(c["inputs"], c["steps"], sp)
    for g in GROUPS:
        for sl in (0, 1, 3, 7):
            plan, got = _generate(driver, tmp_path, sp, c["width"], c["steps"], _wire(c["inputs"]), 1, g, sl)
            assert plan[0] == g and (sl == 0 or plan[1] == sl)
            assert got == want, (c["name"], g, sl)


@pytest.mark.parametrize("c", load_golden("stark_variants.json")["cases"], ids=lambda c: c["name"])
def test_variant_units(c, driver, tmp_path):
    """The first and last unit of every batch of the variant matrix (widths 1 .. 9, the 256-term system), 512 steps at most, under the
    default plan and under one forced group and slice per case."""
    steps = min(c["steps"], 512)
    sp = sv.step_polys(c)
    units = [0, c["batch"] - 1]
    ins = [sv.unit_inputs(c, u) for u in units]
    want = b"".join(_want(i, steps, sp) for i in ins)
    k = sum(map(ord, c["name"]))
    for g, sl in ((0, 0), (GROUPS[k % 5], (5, 64, 100)[k % 3])):
        _, got = _generate(driver, tmp_path, sp, c["width"], steps, b"".join(_wire(i) for i in ins), len(units), g, sl)
        assert got == want, (c["name"], g, sl)


def test_default_plans(driver, tmp_path):
    """The defaults the library chooses: MiMC walks one lane per unit (its 2 products per step gain nothing from a split); the 256-term
    system splits over 16 lanes; a slice holds about 2^13 sequential products."""
    mimc = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]
    plan, _ = _generate(driver, tmp_path, mimc, 2, 4, _wire([42, 3]), 1)
    assert plan == (1, (1 << 13) // 2, 2)
    c = [x for x in load_golden("stark_variants.json")["cases"] if x["name"] == "w9_256_terms"][0]
    plan, _ = _generate(driver, tmp_path, sv.step_polys(c), 9, 2, _wire(sv.unit_inputs(c, 0)), 1)
    assert plan[0] == 16 and plan[1] == (1 << 13) // plan[2]
    one, _ = _generate(driver, tmp_path, sv.step_polys(c), 9, 2, _wire(sv.unit_inputs(c, 0)), 1, 1)
    assert one[2] >= 4 * plan[2], (one, plan)


# 256 terms, every exponent 255, coefficient 2: one step is about 34600 products on one lane, more than a dispatch's budget
HEAVY = [{tuple((t * 7 + v) % 256 if v == t % 9 else 255 for v in range(9)): 2 for t in range(c, 256, 9)} for c in range(9)]


@pytest.mark.parametrize("group", [1, 2])
def test_steps_longer_than_a_dispatch_budget(driver, tmp_path, group):
    """A step that costs more than a dispatch's budget still gets a slice of one step (the default slice never rounds down to 0)."""
    assert sum(len(d) for d in HEAVY) == 256
    ins = [list(range(2, 11))]
    plan, got = _generate(driver, tmp_path, HEAVY, 9, 3, _wire(ins[0]), 1, group)
    assert plan[0] == group and plan[1] == 1 and plan[2] > 1 << 13, plan
    assert got == _want(ins[0], 3, HEAVY)


EDGES = [
    # (name, width, step polynomials, inputs of two units)
    ("zero_polynomial", 2, [{}, {(1, 1): 1}], [[5, 7], [0, 1]]),
    ("coefficients_0_and_p_minus_1", 2, [{(1, 0): P - 1, (0, 1): 0}, {(1, 1): P - 1, (0, 0): 3}], [[5, 7], [P - 1, 2]]),
    ("exponent_255", 2, [{(255, 0): 1}, {(3, 255): 2, (0, 0): 1}], [[3, 5], [P - 2, 1]]),
    ("fib_from_zero", 2, [{(0, 1): 1}, {(0, 1): 1, (1, 0): 1}], [[0, 1], [0, 0]]),
    ("constant_terms_only", 3, [{(0, 0, 0): 9}, {(0, 0, 0): 1}, {(0, 0, 0): 0}], [[1, 2, 3], [0, 0, 0]]),
    ("width_9_dense", 9, [{tuple(int(v == c or v == (c + 1) % 9) * (1 + (c % 3)) for v in range(9)): c + 1, (0,) * 9: c} for c in range(9)],
     [list(range(1, 10)), [0] * 9]),
]


@pytest.mark.parametrize("name,width,sp,ins", EDGES, ids=[e[0] for e in EDGES])
def test_edge_systems(name, width, sp, ins, driver, tmp_path):
    for steps in (1, 3, 1000):
        want = b"".join(_want(i, steps, sp) for i in ins)
        for g, sl in ((0, 0), (2, 3), (16, 1)):
            _, got = _generate(driver, tmp_path, sp, width, steps, b"".join(_wire(i) for i in ins), 2, g, sl)
            assert got == want, (name, steps, g, sl)


def test_unreduced_inputs(driver, tmp_path):
    """Inputs >= p (x + p, still below 2^256) give the witness of x; row 0 is stored reduced."""
    sp = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]
    raw = (42 + P).to_bytes(32, "big") + (P + 3).to_bytes(32, "big")
    for g in GROUPS:
        _, got = _generate(driver, tmp_path, sp, 2, 1000, raw, 1, g, 64)
        assert got == _want([42, 3], 1000, sp), g
