"""The packed-word witness generator's per-lane step, store forms and plan (starks_amd/csrc/mod64witness_items.cuh) run on the host in
the kernel's decomposition (tests/native/mod64witness_host.cpp, hipcc): over the whole grid of tests/mod64witness_cases.py, for groups
of 1 .. 16 lanes and dispatch slices 0 (default), 1 (a dispatch per step: every resume path), 3 and 7, in both store forms, every word
equals the exact oracle (oracle/pyoracle.py with p = the modulus), which tests/golden/mod64_witness.json pins to the reference.  CPU
only."""
import ctypes
import os
import re
import struct
import subprocess

import pytest

import mod64witness_cases as wc
from conftest import ROOT, load_golden
from oracle import pyoracle

GROUPS = (1, 2, 4, 8, 16)
SLICES = (0, 1, 3, 7)
CSRC = os.path.join(ROOT, "starks_amd", "csrc")
with open(os.path.join(CSRC, "mod64witness_items.cuh")) as _fh:
    SLICE_PRODUCTS = 1 << int(re.search(r"M6W_SLICE_PRODUCTS = 1u << (\d+);", _fh.read()).group(1))  # the packed path's own constant
SYMBOLS = ("sh_mod64_stark_witness", "sh_dev_mod64_stark_witness")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("m6wh") / "mod64witness_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC,
                           os.path.join(ROOT, "tests", "native", "mod64witness_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _generate(driver, d, c, groups=(0,), slices=(0,), store=0):
    """-> {(group asked, slice asked): ((group, slice, cost) of the plan, witness words [batch][width][steps])}"""
    coefs, exps, counts = c.terms()
    for name, data in (("modulus", struct.pack("<Q", c.p)), ("inputs", c.input_words()), ("coefs", coefs), ("exps", exps),
                       ("counts", struct.pack("<%dI" % c.width, *counts))):
        (d / name).write_bytes(data)
    out = subprocess.run([driver, str(d), str(c.width), str(c.steps), str(c.batch), ",".join(map(str, groups)), ",".join(map(str, slices)),
                          str(store)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    res = {}
    for line in out.stdout.splitlines():
        g, s, pg, ps, cost = (int(x) for x in line.split())
        res[(g, s)] = ((pg, ps, cost), (d / ("witness.%d.%d" % (g, s))).read_bytes())
    assert len(res) == len(groups) * len(slices)
    return res


def test_oracle_equals_the_reference():
    """pyoracle's trace over Goldilocks, BabyBear, BIG18 and 2^64 - 1, as words, hashes to what the reference's get_computational_trace
    over IntegersModP(p) gave (tests/golden/generate_mod64_witness.py)"""
    G = load_golden("mod64_witness.json")["cases"]
    assert sorted(G) == sorted(wc.FIXTURE)
    for key, (name, sp, steps, inputs) in wc.FIXTURE.items():
        g = G[key]
        assert (g["p"], g["steps"], g["inputs"]) == (wc.MODULI[name], steps, inputs), key
        assert [{tuple(k): v for k, v in d} for d in g["step_polys"]] == sp, key
        w = pyoracle.get_computational_trace(inputs, steps, sp, wc.MODULI[name])
        assert wc.sha(wc.words([v for col in w for v in col])) == g["sha256"], key
        assert [col[-1] for col in w] == g["last"], key


def test_fixture_hashes(driver, tmp_path):
    """the driver's default run on the four fixture cases hashes to the reference's digests"""
    G = load_golden("mod64_witness.json")["cases"]
    for key, (name, sp, steps, inputs) in wc.FIXTURE.items():
        c = wc.Case(name, "fixture-" + key, sp, steps, [inputs])
        plan, got = _generate(driver, tmp_path, c)[(0, 0)]
        assert wc.sha(got) == G[key]["sha256"], key
        assert wc.ints(got)[steps - 1::steps] == G[key]["last"], key


@pytest.mark.parametrize("name", sorted(wc.MODULI))
def test_grid(name, driver, tmp_path):
    """every case of the modulus, every group size and slice, both store forms"""
    cases = [c for c in wc.GRID if c.name == name]
    assert cases
    for c in cases:
        want = wc.want_words(c)
        for store in (0, 1):
            for (g, sl), (plan, got) in _generate(driver, tmp_path, c, GROUPS, SLICES, store).items():
                assert plan[0] == g and (sl == 0 or plan[1] == sl), (c.id, g, sl, plan)
                assert got == want, (c.id, g, sl, store)


def test_grid_covers_what_it_must():
    """a guard on the case table itself (tests/mod64witness_cases.py), not on the code: it keeps a later edit from dropping a case"""
    ids = {c.id for c in wc.GRID}
    assert sorted(wc.MODULI.values()) == sorted([wc.GOLDILOCKS, wc.BIG18, 2013265921, 2130706433, 65537, 257, 17, 3, 15, 2**64 - 1])
    for name in wc.MODULI:
        for sys_steps in ("linear1-s7", "mimc2-s65", "mixed3-s33", "quintic9-s9", "zero2-s5", "stored_plus_p-s100"):
            assert "%s-%s" % (name, sys_steps) in ids
        for tag, _, _ in wc.edge_systems(wc.MODULI[name]):
            for steps in (1, 3, 1000):
                assert "%s-%s-s%d" % (name, tag, steps) in ids
        c = [x for x in wc.GRID if x.id == name + "-stored_plus_p-s100"][0]
        assert [2**64 - 1, 2**64 - 2] in c.inputs
        if 2 * c.p < 2**64:
            assert c.inputs[0] == [42 % c.p + c.p, 3 % c.p + c.p]
    assert {"goldilocks-w9_256_terms-s70", "allones-w9_256_terms-s70"} <= ids
    assert (wc.HEAVY_CASE.p, wc.HEAVY_CASE.steps) == (wc.BIG18, 3)


def test_default_plans(driver, tmp_path):
    """The defaults: MiMC over Goldilocks walks one lane per unit; the 256-term system splits over 16 lanes; a slice holds the packed
    path's own budget of sequential products divided by the plan's cost."""
    c = wc.Case("goldilocks", "mimc2-plan", wc.MIMC_2, 4, [[42, 3]])
    plan, got = _generate(driver, tmp_path, c)[(0, 0)]
    assert plan == (1, SLICE_PRODUCTS // 2, 2)
    assert got == wc.trace_words(c.p, [42, 3], 4, wc.MIMC_2)
    w9 = [x for x in wc.GRID if x.id == "goldilocks-w9_256_terms-s70"][0]
    res = _generate(driver, tmp_path, w9, (0, 1), (0,))
    plan, one = res[(0, 0)][0], res[(1, 0)][0]
    assert plan[0] == 16 and plan[1] == SLICE_PRODUCTS // plan[2]
    assert one[2] >= 4 * plan[2], (one, plan)


@pytest.mark.parametrize("group", [1, 2])
def test_steps_longer_than_a_dispatch_budget(driver, tmp_path, group):
    """A step that costs more than a dispatch's budget still gets a slice of one step (the default slice never rounds down to 0)."""
    c = wc.HEAVY_CASE
    assert sum(len(d) for d in c.sp) == 256
    plan, got = _generate(driver, tmp_path, c, (group,), (0,))[(group, 0)]
    assert plan[0] == group and plan[1] == 1 and plan[2] > SLICE_PRODUCTS, plan
    assert got == wc.want_words(c)


def test_library_cross_compiles():
    """the two new translation units for gfx950, and the symbols the header declares in the built library"""
    for src in ("mod64witness.hip", "api_mod64stark.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in SYMBOLS:
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header


def test_python_length_checks(monkeypatch):
    """without a device: mod64_witness_flat and mod64_prove_input_words_flat refuse buffers of the wrong length before asking for a
    context"""
    from starks_amd import IntegersModP, _lib, stark
    from starks_amd.multivariate_polynomial import multivariates_over
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("a length error must not ask for a context"))
    F = IntegersModP(wc.GOLDILOCKS)
    mv = multivariates_over(F, 2).factory
    sp = [mv({k: F(v) for k, v in d.items()}) for d in wc.MIMC_2]
    with pytest.raises(ValueError):
        stark.mod64_witness_flat(wc.GOLDILOCKS, [1, 2, 3], 8, 2, sp)
    with pytest.raises(ValueError):
        stark.mod64_witness_flat(wc.GOLDILOCKS, bytes(15), 8, 2, sp)
    with pytest.raises(ValueError):
        stark.mod64_witness_flat(wc.GOLDILOCKS, [1, 2], 8, 2, sp, batch=2)
    with pytest.raises(ValueError):
        stark.mod64_prove_input_words_flat(wc.GOLDILOCKS, [1, 2, 3], 8, 8, 2, sp)
    with pytest.raises(ValueError):
        stark.mod64_prove_input_words_flat(wc.GOLDILOCKS, bytes(24), 8, 8, 2, sp, batch=2)
