"""The generic-modulus witness generator's per-lane step, store forms and plan (starks_amd/csrc/modwitness_items.cuh) run on the host in
the kernel's decomposition (tests/native/modwitness_host.cpp, hipcc): over the whole grid of tests/modwitness_cases.py, for groups of
1 .. 16 lanes and dispatch slices 0 (default), 1 (a dispatch per step: every resume path), 3 and 7, in both store forms, every byte
equals the exact oracle (oracle/pyoracle.py with p = the modulus), which tests/golden/mod_witness.json pins to the reference.  CPU only."""
import hashlib
import os
import re
import struct
import subprocess

import pytest

import modwitness_cases as wc
from conftest import ROOT, load_golden
from oracle import pyoracle

GROUPS = (1, 2, 4, 8, 16)
SLICES = (0, 1, 3, 7)
with open(os.path.join(ROOT, "starks_amd", "csrc", "modwitness_items.cuh")) as _fh:
    SLICE_PRODUCTS = 1 << int(re.search(r"MWI_SLICE_PRODUCTS = 1u << (\d+);", _fh.read()).group(1))  # the generic path's own constant


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mwh") / "modwitness_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "modwitness_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _generate(driver, d, c, groups=(0,), slices=(0,), store=0):
    """-> {(group asked, slice asked): ((group, slice, cost) of the plan, witness bytes [batch][width][steps])}"""
    coefs, exps, counts = c.terms()
    for name, data in (("modulus", c.p.to_bytes(32, "big")), ("inputs", c.input_wire()), ("coefs", coefs), ("exps", exps),
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
    """pyoracle's trace over BN254, Goldilocks, BabyBear and P43 hashes to what the reference's get_computational_trace over
    IntegersModP(p) gave (tests/golden/generate_mod_witness.py)"""
    G = load_golden("mod_witness.json")["cases"]
    assert sorted(G) == sorted(wc.FIXTURE)
    for key, (name, sp, steps, inputs) in wc.FIXTURE.items():
        g = G[key]
        assert (g["p"], g["steps"], g["inputs"]) == (wc.MODULI[name], steps, inputs), key
        assert [{tuple(k): v for k, v in d} for d in g["step_polys"]] == sp, key
        w = pyoracle.get_computational_trace(inputs, steps, sp, wc.MODULI[name])
        assert hashlib.sha256(wc.mc.wire([v for col in w for v in col])).hexdigest() == g["sha256"], key
        assert [col[-1] for col in w] == g["last"], key


@pytest.mark.parametrize("name", sorted(wc.MODULI))
def test_grid(name, driver, tmp_path):
    """every case of the modulus, every group size and slice, both store forms"""
    cases = [c for c in wc.GRID if c.name == name]
    assert cases
    for c in cases:
        want = wc.want_wire(c)
        for store in (0, 1):
            for (g, sl), (plan, got) in _generate(driver, tmp_path, c, GROUPS, SLICES, store).items():
                assert plan[0] == g and (sl == 0 or plan[1] == sl), (c.id, g, sl, plan)
                assert got == want, (c.id, g, sl, store)


def test_default_plans(driver, tmp_path):
    """The defaults: MiMC over BN254 walks one lane per unit; the 256-term system splits over 16 lanes; a slice holds the generic
    path's own budget of sequential products divided by the plan's cost."""
    c = wc.Case("bn254", "mimc2-plan", wc.MIMC_2, 4, [[42, 3]])
    plan, got = _generate(driver, tmp_path, c)[(0, 0)]
    assert plan == (1, SLICE_PRODUCTS // 2, 2)
    assert got == wc.trace_wire(c.p, [42, 3], 4, wc.MIMC_2)
    w9 = [x for x in wc.GRID if x.id == "bn254-w9_256_terms-s70"][0]
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
    assert got == wc.want_wire(c)
