"""The run-time-modulus field arithmetic on the MI355X (tests/native/modarith_ops.hip --device, one element per thread): every function
of starks_amd/csrc/fpm.cuh and starks_amd/csrc/fp64m.cuh and the small functions the items headers build on them, in the device
compile -- __umul64hi, the uint4 accesses of mn_ld / mn_st, the modulus block as a kernel argument -- against exact integers.  The
cases are tests/modarith_cases.py's, per op and modulus: the edge set crossed, at least 8 vectors of every operand class the headers'
comments name and 20 000 random operands at 256-thread blocks, and the layouts -- class vectors on lanes 0, 31, 32 and 63, two rare
lanes per wave, whole rare waves, waves mixing classes and exponent lengths, a partial last wave -- at blocks of 64, 256, 1024 and 96
threads, the last with a whole block past the end.  One process per family runs every job; every result must equal the model's
bytes and the host mode's."""
import pytest

import modarith_cases as ma

pytestmark = pytest.mark.gpu

LAYOUT_BLOCKS = (64, 256, 1024, 96)
CASES = [(f, name, op) for f in sorted(ma.MODULI) for name in sorted(ma.MODULI[f]) for op in ma.ops_of(f, name)]


def _grid(n, block, extra=0):
    return (n + block - 1) // block + extra


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{family: {"host": {tag: bytes}, "device": {tag: bytes}}}: per family one host process and one device process run every modulus,
    op and layout, each under its time limit; a non-zero exit of either fails the module here."""
    d = tmp_path_factory.mktemp("modarith_gpu")
    exe = ma.build_harness(d / "modarith_ops")
    out = {}
    for family in sorted(ma.MODULI):
        wd = d / family
        wd.mkdir()
        host, dev = [], []
        for name in sorted(ma.MODULI[family]):
            for op in ma.ops_of(family, name):
                tag = "%s.%s" % (name, op)
                n = len(ma.operands(family, name, op, "main"))
                host.append(ma.job(family, name, op, "main", 0, 0, "host.%s.main" % tag))
                dev.append(ma.job(family, name, op, "main", _grid(n, 256), 256, "%s.main.256" % tag))
                n = len(ma.operands(family, name, op, "layout"))
                host.append(ma.job(family, name, op, "layout", 0, 0, "host.%s.layout" % tag))
                for block in LAYOUT_BLOCKS:   # at 96 threads, one block more than needed: a whole block past the end returns at once
                    dev.append(ma.job(family, name, op, "layout", _grid(n, block, block == 96), block, "%s.layout.%d" % (tag, block)))
        out[family] = {"host": ma.run_jobs(exe, "host", host, wd), "device": ma.run_jobs(exe, "device", dev, wd, timeout=300)}
    return out


@pytest.mark.parametrize("family,name,op", CASES)
def test_device_against_exact_integers(results, family, name, op):
    host, got = results[family]["host"], results[family]["device"]
    tag = "%s.%s" % (name, op)
    for part in ("main", "layout"):
        h = host["host.%s.%s" % (tag, part)]
        assert h == ma.case_set(family, name, op, part)[2], "host: " + ma.mismatches(family, name, op, part, h)
    for t in ["%s.main.256" % tag] + ["%s.layout.%d" % (tag, b) for b in LAYOUT_BLOCKS]:
        part, block = t.split(".")[-2:]
        r = got[t]
        assert r == ma.case_set(family, name, op, part)[2], "%s threads per block: %s" % (block, ma.mismatches(family, name, op, part, r, int(block)))
        assert r == host["host.%s.%s" % (tag, part)]
