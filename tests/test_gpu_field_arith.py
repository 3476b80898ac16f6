"""Every primitive of starks_amd/csrc/fp256.cuh on the MI355X (tests/native/fp256_ops.hip --device, one element per thread) against exact
integers, in two builds: the library's flags (the inline-asm add, sub and six-limb sum with their lane masks and fp_lane_bit, the asm
products) and -DSHK_NO_ADD_ASM (the C paths behind the FP_ANY ballot).  The cases are tests/field_cases.py's: the edge set and about
10^5 random operands per op at 256-thread blocks, and the layouts -- each rare-branch vector on every lane 0..63, two rare lanes per
wave, whole rare waves, waves mixing branches, a partial last wave -- at blocks of 64, 256, 1024 and 96 threads.  Every result must
equal the model's bytes and the host mode's, the non-canonical lazily reduced representatives included."""
import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

BUILDS = {"asm": (), "no_add_asm": ("SHK_NO_ADD_ASM",)}
LAYOUT_BLOCKS = (64, 256, 1024, 96)


def _grid(n, block, extra=0):
    return (n + block - 1) // block + extra


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{build: {tag: result bytes}} for every device job, and {"host": ...}: one process per build runs every op and layout."""
    d = tmp_path_factory.mktemp("fp256_gpu")
    exes = {b: fc.build_harness(d / ("fp256_ops_" + b), defines) for b, defines in BUILDS.items()}
    jobs = []
    for op in fc.OPS:
        n = len(fc.case_set(op, "main")[0])
        jobs.append((op, "main", _grid(n, 256), 256, "%s.main.256" % op))
        n = len(fc.case_set(op, "layout")[0])
        for block in LAYOUT_BLOCKS:   # at 96 threads, one block more than needed: a whole block past the end returns at once
            jobs.append((op, "layout", _grid(n, block, block == 96), block, "%s.layout.%d" % (op, block)))
    out = {"host": fc.run_jobs(exes["asm"], "host", [(op, part, 0, 0, "%s.%s" % (op, part)) for op in fc.OPS for part in ("main", "layout")],
                               d)}
    for b in BUILDS:
        out[b] = fc.run_jobs(exes[b], "device", [j[:4] + (b + "." + j[4],) for j in jobs], d, timeout=300)
    return out


@pytest.mark.parametrize("op", sorted(fc.OPS))
@pytest.mark.parametrize("build", sorted(BUILDS))
def test_device_against_exact_integers(results, build, op):
    host = results["host"]
    for part in ("main", "layout"):
        assert host["%s.%s" % (op, part)] == fc.case_set(op, part)[2], "host: " + fc.mismatches(op, part, host["%s.%s" % (op, part)])
    got = results[build]
    for tag in ["%s.main.256" % op] + ["%s.layout.%d" % (op, b) for b in LAYOUT_BLOCKS]:
        part, block = tag.split(".")[1:]
        r = got[build + "." + tag]
        assert r == fc.case_set(op, part)[2], "%s, %s threads per block: %s" % (build, block, fc.mismatches(op, part, r, int(block)))
        assert r == host["%s.%s" % (op, part)]
