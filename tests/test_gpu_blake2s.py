"""Every form of starks_amd/csrc/blake2s.cuh, and sample_indices_quad, on the MI355X (tests/native/blake2s_ops.hip --device) in nine
builds: the library's defaults (the generated single-lane asm rounds, the quad-lane asm half-rounds), -DB2_NO_ASM, -DB2Q_NO_ASM, both,
and the generator's other forms of the single-lane rounds (--two-adds, --no-branch, --e64, --align, --sdwa16, through -DB2_ASM_INC).
Each build runs every op and layout of tests/hash_cases.py in one process: single-lane pair and short hashes; block chains of 1..255
compressions with one k per wave and with every lane its own k (the asm rounds under a changing exec mask); vb_hash_two up to 27
blocks; the quad-lane compression at blocks of 64, 256 and 512 threads with every quad live, with power-of-two prefixes of live quads
and with a partial last block; the sampler over its argument grid with dead quads in the last block.  Every record must equal
hashlib.blake2s / get_pseudorandom_indices bytes, and, for the ops that have a host path, the host mode's.  Records that a kernel
must not write must still hold the 0xa5 fill."""
import time

import pytest

import hash_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """{build: {tag: result bytes}} for every device job, and {"host": ...}.  Every harness is built before any process opens the GPU."""
    d = tmp_path_factory.mktemp("blake2s_gpu")
    t0 = time.time()
    exes = hc.build_all(d)
    t1 = time.time()
    host_jobs = [(op, part, 0, 0, "%s.%s" % (op, part)) for op in hc.HOST_OPS for part in hc.PARTS[op]]
    out = {"host": hc.run_jobs(exes["default"], "host", host_jobs, d, timeout=300)}
    jobs = hc.device_jobs()
    for b in hc.BUILDS:
        out[b] = hc.run_jobs(exes[b], "device", [j[:4] + (b + "." + j[4],) for j in jobs], d, timeout=120)
    print("\nblake2s_ops: %d builds in %.1f s, %d device runs in %.1f s" % (len(exes), t1 - t0, len(hc.BUILDS), time.time() - t1))
    return out


@pytest.mark.parametrize("op", sorted(hc.OPS))
@pytest.mark.parametrize("build", sorted(hc.BUILDS))
def test_device_against_hashlib(results, build, op):
    host = results["host"]
    for op_, part, _, block, tag in hc.device_jobs():
        if op_ != op:
            continue
        got = results[build][build + "." + tag]
        assert got == hc.case_set(op, part)[2], "%s, %d threads per block: %s" % (build, block, hc.mismatches(op, part, got, block))
        if op in hc.HOST_OPS:
            assert got == host["%s.%s" % (op, part)]
