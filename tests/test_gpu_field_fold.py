"""The fold of fp_add / fp_sub on the MI355X (starks_amd/csrc/fp256.cuh, gen_addasm.py: limb 0 minus the carry, limb 1 plus 0x15f times
the carry minus that borrow, the rare lanes as a scalar mask) against Python integers, through tests/native/fp256_ops.hip --device.

The grid is laid over the eight-limb sum (difference) s as it stands before the fold: limb 1 at 0, 1, c's limb 1 and its neighbours
(0x15e, 0x15f, 0x160), the carry threshold 2^32 - 0x15f and its neighbours, all ones; limb 0 at 0, 1, 2^32 - 2, 2^32 - 1; limbs 2..7 all
zero, all ones, or seeded; and operands a, b that reach s with the carry (borrow) out of limb 7 set and clear -- the two combinations
no operands reach (a sum of 2^257 - 1, a borrow with difference 0) are left out.  The grid fills whole waves, one element per lane.
Then a sweep: one wave per lane position, that lane alone holding a grid case whose fold leaves limb 1 (the wave-uniform branch is
taken for one lane, its 63 neighbours are grid cases that stay on the common path); the rare cases take turns."""
import os
import random

import pytest

import native_harness

pytestmark = pytest.mark.gpu

P = 2**256 - 2**32 * 351 + 1
M = 1 << 256
C = M - P
LIMB1 = (0, 1, 0x15e, 0x15f, 0x160, 0xfffffea0, 0xfffffea1, 0xfffffea2, 0xffffffff)
LIMB0 = (0, 1, 0xfffffffe, 0xffffffff)
HARNESS = os.path.join(native_harness.ROOT, "tests", "native", "fp256_ops.hip")


def m_add(a, b):
    v = a + b
    while v >= M:           # 2^256 == c
        v = (v & (M - 1)) + (v >> 256) * C
    return v


def m_sub(a, b):
    d = a - b
    while d < 0:            # d + 2^256 - c
        d += P
    return d


def _operands(op, s, top, rng):
    """a, b in [0, 2^256) whose 256-bit sum (difference) is s with the carry (borrow) out of limb 7 equal to `top`, or None"""
    if op == "add":
        if top:
            if s > M - 2:
                return None
            a = rng.randrange(s + 1, M)
            return a, M + s - a
        a = rng.randrange(0, s + 1)
        return a, s - a
    if top:
        if s == 0:
            return None
        a = rng.randrange(0, s)
        return a, a + M - s
    a = rng.randrange(s, M)
    return a, a - s


def _leaves_limb1(op, s, top):
    """does the fold of +c (-c) into limbs 0..1 carry (borrow) out of limb 1?"""
    if not top:
        return False
    lo = s & ((1 << 64) - 1)
    return lo + C >= 1 << 64 if op == "add" else lo < C


def _cases(op):
    rng = random.Random("fold:" + op)
    seeded = rng.getrandbits(192)
    grid = []
    for l1 in LIMB1:
        for l0 in LIMB0:
            for upper in (0, (1 << 192) - 1, seeded):
                for top in (0, 1):
                    s = l0 | (l1 << 32) | (upper << 64)
                    ab = _operands(op, s, top, rng)
                    if ab is not None:
                        grid.append((ab, _leaves_limb1(op, s, top)))
    rare = [ab for ab, r in grid if r]
    common = [ab for ab, r in grid if not r]
    assert len(grid) == 9 * 4 * 3 * 2 - 1 and len(rare) >= 12 and len(common) >= 63
    cases = [ab for ab, _ in grid]
    cases += common[:64 - len(cases) % 64]      # the grid ends on a wave boundary
    assert len(cases) % 64 == 0
    k = 0
    for lane in range(64):
        for j in range(64):
            if j == lane:
                cases.append(rare[lane % len(rare)])
            else:
                cases.append(common[k % len(common)])
                k += 1
    return cases


def _encode(cases):
    return b"".join(a.to_bytes(32, "little") + b.to_bytes(32, "little") for a, b in cases)


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("fp256_fold")
    exe = native_harness.build(HARNESS, d / "fp256_ops")
    cases = {op: _cases(op) for op in ("add", "sub")}
    jobs = [(op, "fold", (len(cases[op]) + 63) // 64, 64, op) for op in cases]     # one launch per op, a wave per block
    got = native_harness.run_jobs(exe, "device", jobs, d, lambda op, part: (len(cases[op]), _encode(cases[op])), timeout=120)
    return cases, got


@pytest.mark.parametrize("op", ["add", "sub"])
def test_fold_against_integers(results, op):
    cases, got = results
    model = m_add if op == "add" else m_sub
    assert len(got[op]) == 32 * len(cases[op])
    bad = []
    for i, (a, b) in enumerate(cases[op]):
        want = model(a, b)
        assert want % P == ((a + b) if op == "add" else (a - b)) % P
        r = int.from_bytes(got[op][32 * i:32 * i + 32], "little")
        if r != want:
            bad.append("element %d (wave %d lane %d): %#x %s %#x: got %#x want %#x" % (i, i // 64, i % 64, a, op, b, r, want))
    assert not bad, "%d of %d differ: %s" % (len(bad), len(cases[op]), "; ".join(bad[:4]))
