"""The STARK kernel variant matrix (tests/golden/stark_variants.json): which kernel instance of starks_amd/csrc/stark.hip a batch
reaches, read from the kernel source itself, and the traces of the fixture's units.  Shared by tests/test_stark_oracle.py (CPU: the
matrix covers every cell) and tests/test_gpu_parity.py (GPU: every unit of every batch equals its fixture hash)."""
import hashlib
import os
import re
import struct

P = 2**256 - 2**32 * 351 + 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STARK_HIP = os.path.join(ROOT, "starks_amd", "csrc", "stark.hip")


def thresholds():
    """-> (wide, split, split4) in rows = steps * ext / 4 * batch, parsed from stark.hip: a launch is WIDE from STARK_WIDE_THREADS
    rows on; the quotient kernel splits rows over two lanes up to 2^SHK_STARK_SPLIT_LOG rows, the lincomb kernel over four up to half
    of that."""
    src = open(STARK_HIP).read()
    wide = re.search(r"constexpr uint64_t STARK_WIDE_THREADS = 1ull << (\d+);", src)
    split = re.search(r"#define SHK_STARK_SPLIT_LOG (\d+)", src)
    assert wide and split, "stark.hip no longer defines STARK_WIDE_THREADS / SHK_STARK_SPLIT_LOG the way this test reads them"
    # the launch conditions this classification mirrors
    assert "const bool wide = (a.n >> 2) * a.batch >= STARK_WIDE_THREADS;" in src
    assert "const bool split = (a.n >> 2) * a.batch <= STARK_SPLIT_ROWS;" in src
    assert "const bool split = (a.n >> 2) * a.batch <= STARK_SPLIT4_ROWS;" in src
    lg = int(split.group(1))
    assert lg > 0, "the split kernels are compiled out: the narrow cells below no longer exist"
    return 1 << int(wide.group(1)), 1 << lg, 1 << (lg - 1)


def rows(case):
    return case["steps"] * case["ext"] // 4 * case["batch"]


def regimes(case, th=None):
    """-> (quotient kernel, lincomb kernel) a case launches: ("narrow" | "middle" | "wide", W) and (..., 1 | 2 | 0 = generic)."""
    wide, split, split4 = th or thresholds()
    r = rows(case)
    q = "wide" if r >= wide else "narrow" if r <= split else "middle"
    lc = "wide" if r >= wide else "narrow" if r <= split4 else "middle"
    w = case["width"]
    return (q, w), (lc, w if w <= 2 else 0)


def required_cells(th=None):
    """Every cell the matrix must hold at least one case of."""
    wide, split, split4 = th or thresholds()
    cells = {("quotient", k, w) for k in ("narrow", "middle", "wide") for w in range(1, 10)}
    cells |= {("lincomb", k, w) for k in ("narrow", "middle", "wide") for w in (1, 2, 0)}
    cells |= {("band", w) for w in (1, 2, 0)}  # quotients narrow, lincomb middle
    return cells


def cells_of(case, th=None):
    th = th or thresholds()
    (q, w), (lc, lw) = regimes(case, th)
    out = {("quotient", q, w), ("lincomb", lc, lw)}
    if q == "narrow" and lc == "middle":
        out.add(("band", lw))
    return out


def boundary_rows(case, th=None):
    """The threshold rows this case sits on: 'S', 'S+1p' (one proof above S), 'S-1p' for S in the three thresholds."""
    wide, split, split4 = th or thresholds()
    one = case["steps"] * case["ext"] // 4
    r = rows(case)
    out = set()
    for name, s in (("split4", split4), ("split", split), ("wide", wide)):
        if r == s:
            out.add(name)
        elif r == s + one:
            out.add(name + "+1p")
        elif r == s - one:
            out.add(name + "-1p")
    return out


def seeded(seed, i):
    return int.from_bytes(hashlib.blake2s(struct.pack("<QQ", seed, i)).digest(), "big") % P


def unit_inputs(case, unit):
    """generate_large.variant_inputs: distinct inputs for every unit of a batch."""
    w = case["width"]
    return [seeded(case["seed"], unit * w + j) for j in range(w)]


def step_polys(case):
    return [{tuple(k): v for k, v in d} for d in case["step_polys"]]


def trace(inputs, steps, sp):
    """pyoracle.get_computational_trace (air.py:32-52), with each term's powers taken once: witness[dim][step]."""
    terms = [[(c % P, [(v, e) for v, e in enumerate(ex) if e]) for ex, c in sorted(d.items())] for d in sp]
    cur = [x % P for x in inputs]
    cols = [[x] for x in cur]
    for _ in range(steps - 1):
        nxt = []
        for tl in terms:
            y = 0
            for c, vs in tl:
                pr = c
                for v, e in vs:
                    pr = pr * (cur[v] if e == 1 else pow(cur[v], e, P)) % P
                y += pr
            nxt.append(y % P)
        cur = nxt
        for j, x in enumerate(cur):
            cols[j].append(x)
    return cols
