"""Cases, inputs and expected bytes for every Merkle tree form and the FRI fold of starks_amd/csrc/kernels.hip, as run by
tests/native/tree_ops.hip.  Shared by tests/test_trees_host.py (CPU: the harness builds and refuses bad jobs, the grid covers every
form, the expectations agree with each other) and tests/test_gpu_trees.py (GPU: the whole grid, node for node).

Which kernels a case launches is read from kernels.hip itself (thresholds(), cells_of()): the dispatch's constants are parsed and
its launch conditions asserted word for word, so a change to the dispatch fails here instead of leaving a form untested.

Expected trees are hashlib.blake2s (small trees) or oracle/oracle.c's or_merkelize (large ones) over the leaves; a limb-form leaf
hashes as its canonical bytes, v % p.  Fold columns are oracle.pyoracle.fri_fold (exact Lagrange over ints) for small n and the C
oracle's fold for large n, with the round's generator w0^(2^round_shift).  Packed trees are pyoracle.merkelize_polynomial_evaluations.
Output buffers start as 0xa5 bytes: what a form must not write (the leaf level of the forms that do not store it) is expected as
0xa5 bytes."""
import functools
import hashlib
import os
import random
import re

import numpy as np

import native_harness

ROOT = native_harness.ROOT
HARNESS = os.path.join(ROOT, "tests", "native", "tree_ops.hip")
KERNELS = os.path.join(native_harness.CSRC, "kernels.hip")

P = 2**256 - 2**32 * 351 + 1
M = 2**256
EDGES = (0, 1, P - 1, P, P + 1, M - 1)
CHALLENGES = (P, P + 1, M - 1)
SENTINEL = b"\xa5"
SMALL_TREE = 16  # trees up to this many leaves are hashed with hashlib, larger ones by the C oracle
SMALL_FOLD = 1 << 10  # folds up to this many values use the exact Lagrange route of pyoracle, larger ones the C oracle
FORMS = {"raw": 3, "limb": 1, "nostore": 0}  # the harness's tree form: 2 raw + store
TPB = 256


# ---- the dispatch, read from kernels.hip ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def thresholds():
    """-> {"wide": MERKLE_WIDE_THREADS, "mid": 2^MID_MIN_LOG, "serial": MERKLE_SERIAL_MAX_LEAVES, "tpb": TPB} from kernels.hip, after
    checking that its launch conditions are still the ones cells_of() mirrors"""
    src = open(KERNELS).read()
    wide = re.search(r"constexpr uint64_t MERKLE_WIDE_THREADS = 1ull << (\d+);", src)
    mid = re.search(r"constexpr int MID_MIN_LOG = (\d+);", src)
    serial = re.search(r"constexpr uint64_t MERKLE_SERIAL_MAX_LEAVES = 1ull << (\d+);", src)
    tpb = re.search(r"constexpr int TPB = (\d+);", src)
    assert wide and mid and serial and tpb, "kernels.hip no longer defines the Merkle thresholds the way this file reads them"
    conditions = [
        "if (!raw_leaves && !store_leaves && n * batch <= MERKLE_SERIAL_MAX_LEAVES) {",
        "const bool wide = (n >> 2) * batch >= MERKLE_WIDE_THREADS;",
        "while (L >= 2 && ((1ull << (L - 2)) * batch) >= (1ull << MID_MIN_LOG)) {",
        "if (((1ull << (L - 2)) * batch) >= MERKLE_WIDE_THREADS / 2)",
        "if (q < 4 || q * a.batch > MERKLE_SERIAL_MAX_LEAVES) {",
        "const int launches = (L + 7) / 8, levels = (L + launches - 1) / launches;",
        "const int launches = ((int)logn + 7) / 8, levels = ((int)logn + launches - 1) / launches;",
        "const int launches = ((int)logq + 7) / 8, levels = ((int)logq + launches - 1) / launches;",
        "return merkle_serial_levels((int)logn - levels, n, batch, d_nodes, st);",
        "return merkle_serial_levels((int)logq - levels, q, a.batch, d_nodes2, st);",
        "return shk_merkelize(a.column, false, q, a.batch, d_nodes2, st, false);",
        "return shk_merkle_upper_levels(n, 1, d_nodes, st);",
    ]
    for c in conditions:
        assert c in src, "kernels.hip's Merkle dispatch changed (%r): update tree_cases.cells_of" % c
    # every serial entry launches the 128-quad kernel for a step of 8 levels and the 64-quad one below that
    for leaves in ("TOP_FROM_NODES", "TOP_FROM_VALUES", "TOP_FROM_FOLD"):
        pat = r"if \(levels == 8\)\s+hipLaunchKernelGGL\(\(merkle_top_kernel<128, %s>\)[^;]*;\s+else\s+hipLaunchKernelGGL\(\(merkle_top_kernel<64, %s>\)" % (
            leaves, leaves)
        assert re.search(pat, src), "the quad size of merkle_top_kernel<%s> is no longer chosen by levels == 8" % leaves
    return {"wide": 1 << int(wide.group(1)), "mid": 1 << int(mid.group(1)), "serial": 1 << int(serial.group(1)),
            "tpb": int(tpb.group(1))}


def log2(n):
    assert n & (n - 1) == 0 and n > 0
    return n.bit_length() - 1


def first_step(levels_total):
    """levels of the first launch of a serial part of levels_total levels (8 per launch at most, dealt evenly)"""
    launches = (levels_total + 7) // 8
    return (levels_total + launches - 1) // launches


def quads(levels):
    return 128 if levels == 8 else 64


def serial_cells(L):
    out = set()
    if L <= 0:
        return out
    out.add(("serial", "levels", L))
    out.add(("serial", "launches", (L + 7) // 8))
    while L > 0:
        s = first_step(L)
        out.add(("serial", "quads", quads(s)))
        L -= s
    return out


def upper_cells(n, batch, th):
    out = set()
    L = log2(n) - 2
    while L >= 2 and (1 << (L - 2)) * batch >= th["mid"]:
        cnt = 1 << (L - 2)
        wide = "wide" if cnt * batch >= th["wide"] // 2 else "narrow"
        out.add(("mid", wide, "one" if cnt == 1 else "full" if cnt >= th["tpb"] else "partial"))
        L -= 2
    return out | serial_cells(L)


def tree_cells(n, batch, form, th):
    if form == "nostore" and n * batch <= th["serial"]:
        s = first_step(log2(n))
        return {("values", quads(s))} | serial_cells(log2(n) - s)
    wide = "wide" if (n >> 2) * batch >= th["wide"] else "narrow"
    return {("leaf", form, wide)} | upper_cells(n, batch, th)


def cells_of(case, th=None):
    """the kernel forms a case launches"""
    th = th or thresholds()
    op, n, batch = case["op"], case["n"], case["batch"]
    if op == "tree":
        return tree_cells(n, batch, case["form"], th)
    if op == "packed":
        return {("packed", "k", case["k"]), ("packed", "n", n)} | upper_cells(n, 1, th)
    out = {("fold", "round_shift", "0" if case["round_shift"] == 0 else ">0"), ("fold", "hi", "present" if case["hi"] else "absent"),
           ("fold", "challenge", "nodes" if case["from_nodes"] else "special_x")}
    if op == "fold":
        return out
    q = n // 4
    if q < 4 or q * batch > th["serial"]:
        return out | {("foldtree", "unfused")} | tree_cells(q, batch, "nostore", th)
    s = first_step(log2(q))
    return out | {("foldtree", "fused", quads(s))} | serial_cells(log2(q) - s)


def required_cells(th=None):
    th = th or thresholds()
    cells = {("leaf", f, w) for f in FORMS for w in ("wide", "narrow")}
    cells |= {("values", 64), ("values", 128)}
    # a wide mid launch with one parent per tree needs batch >= MERKLE_WIDE_THREADS / 2 trees: more than a grid's y dimension holds
    cells |= {("mid", w, g) for w in ("wide", "narrow") for g in ("full", "partial", "one")} - {("mid", "wide", "one")}
    cells |= {("serial", "levels", L) for L in range(1, 17)}
    cells |= {("serial", "quads", 64), ("serial", "quads", 128), ("serial", "launches", 1), ("serial", "launches", 2)}
    cells |= {("foldtree", "fused", 64), ("foldtree", "fused", 128), ("foldtree", "unfused")}
    cells |= {("fold", "round_shift", s) for s in ("0", ">0")} | {("fold", "hi", h) for h in ("absent", "present")}
    cells |= {("fold", "challenge", c) for c in ("special_x", "nodes")}
    cells |= {("packed", "k", k) for k in (1, 2, 3, 7, 8, 16)} | {("packed", "n", 4)}
    return cells


# ---- the grid ------------------------------------------------------------------------------------------------------------------
def _tree(name, n, batch, form):
    return {"name": name, "op": "tree", "n": n, "batch": batch, "form": form}


def _fold(name, op, n, batch, log_n0, lb, hi, from_nodes, sx=None):
    return {"name": name, "op": op, "n": n, "batch": batch, "log_n0": log_n0, "lb": lb, "round_shift": log_n0 - log2(n), "hi": hi,
            "from_nodes": from_nodes, "sx": sx}


@functools.lru_cache(None)
def cases():
    out = [
        # batches: leaf kernels wide and narrow in each form, the mid kernel's partial workgroups and single parents
        _tree("raw_4k_x1024", 1 << 12, 1024, "raw"),        # leaf wide; mid wide full, narrow partial; serial 6
        _tree("limb_1k_x4096", 1 << 10, 4096, "limb"),      # leaf wide; mid wide partial, narrow partial; serial 4
        _tree("nostore_64_x32k", 64, 1 << 15, "nostore"),   # leaf wide; mid narrow partial, narrow one
        _tree("raw_16_x32k", 16, 1 << 15, "raw"),           # leaf narrow; mid narrow one
        _tree("limb_4k_x256", 1 << 12, 256, "limb"),        # leaf narrow; mid narrow full; serial 8
        _tree("limb_4k_x512", 1 << 12, 512, "limb"),        # leaf wide from 2^19 rows exactly
        _tree("nostore_4k_x16", 1 << 12, 16, "nostore"),    # leaf narrow; serial 10 over 16 trees
        _tree("nostore_1k_x33", 1 << 10, 33, "nostore"),    # just above the serial-from-values limit
        _tree("raw_4_x1", 4, 1, "raw"), _tree("limb_4_x5", 4, 5, "limb"), _tree("nostore_4_x64", 4, 64, "nostore"),
        # serial from the values
        _tree("values_128_x256", 1 << 7, 256, "nostore"), _tree("values_256_x128", 1 << 8, 128, "nostore"),
        _tree("values_32k_x1", 1 << 15, 1, "nostore"), _tree("values_8k_x4", 1 << 13, 4, "nostore"),
        _tree("values_512_x2", 1 << 9, 2, "nostore"), _tree("values_1k_x32", 1 << 10, 32, "nostore"),
        _tree("limb_128_x3", 1 << 7, 3, "limb"), _tree("raw_32k_x2", 1 << 15, 2, "raw"),
    ]
    # one tree per remaining serial level count 1 .. 16 (log n = L + 2: no mid launch), the forms taking turns
    for L in range(1, 17):
        out.append(_tree("serial%d" % L, 1 << (L + 2), 1, ("raw", "limb")[L % 2]))
    out += [
        _fold("fold_1k", "fold", 1 << 10, 1, 10, 10, False, False, M - 1),
        _fold("fold_256_x8_nodes_hi", "fold", 1 << 8, 8, 12, 6, True, True),
        _fold("fold_64_x64_hi", "fold", 64, 64, 8, 4, True, False, P),
        _fold("fold_4k_x4_nodes", "fold", 1 << 12, 4, 13, 13, False, True),
        _fold("fold_16k_x2_hi", "fold", 1 << 14, 2, 16, 8, True, False, P + 1),
        _fold("fold_4_x3", "fold", 4, 3, 4, 2, True, False, 5),
        _fold("foldtree_64_x4_nodes", "foldtree", 64, 4, 8, 8, False, True),
        _fold("foldtree_1k_x16_hi", "foldtree", 1 << 10, 16, 10, 5, True, False, 12345),
        _fold("foldtree_128k_x1", "foldtree", 1 << 17, 1, 17, 9, True, True),
        _fold("foldtree_32k_x2", "foldtree", 1 << 15, 2, 15, 15, False, False, M - 1),
        _fold("foldtree_16k_x16", "foldtree", 1 << 14, 16, 16, 8, True, True),
        _fold("foldtree_16_x8", "foldtree", 16, 8, 4, 4, False, False, P),
        _fold("foldtree_512_x64", "foldtree", 1 << 9, 64, 11, 6, True, True),
    ]
    for n, k in ((4, 1), (8, 2), (64, 3), (1 << 10, 7), (16, 8), (256, 16), (4, 16), (1 << 12, 3), (4, 7), (1 << 13, 1)):
        out.append({"name": "packed_%d_k%d" % (n, k), "op": "packed", "n": n, "batch": 1, "k": k})
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return [c for c in cases() if c["name"] == name][0]


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _rng(c, what):
    return random.Random("%s/%s" % (c["name"], what))


def _edge_rows(q):
    """rows that get edge values: the first rows, the first and last of each of the first two workgroups, and the last rows"""
    rows = [0, 1, 2, 3, 4, 5, TPB - 1, TPB, 2 * TPB - 1, q - 2, q - 1]
    return sorted({r for r in rows if 0 <= r < q})


def _put(buf, idx, v):
    buf[32 * idx:32 * idx + 32] = v.to_bytes(32, "big")


def values(c, b, n=None, what="values"):
    """the n wire values of tree / column b: distinct, seeded; each edge value in every quarter of a permute4 row, on the first and
    last rows of workgroups; a few random values in [p, 2^256)"""
    n = n or c["n"]
    rng = _rng(c, "%s/%d" % (what, b))
    buf = bytearray(rng.randbytes(32 * n))
    q = n // 4
    for k, r in enumerate(_edge_rows(q)):
        for j in range(4):
            _put(buf, r + j * q, EDGES[(k + j + b) % len(EDGES)])
    for _ in range(min(8, n // 8)):
        _put(buf, rng.randrange(n), P + rng.randrange(M - P))
    return bytes(buf)


def canonical(wire):
    """the wire values reduced mod p (only values >= p change: their first word is 0xffffffff)"""
    a = np.frombuffer(wire, dtype=">u4").reshape(-1, 8)
    cand = np.nonzero(a[:, 0] == 0xffffffff)[0]
    if not len(cand):
        return wire
    buf = bytearray(wire)
    for i in cand.tolist():
        v = int.from_bytes(buf[32 * i:32 * i + 32], "big")
        if v >= P:
            _put(buf, i, v - P)
    return bytes(buf)


def root_of(n):
    return pow(7, (P - 1) // n, P)


def fold_tables(c):
    """(lo, hi or None, inv_i) for w0 of order 2^log_n0; lo[0] is 1 + p, an unreduced one"""
    n0 = 1 << c["log_n0"]
    w0 = root_of(n0)
    lo, x = [], 1
    for _ in range(1 << c["lb"]):
        lo.append(x)
        x = x * w0 % P
    lo[0] = 1 + P
    hi = None
    if c["hi"]:
        step, hi, y = pow(w0, 1 << c["lb"], P), [], 1
        for _ in range(1 << (c["log_n0"] - c["lb"])):
            hi.append(y)
            y = y * step % P
    return lo, hi, pow(w0, 3 * n0 // 4, P)


def challenges(c):
    """the challenge of each batch b, as 32 bytes: special_x for all, or node 1 of tree b (p, p+1, 2^256-1, then random)"""
    if not c["from_nodes"]:
        return [c["sx"].to_bytes(32, "big")] * c["batch"]
    rng = _rng(c, "nodes")
    return [(CHALLENGES[b] if b < len(CHALLENGES) else rng.randrange(M)).to_bytes(32, "big") for b in range(c["batch"])]


def _w32(v):
    return int(v).to_bytes(32, "big")


def job_input(name):
    c = case(name)
    if c["op"] == "tree":
        return b"".join(values(c, b) for b in range(c["batch"]))
    if c["op"] == "packed":
        return b"".join(values(c, j, what="evals") for j in range(c["k"]))
    lo, hi, inv_i = fold_tables(c)
    head = b"".join(x.to_bytes(4, "little") for x in (c["log_n0"], c["lb"], c["round_shift"], 0, 0, 0, 0, 0))
    sx = c["sx"].to_bytes(32, "big") if not c["from_nodes"] else bytes(32)
    parts = [head, _w32(inv_i), sx, b"".join(map(_w32, lo))]
    if hi is not None:
        parts.append(b"".join(map(_w32, hi)))
    parts += [values(c, b) for b in range(c["batch"])]
    if c["from_nodes"]:
        parts += challenges(c)
    return b"".join(parts)


def job_line(c, inp, out):
    arg = {"tree": lambda: FORMS[c["form"]], "packed": lambda: c["k"]}.get(c["op"], lambda: int(c["hi"]) + 2 * int(c["from_nodes"]))()
    return "%s %d %d %d %s %s" % (c["op"], c["n"], c["batch"], arg, inp, out)


# ---- expected bytes ------------------------------------------------------------------------------------------------------------
def tree_hashlib(leaves):
    """merkle_tree.py:36-56 over 32-byte leaves, node 0 as 32 zero bytes (what the kernels store there)"""
    n = len(leaves) // 32
    q = n // 4
    nodes = [b""] * n + [leaves[32 * (i + j * q):32 * (i + j * q) + 32] for i in range(q) for j in range(4)]
    for i in range(n - 1, 0, -1):
        nodes[i] = hashlib.blake2s(nodes[2 * i] + nodes[2 * i + 1]).digest()
    nodes[0] = bytes(32)
    return b"".join(nodes)


def tree_bytes(leaves):
    from oracle import coracle
    return tree_hashlib(leaves) if len(leaves) // 32 <= SMALL_TREE else coracle.merkelize_bytes(leaves)


def expected_tree(c, b, leaves_wire=None, n=None, form=None):
    """the 2n nodes of tree b; the leaf level as 0xa5 bytes when the form does not store it"""
    n = n or c["n"]
    form = form or c["form"]
    leaves = leaves_wire if leaves_wire is not None else values(c, b)
    t = tree_bytes(leaves if form == "raw" else canonical(leaves))
    return t[:32 * n] + SENTINEL * (32 * n) if form == "nostore" else t


def fold_column(c, b):
    """the q = n/4 column values of batch b (canonical ints)"""
    from oracle import coracle, pyoracle
    n = c["n"]
    vals = [int.from_bytes(v, "big") for v in _split(values(c, b))]
    w = pow(root_of(1 << c["log_n0"]), 1 << c["round_shift"], P)
    sx = challenges(c)[b]
    if n <= SMALL_FOLD:
        xs = [pow(w, i, P) for i in range(n)]
        return pyoracle.fri_fold([v % P for v in vals], xs, int.from_bytes(sx, "big") % P, P)
    return coracle.fold(vals, w, sx)


def _split(buf, size=32):
    return [buf[i:i + size] for i in range(0, len(buf), size)]


def column_of(raw):
    """the harness's limb-form column records -> canonical ints"""
    return [int.from_bytes(r, "little") % P for r in _split(raw)]


def expected_packed(c):
    """(nodes [n][32 B], leaves [n][k][32 B]) of merkelize_polynomial_evaluations"""
    from oracle import pyoracle
    evals = [[int.from_bytes(v, "big") for v in _split(values(c, j, what="evals"))] for j in range(c["k"])]
    t = pyoracle.merkelize_polynomial_evaluations(evals)
    n = c["n"]
    return bytes(32) + b"".join(t[1:n]), b"".join(t[n:])


def first_bad_node(got, want, n):
    """(tree b, level, index in level) of the first wrong node of the first wrong tree, looking at the lowest level first (the leaf
    level is level log2(n); a wrong node 0 is reported as level -1)"""
    for b in range(len(want) // (64 * n)):
        g, e = got[64 * n * b:64 * n * (b + 1)], want[64 * n * b:64 * n * (b + 1)]
        if g == e:
            continue
        for lvl in range(log2(n), -1, -1):
            for i in range(1 << lvl, 2 << lvl):
                if g[32 * i:32 * i + 32] != e[32 * i:32 * i + 32]:
                    return b, lvl, i - (1 << lvl)
        return b, -1, 0
    return None


def check(c, out):
    """None if the harness's output of case c is what it must be, else where it first differs"""
    op, n, batch = c["op"], c["n"], c["batch"]
    if op == "tree":
        if len(out) != 64 * n * batch:
            return "%d output bytes, want %d" % (len(out), 64 * n * batch)
        for b in range(batch):
            want = expected_tree(c, b)
            got = out[64 * n * b:64 * n * (b + 1)]
            if got != want:
                _, lvl, i = first_bad_node(got, want, n)
                return "first bad node: tree %d, level %d, index %d" % (b, lvl, i)
        return None
    if op == "packed":
        nodes, leaves = expected_packed(c)
        if len(out) != len(nodes) + len(leaves):
            return "%d output bytes, want %d" % (len(out), len(nodes) + len(leaves))
        if out[:len(nodes)] != nodes:
            _, lvl, i = first_bad_node(out[:len(nodes)] + bytes(32 * n), nodes + bytes(32 * n), n)
            return "first bad node: level %d, index %d" % (lvl, i)
        if out[len(nodes):] != leaves:
            s = next(s for s in range(n * c["k"]) if out[len(nodes) + 32 * s:len(nodes) + 32 * s + 32] != leaves[32 * s:32 * s + 32])
            return "first bad leaf element: slot %d, element %d" % (s // c["k"], s % c["k"])
        return None
    q = n // 4
    want_len = 32 * q * batch + (64 * q * batch if op == "foldtree" else 0)
    if len(out) != want_len:
        return "%d output bytes, want %d" % (len(out), want_len)
    cols = []
    for b in range(batch):
        got = column_of(out[32 * q * b:32 * q * (b + 1)])
        want = fold_column(c, b)
        if got != want:
            i = next(i for i in range(q) if got[i] != want[i])
            return "first bad column row: batch %d, row %d" % (b, i)
        cols.append(want)
    if op == "foldtree":
        nodes = out[32 * q * batch:]
        for b in range(batch):
            want = expected_tree(c, b, b"".join(map(_w32, cols[b])), q, "nostore")
            got = nodes[64 * q * b:64 * q * (b + 1)]
            if got != want:
                _, lvl, i = first_bad_node(got, want, q)
                return "first bad node: tree %d, level %d, index %d" % (b, lvl, i)
    return None


# ---- running -------------------------------------------------------------------------------------------------------------------
def build(workdir, csrc=None):
    exe = os.path.join(str(workdir), "tree_ops")
    csrc = csrc or native_harness.CSRC
    return native_harness.build([HARNESS, os.path.join(csrc, "kernels.hip")], exe, csrc=csrc)


def run(exe, names, workdir, timeout=300):
    """one harness process for the cases `names` -> {name: path of its output}.  The inputs are removed once the process is done;
    each output is meant to be read, checked and removed case by case (read_output), so no more than one is held in memory."""
    import subprocess
    lines, outs = [], {}
    for name in names:
        inp = os.path.join(str(workdir), name + ".in")
        with open(inp, "wb") as fh:
            fh.write(job_input(name))
        outs[name] = os.path.join(str(workdir), name + ".out")
        lines.append(job_line(case(name), inp, outs[name]))
    jf = os.path.join(str(workdir), "tree_jobs")
    with open(jf, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    try:
        p = subprocess.run([exe, jf], capture_output=True, text=True, timeout=timeout)
    finally:
        for name in names:
            os.remove(os.path.join(str(workdir), name + ".in"))
    assert p.returncode == 0, "tree_ops exited %d: %s%s" % (p.returncode, p.stdout, p.stderr)
    return outs


def read_output(path):
    """the bytes of one harness output, the file removed"""
    with open(path, "rb") as fh:
        data = fh.read()
    os.remove(path)
    return data
