"""The Merkle tree and FRI fold harness (tests/native/tree_ops.hip) and its case grid (tests/tree_cases.py), on the CPU: the harness
cross-compiles with kernels.hip alone, refuses every malformed job before it touches the GPU, the grid reaches every kernel form
kernels.hip dispatches to, and the expected bytes agree with each other where two references overlap.  CPU only."""
import os
import random
import subprocess

import pytest

import tree_cases as tc


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return tc.build(tmp_path_factory.mktemp("tree_ops"))


def test_harness_cross_compiles(exe):
    assert os.path.getsize(exe) > 0


def test_grid_covers_every_cell():
    """every required form has a case, with the thresholds read from kernels.hip; printed cell by cell"""
    th = tc.thresholds()
    by_cell = {}
    for c in tc.cases():
        for cell in tc.cells_of(c, th):
            by_cell.setdefault(cell, []).append(c["name"])
    for cell in sorted(tc.required_cells(th), key=str):
        print("covered" if cell in by_cell else "MISSING", cell, by_cell.get(cell, []))
    assert tc.required_cells(th) <= set(by_cell)


def test_cases_place_edges_and_distinct_values():
    """every quarter of a permute4 row holds each edge value somewhere, the first and last rows of the first workgroup included, and
    the values of a tree are otherwise distinct"""
    c = tc.case("limb_4k_x256")
    q = c["n"] // 4
    for b in (0, 1):
        vals = [int.from_bytes(v, "big") for v in tc._split(tc.values(c, b))]
        for j in range(4):
            assert {vals[r + j * q] for r in tc._edge_rows(q)} == set(tc.EDGES)
        assert {vals[j * q + r] for j in range(4) for r in (0, 255)} <= set(tc.EDGES)
        rest = [v for i, v in enumerate(vals) if i % q not in tc._edge_rows(q)]
        assert len(set(rest)) == len(rest)
        assert any(v >= tc.P for v in rest)  # the random unreduced ones
        assert tc.canonical(tc.values(c, b)) == b"".join(tc._w32(v % tc.P) for v in vals)


def test_expectations_agree():
    """hashlib trees equal the C oracle's (every size the grid hashes with hashlib, and beyond), and pyoracle's Lagrange fold equals
    the C fold, with unreduced values and challenges and a later round's generator"""
    from oracle import coracle, pyoracle
    rng = random.Random(7)
    for logn in range(2, 9):
        leaves = rng.randbytes(32 << logn)
        assert tc.tree_hashlib(leaves) == coracle.merkelize_bytes(leaves)
    for name in ("fold_256_x8_nodes_hi", "fold_64_x64_hi", "fold_4_x3", "foldtree_64_x4_nodes"):
        c = tc.case(name)
        w = pow(tc.root_of(1 << c["log_n0"]), 1 << c["round_shift"], tc.P)
        for b in range(min(c["batch"], 4)):
            vals = [int.from_bytes(v, "big") for v in tc._split(tc.values(c, b))]
            sx = tc.challenges(c)[b]
            xs = [pow(w, i, tc.P) for i in range(c["n"])]
            assert tc.fold_column(c, b) == coracle.fold(vals, w, sx)
            assert pyoracle.fri_fold([v % tc.P for v in vals], xs, int.from_bytes(sx, "big") % tc.P, tc.P) == coracle.fold(vals, w, sx)
    # the tables: lo * hi covers every power of w0, and inv_i is the inverse of the 4th root of unity
    c = tc.case("fold_256_x8_nodes_hi")
    lo, hi, inv_i = tc.fold_tables(c)
    w0 = tc.root_of(1 << c["log_n0"])
    for e in (0, 1, 63, 64, 1000, (1 << c["log_n0"]) - 1):
        assert lo[e & ((1 << c["lb"]) - 1)] * hi[e >> c["lb"]] % tc.P == pow(w0, e, tc.P)
    assert inv_i * pow(w0, 1 << (c["log_n0"] - 2), tc.P) % tc.P == 1


def test_packed_expectation_layout():
    """the packed expectation is the reference's tree: node 0 zero, nodes 1..n-1, then the permuted k-element leaves"""
    from oracle import pyoracle
    c = tc.case("packed_64_k3")
    nodes, leaves = tc.expected_packed(c)
    evals = [tc._split(tc.values(c, j, what="evals")) for j in range(3)]
    assert len(nodes) == 32 * 64 and nodes[:32] == bytes(32) and len(leaves) == 32 * 64 * 3
    assert leaves[:96] == evals[0][0] + evals[1][0] + evals[2][0]
    assert leaves[96:192] == evals[0][16] + evals[1][16] + evals[2][16]  # slot 1 = leaf n/4
    assert nodes[32:64] == pyoracle.blake(nodes[64:128])


def _refused(exe, tmp_path, line, data):
    (tmp_path / "in").write_bytes(data)
    (tmp_path / "jobs").write_text(line.replace("IN", str(tmp_path / "in")).replace("OUT", str(tmp_path / "out")) + "\n")
    p = subprocess.run([exe, str(tmp_path / "jobs")], capture_output=True, text=True, timeout=60)
    return p.returncode == 2 and not os.path.exists(tmp_path / "out"), p.stdout + p.stderr


def test_harness_refuses_bad_jobs(exe, tmp_path):
    """n not a power of two or below 4, batch 0, k 0, a raw tree without its leaf level, packed with a batch, foldtree with n/4 < 4,
    a wrong input size, fold arguments that index outside their tables, an unknown op or a malformed line: status 2, no output --
    even when a valid job comes first"""
    ok_tree = "tree 16 1 1 IN OUT"
    fold16 = tc.case("foldtree_16_x8")

    def fold_in(c, **kw):
        c = dict(c, **kw)
        head = b"".join(x.to_bytes(4, "little") for x in (c["log_n0"], c["lb"], c["round_shift"], 0, 0, 0, 0, 0))
        lo = 1 << c["lb"]
        hi = (1 << (c["log_n0"] - c["lb"])) if c["hi"] else 0
        return head + bytes(64 + 32 * (lo + hi) + 32 * c["n"] * c["batch"] + (32 * c["batch"] if c["from_nodes"] else 0))

    v = lambda n: bytes(32 * n)  # noqa: E731
    cases = [("tree 12 1 1 IN OUT", v(12)), ("tree 2 1 1 IN OUT", v(2)), ("tree 0 1 1 IN OUT", v(0)), ("tree 16 0 1 IN OUT", v(0)),
             ("tree 16 1 2 IN OUT", v(16)), ("tree 16 1 5 IN OUT", v(16)), ("tree 16 2 1 IN OUT", v(16)), ("tree 16 1 1 IN OUT", v(17)),
             ("tree 16 65536 1 IN OUT", v(16 * 65536)),
             ("packed 16 1 0 IN OUT", v(0)), ("packed 16 2 1 IN OUT", v(32)), ("packed 16 1 2 IN OUT", v(16)),
             ("packed 6 1 1 IN OUT", v(6)), ("foldtree 8 1 0 IN OUT", fold_in(fold16, n=8, batch=1, log_n0=3, lb=3, round_shift=0)),
             ("fold 16 8 0 IN OUT", fold_in(fold16)[:-32]), ("fold 16 8 0 IN OUT", fold_in(fold16, round_shift=1)),
             ("fold 16 8 0 IN OUT", fold_in(fold16, lb=2)), ("fold 16 8 4 IN OUT", fold_in(fold16)),
             ("fold 16 8 0 IN OUT", fold_in(fold16, lb=5)), ("fold 16 8 0 IN OUT", b"\x04\x00"),
             ("fold 16 8 1 IN OUT", fold_in(fold16, lb=3)), ("fold 16 8 3 IN OUT", fold_in(fold16, hi=True, lb=2)),
             ("merkle 16 1 1 IN OUT", v(16)), ("tree 16 1 IN OUT", v(16)),
             (ok_tree + "\ntree 12 1 1 IN OUT", v(16))]
    assert tc.job_line(fold16, "IN", "OUT") == "foldtree 16 8 0 IN OUT"
    for line, data in cases:
        ok, msg = _refused(exe, tmp_path, line, data)
        assert ok, (line, len(data), msg)
