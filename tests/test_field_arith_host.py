"""Every primitive of starks_amd/csrc/fp256.cuh on the host (tests/native/fp256_ops.hip --host: the header's portable C paths, which
build every twiddle table and run the host verifiers) against exact integers: the edge set, every named rare carry and borrow branch,
and about 10^5 random operands per op (tests/field_cases.py).  Results must equal the models' bytes, the non-canonical lazily reduced
representatives included.  CPU only; tests/test_gpu_field_arith.py runs the same cases on the device."""
import os
import subprocess

import pytest

import field_cases as fc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return fc.build_harness(tmp_path_factory.mktemp("fp256_ops") / "fp256_ops")


def test_branch_vectors_take_their_branches(capsys):
    """Each rare continuation has at least two vectors, each shown to take it (and only the branches it names) by emulating the limbs;
    the images of the vectors for neg, the raw products and the two reductions take the same branches."""
    rows = []
    for name, (op, flags, vecs) in fc.BRANCHES.items():
        assert len(vecs) >= 2, name
        for v in vecs:
            assert fc.taken(op, v) == flags, (name, [hex(x) for x in v])
        rows.append("%-36s %-5s %d vectors: %s" % (name, op, len(vecs), ", ".join("(" + ", ".join(hex(x) for x in v[:2]) + ")" for v in vecs[:2])))
    for op in ("neg", "mulwide", "mul2wide", "redwide", "red13"):
        images = fc.rare_operands(op)
        assert images
        for name, vecs in images.items():
            assert all(fc.taken(op, v) == fc.BRANCHES[name][1] for v in vecs), (op, name)
    with capsys.disabled():
        print("\nbranch -> vectors\n" + "\n".join(rows))


def test_models_are_the_residues():
    """The exact representatives the tests expect are the residues the ops promise (checked per case in field_cases.expected); a few
    fixed points as a cross-check of the models themselves."""
    P, M, C = fc.P, fc.M, fc.C
    assert fc.m_add(M - 1, M - 1) == M - 2 - 2 * P + M   # two folds: 2^257 - 2 - 2p
    assert fc.m_sub(0, M - 1) == P + 1 - M + P            # two borrows
    # fp_inv(p) returns p itself: a lazily reduced 0, like fp_mul(p, p)
    assert fc.m_inv(0) == 0 and fc.m_inv(P) == P and fc.canon(fc.m_inv(2)) == (P + 1) // 2
    assert fc.m_div4(M - 1) * 4 % P == (M - 1) % P and fc.m_div4(0) == 0
    for t in ((1 << 512) - 1, (1 << 385) - 1, M * C):
        assert fc.fold(t) < M and fc.fold(t) % P == t % P


@pytest.mark.parametrize("op", sorted(fc.OPS))
def test_host_paths_against_exact_integers(harness, tmp_path, op):
    """--host on the edge set and random operands, and on the device layouts (every branch vector among ordinary operands): bytes equal
    the model's."""
    got = fc.run_jobs(harness, "host", [(op, part, 0, 0, part) for part in ("main", "layout")], tmp_path)
    for part in ("main", "layout"):
        assert got[part] == fc.case_set(op, part)[2], fc.mismatches(op, part, got[part])


def test_harness_refuses_bad_jobs(harness, tmp_path):
    """A record file of the wrong size, an unknown op, or a launch with fewer threads than elements is refused before anything runs
    (the launch check comes before any device call, so it runs here too)."""
    (tmp_path / "in").write_bytes(bytes(64 * 3 - 4))
    for mode, line in (("host", "add 3 0 0 %s/in %s/out"), ("host", "add 2 0 0 %s/in %s/out"), ("host", "nope 3 0 0 %s/in %s/out"),
                       ("device", "add 6 1 5 %s/in %s/out"), ("device", "add 6 1 0 %s/in %s/out"), ("device", "add 6 1 2048 %s/in %s/out")):
        (tmp_path / "jobs").write_text(line % (tmp_path, tmp_path) + "\n")
        p = subprocess.run([harness, "--" + mode, str(tmp_path / "jobs")], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (line, p.stdout, p.stderr)
        assert not os.path.exists(tmp_path / "out")
