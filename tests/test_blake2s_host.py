"""Every form of starks_amd/csrc/blake2s.cuh on the host (tests/native/blake2s_ops.hip --host: b2_compress_cpp behind both template
forms, the host verifiers' path, and vb_hash_two) against hashlib.blake2s and the C oracle, on tests/hash_cases.py's messages; the
sampler cases against the oracle's get_pseudorandom_indices; and a cross-compile of every device build tests/test_gpu_blake2s.py runs:
the defaults, -DB2_NO_ASM, -DB2Q_NO_ASM, both, and one build per generator form of the single-lane asm rounds.  CPU only."""
import os
import subprocess

import pytest

import hash_cases as hc


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    d = tmp_path_factory.mktemp("blake2s_ops")
    return d, hc.build_all(d)


@pytest.mark.parametrize("op", hc.HOST_OPS)
def test_host_paths_against_hashlib(builds, tmp_path, op):
    """--host on every part of the op: both halves of each record (the <true> and <false> forms, which are the C++ rounds on the host)
    equal hashlib.blake2s of the message"""
    exe = builds[1]["default"]
    got = hc.run_jobs(exe, "host", [(op, part, 0, 0, part) for part in hc.PARTS[op]], tmp_path, timeout=300)
    for part in hc.PARTS[op]:
        assert got[part] == hc.case_set(op, part)[2], hc.mismatches(op, part, got[part])


def test_oracle_agrees_with_hashlib():
    """the expected digests are also the C oracle's (oracle/oracle.c), for every message length the cases use; and the expected
    index sets are also the oracle's get_pseudorandom_indices"""
    from oracle import coracle
    msgs = hc.special_blocks()[:40] + [bytes(range(ln)) for ln in range(65)] + [bytes(64 * k) for k in hc.CHAIN_KS]
    msgs += [os.urandom(2 * ln) for ln in hc.VB_LENS]
    for m in msgs:
        assert coracle.blake2s(m) == hc.blake(m), m.hex()
    from starks_amd.utils import get_pseudorandom_indices
    for i, (modulus, count, exclude) in enumerate(hc.sample_args()):
        entropy = bytes([i & 255]) * 32
        assert coracle.pseudorandom_indices(entropy, modulus, count, exclude) == get_pseudorandom_indices(entropy, modulus, count, exclude)


def test_sampler_cases_cover_the_grid():
    """every count, modulus and exclude of the grid occurs, only arguments the library takes, and the main batch leaves dead quads in
    its last block; the expected records pad past `count` with the 0xa5 the kernel must leave alone"""
    args = hc.sample_args()
    assert {c for _, c, _ in args} == set(hc.SAMPLE_COUNTS) and {e for _, _, e in args} == set(hc.SAMPLE_EXCLUDES)
    assert {m for m, _, _ in args} == set(hc.sample_moduli())
    assert all(m < 1 << 24 and hc.real_modulus(m, e) >= 1 for m, _, e in args)
    for part in hc.PARTS["sample"]:
        n, _, want = hc.case_set("sample", part)
        assert n % 16
        assert len(want) == n * 4 * hc.SAMPLE_WORDS


def test_every_build_cross_compiles(builds):
    """all nine device builds compile for gfx950; each generator form's include differs from the committed one, and no two builds
    are the same binary"""
    d, exes = builds
    assert set(exes) == set(hc.BUILDS)
    committed = open(os.path.join(hc.native_harness.CSRC, "blake2s_asm.inc"), "rb").read()
    for name, (_, gen) in hc.BUILDS.items():
        assert os.path.getsize(exes[name]) > 0
        if gen is not None:
            assert open(os.path.join(str(d), "blake2s_asm_%s.inc" % name), "rb").read() != committed, name
    assert len({open(e, "rb").read() for e in exes.values()}) == len(exes)


def test_harness_refuses_bad_jobs(builds, tmp_path):
    """a record outside what its op takes (a short len of 65, a chain of 0 or 256 blocks, a vb_hash_two len not a multiple of 32,
    sampler arguments the library refuses or that differ inside a block), a record file of the wrong size, a device-only op on the
    host, or a launch with too few threads or the wrong sampler block is refused before anything runs"""
    exe = builds[1]["default"]

    def rec(op, head):
        ib = hc.OPS[op][0]
        skip = {"sample": 32, "quad": 64}.get(op, 0)   # the arguments after the entropy / the message
        return (bytes(skip) + hc._w(*head) + bytes(ib))[:ib]

    cases = [("host", "short", [rec("short", [65])]), ("host", "chain", [rec("chain", [0])]), ("host", "chain", [rec("chain", [256])]),
             ("host", "vbtwo", [rec("vbtwo", [48])]), ("host", "vbtwo", [rec("vbtwo", [896])]), ("host", "quad", [rec("quad", [])]),
             ("device", "sample", [rec("sample", [8, 4, 1])]), ("device", "sample", [rec("sample", [1 << 24, 4, 0])]),
             ("device", "sample", [rec("sample", [1, 4, 2])]), ("device", "sample", [rec("sample", [8, 256, 0])]),
             ("device", "sample", [rec("sample", [8, 4, 0]), rec("sample", [8, 5, 0])]),
             ("device", "quad", [rec("quad", [65, 1])])]
    for mode, op, recs in cases:
        (tmp_path / "in").write_bytes(b"".join(recs))
        (tmp_path / "jobs").write_text("%s %d 1 64 %s/in %s/out\n" % (op, len(recs), tmp_path, tmp_path))
        p = subprocess.run([exe, "--" + mode, str(tmp_path / "jobs")], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (mode, op, recs[0][:48].hex(), p.stdout, p.stderr)
        assert not os.path.exists(tmp_path / "out")
    pair = bytes(64 * 3)
    (tmp_path / "in").write_bytes(pair)
    for mode, line in (("host", "pair 4 0 0 %s/in %s/out"), ("device", "pair 3 1 2 %s/in %s/out"),
                       ("device", "quad 1 1 2 %s/in %s/out"), ("device", "sample 1 1 128 %s/in %s/out"),
                       ("device", "pair 3 1 2048 %s/in %s/out")):
        (tmp_path / "jobs").write_text(line % (tmp_path, tmp_path) + "\n")
        p = subprocess.run([exe, "--" + mode, str(tmp_path / "jobs")], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (line, p.stdout, p.stderr)
        assert not os.path.exists(tmp_path / "out")
