"""The run-time-modulus field arithmetic on the host (tests/native/modarith_ops.hip --host): every function of starks_amd/csrc/fpm.cuh
and starks_amd/csrc/fp64m.cuh and the small functions built on them (fpm_pow_limbs, mf_half, me_below_p, me_coef, mp_mulp, mp_sub,
mp_inv1; f64_from_limbs, m6_half, m6_wire_words, m6e_coef, m6p_mulp, m6p_sub, m6p_inv1) against exact integers, for every modulus of
tests/modarith_cases.py: 13 below 2^256 and 11 below 2^64.  Per op and modulus: the edge set crossed with itself, at least 8 vectors
of every operand class the headers' comments name (asserted when the set is built), 20 000 random operands (2 000 for pow, 500 for
pow_limbs and inv1), and the device layouts.  Results must equal the models' bytes.  This is where the models and the classifiers
are proven; tests/test_gpu_modarith.py runs the same cases on the device.  CPU only; about 70 s on one core, the harness build
included."""
import os
import subprocess

import pytest

import modarith_cases as ma

PAIRS = [(f, name) for f in sorted(ma.MODULI) for name in sorted(ma.MODULI[f])]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return ma.build_harness(tmp_path_factory.mktemp("modarith_ops") / "modarith_ops")


def test_moduli_and_models():
    """the moduli the issue names are here, inv1 runs exactly on the primes, and a few fixed points of the models and classifiers"""
    big, word = ma.MODULI["fpm"], ma.MODULI["f64"]
    assert len(big) == 13 and {2**256 - 189, 3, 2**255 + 95, 2**256 - 351 * 2**32 + 1, 4369} <= set(big.values())
    assert len(word) == 11 and {0xffffffffffe40001, 2**64 - 59, 2**64 - 1, 3, 2**64 - 2**32 + 1} <= set(word.values())
    assert not ma.is_prime(4369) and not ma.is_prime(2**64 - 1) and ma.is_prime(2**256 - 189) and ma.is_prime(2**64 - 59)
    assert "inv1" not in ma.ops_of("fpm", "composite") and "inv1" not in ma.ops_of("f64", "all_ones") and "inv1" in ma.ops_of("f64", "f3")
    p = 2**64 - 59
    assert ma.mul_classes("f64", p, 0, 5) == ({"lo_zero", "not_taken", "zero"}, 0)
    assert ma.mul_classes("f64", p, p, 5) == ({"taken", "sum_eq_p", "zero"}, 0)
    assert ma.mul_classes("fpm", ma.MODULI["fpm"]["mimc"], 2**256 - 1, ma.MODULI["fpm"]["mimc"] - 1)[0] >= {"top", "taken"}
    assert ma.half_classes("f64", p, p - 2) == {"odd_carry"} and ma.half_classes("f64", 17, 3) == {"odd"}
    assert ma.add_classes("f64", p, p - 1, p - 1) == {"carry"} and ma.add_classes("fpm", 17, 8, 9) == {"eq_p"}


@pytest.mark.parametrize("family,name", PAIRS)
def test_every_reachable_class_has_its_vectors(family, name):
    """at least MIN_CLASS vectors of each class that can occur over this modulus, each shown by the classifier to be of its class;
    the classes `reachable` rules out did not occur among the candidates (asserted inside class_vectors)"""
    p = ma.MODULI[family][name]
    for op in sorted(ma.CLASSIFY):
        found = ma.class_vectors(family, name, op)
        assert set(found) == ma.reachable(family, p, op)
        for c, vecs in found.items():
            assert len(vecs) >= ma.MIN_CLASS, (family, name, op, c)
            assert all(c in ma.classes_of(family, name, op, v) for v in vecs), (family, name, op, c)
    R = 1 << ma.BITS[family]
    mul = ma.class_vectors(family, name, "mul")
    if family == "f64":
        assert ("carry" in mul) == ("wrap" in mul) == (2 * p > R) and "lo_zero" in mul
    else:
        assert ("top" in mul) == (2 * p > R) and ("ninth" in mul) == (p > 1 << 128)


@pytest.mark.parametrize("family,name", PAIRS)
def test_host_against_exact_integers(harness, tmp_path, family, name):
    """--host on every op and part of one modulus: bytes equal the model's"""
    ops = ma.ops_of(family, name)
    got = ma.run_jobs(harness, "host", [ma.job(family, name, op, part, 0, 0, "%s.%s" % (op, part)) for op in ops for part in ("main", "layout")],
                      tmp_path)
    bad = []   # every failing op is reported, so that a broken carry shows under the op and class that name it
    for op in ops:
        for part in ("main", "layout"):
            r = got["%s.%s" % (op, part)]
            if r != ma.case_set(family, name, op, part)[2]:
                bad.append(ma.mismatches(family, name, op, part, r, limit=3))
    assert not bad, "\n".join(bad)


def test_harness_refuses_bad_jobs(harness, tmp_path):
    """A record file of the wrong size, an unknown op, an even modulus, or a launch with fewer threads than elements is refused before
    anything runs (the launch check comes before any device call, so it runs here too)."""
    (tmp_path / "in").write_bytes((17).to_bytes(8, "little") + bytes(16 * 3 - 4))
    (tmp_path / "even").write_bytes((18).to_bytes(8, "little") + bytes(16 * 3))
    (tmp_path / "wide").write_bytes((17).to_bytes(32, "little") + bytes(64 * 3 + 4))
    for mode, line in (("host", "f64_add 3 0 0 %s/in %s/out"), ("host", "f64_add 2 0 0 %s/in %s/out"), ("host", "nope 3 0 0 %s/in %s/out"),
                       ("host", "f64_add 3 0 0 %s/even %s/out"), ("host", "fpm_add 3 0 0 %s/wide %s/out"),
                       ("device", "f64_add 6 1 5 %s/in %s/out"), ("device", "f64_add 6 1 0 %s/in %s/out"),
                       ("device", "fpm_add 6 1 2048 %s/in %s/out")):
        (tmp_path / "jobs").write_text(line % (tmp_path, tmp_path) + "\n")
        p = subprocess.run([harness, "--" + mode, str(tmp_path / "jobs")], capture_output=True, text=True, timeout=60)
        assert p.returncode == 2, (line, p.stdout, p.stderr)
        assert not os.path.exists(tmp_path / "out")
