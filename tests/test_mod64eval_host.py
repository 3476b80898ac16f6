"""sh_mod64_poly_eval's CPU half: tests/native/mod64eval_host.cpp (hipcc) runs the templated drivers of starks_amd/csrc/poly_items.cuh
(pa_eval, pa_eval_direct, pa_eval_tree) over uint64_t with the element steps of mod64eval_items.cuh -- the code api_mod64poly.hip runs
-- on a host Ops: the direct path's lanes, workgroup sums and second pass, the tree path's chunks, root product, descent and combine,
against exact Python-int Horner over ten moduli below 2^64 and against tests/golden/mod_poly_eval.json.  Also: the shapes at the edges
of a point group, unreduced words, the direct shape and the path rule against their stated formulas, the driver's restated host checks,
the library's symbols, header and prototypes, and the Python form without a context.  One more build of the same driver under ASan +
UBSan runs three cases as its own program.  CPU only.
What this half does NOT run: the kernels of mod64eval.hip and the host checks of api_mod64poly.hip: tests/test_gpu_mod64eval.py."""
import ctypes
import os
import random
import subprocess

import pytest

from conftest import ROOT, load_golden
import mod64eval_cases as mc
import modpoly_cases as mp
from mod64eval_cases import FIELDS, IDS, evaluate, unwords, words
from mod64poly_cases import FIXTURE_MODULI

CSRC = os.path.join(ROOT, "starks_amd", "csrc")
G = [c for c in mp.resolved(load_golden("mod_poly_eval.json")) if c["p"] < 2**64]
HIPCC = ["/opt/rocm/bin/hipcc", "-O2", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC]
SRC = os.path.join(ROOT, "tests", "native", "mod64eval_host.cpp")
MODULI = list(FIELDS)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("m6e") / "mod64eval_host")
    subprocess.check_call(HIPCC + [SRC, "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _call(driver, d, p, path, coefs, xs, batch=1, root=None, env=None):
    w, k = root or mc.two_adic_root(p)
    (d / "coefs").write_bytes(words(p, coefs))
    (d / "xs").write_bytes(words(p, xs))
    return subprocess.run([driver, path, str(d), str(p), str(w), str(k), str(batch)], capture_output=True, text=True, timeout=600, env=env)


def _run(driver, d, p, path, coefs, xs, batch=1, root=None):
    """one driver run: the output words and (direct?, a, b, c); checks the transforms the Ops saw against the formula"""
    out = _call(driver, d, p, path, coefs, xs, batch, root)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    seen, formula, transforms, direct, a, b, c = (int(v) for v in out.stdout.split())
    n, m = len(coefs) // batch, len(xs)
    assert formula == mc.max_transform(n, m), (n, m, formula)
    if path != "default":
        assert direct == (path == "direct")
    if direct:
        assert seen == 0 and transforms == 0, "the direct path runs no transform"
        assert (a, b, c) == mc.direct_shape(n, m, batch, mc.M6E_GROUP) or not (n and m)
    elif n and m:
        assert seen == formula, (n, m, seen, formula)
    return unwords((d / "out").read_bytes()), (direct, a, b, c)


def _paths(p, n, m):
    return ["direct"] + (["tree"] if mc.admits(p, n, m) else [])


# ---- exact against Python ints -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", MODULI, ids=IDS.get)
def test_eval_host(driver, tmp_path, p):
    """every pair of PAIRS on the direct path; on the tree path exactly the pairs whose transform 2 pow2(m) the field admits -- counted,
    so nothing is skipped silently; for 2-adicity >= 12 that is every pair"""
    admitted = [(n, m) for n, m in mc.PAIRS if 2 * mp.pow2_at_least(m) <= 1 << min(FIELDS[p], 26)]
    directs = trees = 0
    for n, m in mc.PAIRS:
        coefs, xs = mc.word_inputs(p, n, m)
        want = evaluate(p, coefs, xs)
        got, _ = _run(driver, tmp_path, p, "direct", coefs, xs)
        assert got == want, (n, m, "direct")
        directs += 1
        if (n, m) in admitted:
            got, _ = _run(driver, tmp_path, p, "tree", coefs, xs)
            assert got == want, (n, m, "tree")
            trees += 1
        elif n and m:  # the restated check refuses a forced tree there
            assert _call(driver, tmp_path, p, "tree", coefs, xs).returncode == 7
    assert directs == len(mc.PAIRS) and trees == len(admitted)
    if FIELDS[p] >= 12:
        assert trees == len(mc.PAIRS)


@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.P63, 97], ids=IDS.get)
def test_eval_host_batch_and_wide(driver, tmp_path, p):
    """BATCHES on both paths, and WIDE: long polynomials, W > 1 workgroups per point group, added by the second pass"""
    for n, m, batch in mc.BATCHES:
        coefs, xs = mc.word_inputs(p, n, m, batch)
        for path in _paths(p, n, m):
            got, _ = _run(driver, tmp_path, p, path, coefs, xs, batch)
            assert got == evaluate(p, coefs, xs, batch), (n, m, batch, path)
    for n, m in mc.WIDE:
        coefs, xs = mc.word_inputs(p, n, m)
        got, shape = _run(driver, tmp_path, p, "direct", coefs, xs)
        assert shape[1] > 1 and shape[3] == (mc.M6E_GROUP if m >= mc.M6E_GROUP else 1)
        assert got == evaluate(p, coefs, xs), (n, m)


@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.BIG], ids=IDS.get)
def test_sum_shared_among_lanes(driver, tmp_path, p):
    """W = 128 workgroups for one point and W = 64 for two: the driver adds them as m6e_sum_kernel does, min(W, 64) lanes per output,
    so m6e_sum_item is walked with a step below W (two sums per lane) and with step = W"""
    for n, m in ((1 << 21, 1), (1 << 20, 2)):
        rnd = random.Random(n + m)
        coefs, xs = [rnd.getrandbits(64) for _ in range(n)], [rnd.getrandbits(64) for _ in range(m)]
        got, shape = _run(driver, tmp_path, p, "direct", coefs, xs)
        assert shape[1] == (128 if m == 1 else 64) and shape[3] == 1
        assert got == evaluate(p, coefs, xs), (n, m)


@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.P63, mc.BIG, 97], ids=IDS.get)
def test_group_boundaries(driver, tmp_path, p):
    """m = G - 1 (one point per lane), G, G + 1 and 2 G + 1 (a last group of one point) at n = 255, 256, 257"""
    G_ = mc.M6E_GROUP
    assert mc.GROUP_MS == [G_ - 1, G_, G_ + 1, 2 * G_ + 1] and len(mc.GROUP_SHAPES) == 12
    for n, m in mc.GROUP_SHAPES:
        coefs, xs = mc.word_inputs(p, n, m)
        for path in _paths(p, n, m):
            got, shape = _run(driver, tmp_path, p, path, coefs, xs)
            assert got == evaluate(p, coefs, xs), (n, m, path)
            if path == "direct":
                assert shape[3] == (1 if m < mc.M6E_GROUP else mc.M6E_GROUP)


@pytest.mark.parametrize("p", [mc.GOLDILOCKS, mc.P63, mc.BABYBEAR, 65537, 97], ids=IDS.get)
def test_unreduced_words(driver, tmp_path, p):
    """coefficients and points in [p, 2^64) -- p itself, the largest multiple of p and 2^64 - 1 among them -- give the outputs of their
    residues on both paths"""
    rnd = random.Random(p % 991)
    n, m = 300, 8
    coefs = [rnd.randrange(p) for _ in range(n)]
    xs = [rnd.randrange(p) for _ in range(m)]
    for v in (coefs, xs):  # every other residue below 2^64 - p, so that an unreduced word of it exists above 2^63 too
        v[::2] = [x % (2**64 - p) for x in v[::2]]
    coefs[4], coefs[7], xs[2], xs[5] = 0, 0, 0, 0
    coefs[0] = xs[0] = (2**64 - 1) % p  # lifts to 2^64 - 1
    up_c, up_x = mc.lifted(p, coefs, rnd), mc.lifted(p, xs, rnd)
    up_c[4], up_c[7], up_x[2], up_x[5] = p, p * ((2**64 - 1) // p), p, p * ((2**64 - 1) // p)
    assert up_c[0] == up_x[0] == 2**64 - 1 and sum(v >= p for v in up_c + up_x) >= 8
    assert [v % p for v in up_c] == coefs and [v % p for v in up_x] == xs
    want = evaluate(p, coefs, xs)
    for path in _paths(p, n, m):
        for c, x in ((coefs, xs), (up_c, up_x), (up_c, xs), (coefs, up_x)):
            got, _ = _run(driver, tmp_path, p, path, c, x)
            assert got == want, path


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", FIXTURE_MODULI, ids=IDS.get)
def test_fixture_host(driver, tmp_path, p):
    """the recorded cases below 2^64, operands reduced mod p, both paths where the tree fits: the outputs match the recorded ones, so
    the words are pinned to the reference"""
    assert len(G) == 54 and {c["p"] for c in G} == {mc.GOLDILOCKS, 65537, 97}
    mine = [c for c in G if c["p"] == p]
    assert len(mine) == 18
    trees = 0
    for c in mine:
        coefs, xs = [v % p for v in c["a"]], [v % p for v in c["xs"]]
        for path in _paths(p, len(coefs), len(xs)):
            got, _ = _run(driver, tmp_path, p, path, coefs, xs)
            assert mp.matches(c["out"], got), (c["name"], path)
            trees += path == "tree"
    assert trees == sum(mc.admits(p, len(c["a"]), len(c["xs"])) for c in mine) and trees >= (18 if p != 97 else 1)


# ---- shape, rule and the restated checks ---------------------------------------------------------------------------------------------
def test_shape_and_rule(driver, tmp_path):
    lines = subprocess.check_output([driver, "consts"], text=True).splitlines()
    assert int(lines[0]) == mc.M6E_GROUP
    assert tuple(float(v) for v in lines[1].split()) == mc.M6E_COST
    shapes = [(n, m, b) for n in (0, 1, 255, 256, 1 << 14, (1 << 15) - 1, 1 << 15, (1 << 15) + 5, 1 << 20, 1 << 24)
              for m in [1] + mc.GROUP_MS + [64, 1000, 1 << 12] for b in (1, 3, 64)]
    f = tmp_path / "shapes"
    f.write_text("".join("%d %d %d\n" % s for s in shapes))
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([driver, "shape", str(f)], text=True).splitlines()]
    assert len(rows) == len(shapes)
    for s, got in zip(shapes, rows):
        assert got == mc.direct_shape(s[0], s[1], s[2], mc.M6E_GROUP), s
    assert any(r[0] > 1 for r in rows) and {r[2] for r in rows} == {1, mc.M6E_GROUP}
    grid = [(1 << a, 1 << b, batch) for a in range(0, 26, 2) for b in range(0, 21, 2) for batch in (1, 4)]
    grid += [(1 << 15, 1 << 13, 1), (1 << 16, 1 << 13, 1), (1 << 24, 1, 1), (1 << 20, 1 << 20, 1)]
    f.write_text("".join("%d %d %d\n" % s for s in grid))
    rows = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([driver, "prefer", str(f), "26"], text=True).splitlines()]
    assert len(rows) == len(grid)
    for s, (rule, chosen) in zip(grid, rows):
        assert rule == chosen == mc.direct_preferred(mc.M6E_COST, *s), s
    assert {r[0] for r in rows} == {0, 1}
    # a call whose tree transform exceeds the root's order is direct, whatever the cost rule says
    rows5 = [tuple(int(v) for v in line.split()) for line in subprocess.check_output([driver, "prefer", str(f), "5"], text=True).splitlines()]
    for (n, m, _b), (rule, chosen) in zip(grid, rows5):
        assert chosen == (1 if mc.max_transform(1, m) > 32 else rule), (n, m)
    assert any(rule == 0 and chosen == 1 for rule, chosen in rows5)


def test_default_path_and_small_two_adicity(driver, tmp_path):
    """default = the rule's choice; over 3, 97 and 2^64 - 59 with root = (1, 0) every call is direct and exact, a forced tree refused"""
    for p in (3, 97, mc.BIG):
        coefs, xs = mc.word_inputs(p, 300, 129)
        got, shape = _run(driver, tmp_path, p, "default", coefs, xs, root=(1, 0))
        assert shape[0] == 1 and got == evaluate(p, coefs, xs)
        assert _call(driver, tmp_path, p, "tree", coefs, xs, root=(1, 0)).returncode == 7
    p = mc.GOLDILOCKS
    coefs, xs = mc.word_inputs(p, 1000, 3)
    got, shape = _run(driver, tmp_path, p, "default", coefs, xs)
    assert shape[0] == int(mc.direct_preferred(mc.M6E_COST, 1000, 3, 1)) and got == evaluate(p, coefs, xs)


def test_driver_checks(driver, tmp_path):
    """the driver's restatement of the host checks, each with its own exit code"""
    p = 97
    w, k = mc.two_adic_root(p)
    coefs, xs = list(range(1, 21)), [3, 4, 5]
    for bad in (96, 0, 1):
        assert _call(driver, tmp_path, bad, "direct", coefs, xs, root=(0, 0)).returncode == 4
    assert _call(driver, tmp_path, p, "direct", coefs, xs, root=(w, k - 1)).returncode == 5          # order 32 given as 16
    assert _call(driver, tmp_path, p, "direct", coefs, xs, root=(pow(w, 2, p), k)).returncode == 5   # order 16 given as 32
    assert _call(driver, tmp_path, p, "direct", coefs, xs, root=(w + p, k)).returncode == 5          # at or above p
    assert _call(driver, tmp_path, p, "direct", coefs, xs, root=(1, 29)).returncode == 6
    assert _call(driver, tmp_path, p, "direct", coefs, xs, batch=0).returncode == 3
    assert _call(driver, tmp_path, p, "direct", coefs, xs, batch=3).returncode == 3
    assert _call(driver, tmp_path, p, "tree", coefs, list(range(17))).returncode == 7                # needs 64 > 32
    assert _call(driver, tmp_path, p, "tree", coefs, list(range(16))).returncode == 0
    assert _call(driver, tmp_path, p, "direct", coefs, xs, root=(1, 0)).returncode == 0


# ---- under ASan + UBSan, as its own program -------------------------------------------------------------------------------------------
def test_driver_sanitized(tmp_path):
    exe = str(tmp_path / "mod64eval_host_san")
    subprocess.check_call(HIPCC + ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", SRC,
                                   "-o", exe], stderr=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for p, path, (n, m, batch) in [(97, "tree", (1000, 3, 1)), (mc.P63, "direct", ((1 << 15) + 5, 5, 1)), (mc.GOLDILOCKS, "tree", (300, 33, 2))]:
        coefs, xs = mc.word_inputs(p, n, m, batch)
        out = _call(exe, tmp_path, p, path, coefs, xs, batch, env=env)
        assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
        assert unwords((tmp_path / "out").read_bytes()) == evaluate(p, coefs, xs, batch)
        if path == "direct":
            assert int(out.stdout.split()[4]) > 1  # W > 1


# ---- the library and the Python form -------------------------------------------------------------------------------------------------
def test_library_exports_and_header():
    for src in ("mod64eval.hip", "api_mod64poly.hip"):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-c", os.path.join(CSRC, src), "-o",
                               os.devnull], stderr=subprocess.DEVNULL, timeout=900)
    from starks_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "starkhip.h")).read()
    for name in ("sh_mod64_poly_eval", "sh_dev_mod64_poly_eval"):
        assert name in _lib.exported_symbols() and getattr(L, name).restype is ctypes.c_int
        assert "int %s(" % name in header
        assert len(L._sig[name][1]) == 10 and L._sig[name][1][1] is ctypes.c_uint64  # the modulus is a word
    assert "mod64eval.hip" in open(os.path.join(CSRC, "Makefile")).read()
    still_open = [line for line in header.splitlines() if "STILL OPEN" in line]
    assert still_open and all("sh_mod_poly_eval" not in line and "evaluation" not in line for line in still_open)
    assert all("sh_mod64_poly_eval" not in line for line in still_open)
    assert L.sh_mod_poly_max_transform(4, 1000, 3) == mc.max_transform(1000, 3) == 8  # op 4 states these entries' transform too


def test_python_form_without_a_device(monkeypatch):
    from starks_amd import _lib, polynomial
    monkeypatch.setattr(_lib, "ctx", lambda: pytest.fail("must not ask for a context"))
    for empty in ([], b"", memoryview(bytearray()).cast("Q")):
        out = polynomial.mod64_eval_words(97, [1, 2, 3], empty)
        assert isinstance(out, memoryview) and out.format == "Q" and len(out) == 0
    assert len(polynomial.mod64_eval_words(97, [], [], batch=3)) == 0
    with pytest.raises(ValueError):
        polynomial.mod64_eval_words(97, [1, 2, 3], [1], batch=2)
    with pytest.raises(ValueError):
        polynomial.mod64_eval_words(97, [1, 2, 3], [1], batch=0)
    with pytest.raises(ValueError):
        polynomial.mod64_eval_words(97, [1, 2, 3], [], batch=2)  # the coefficient check comes before the empty result
    with pytest.raises(ValueError):
        polynomial.mod64_eval_words(97, b"\0" * 7, [1])
