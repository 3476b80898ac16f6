"""The batch verifiers' per-item checks (starks_amd/csrc/verify_items.cuh) run on the host in the kernels' decomposition
(tests/native/verify_batch_host.cpp, hipcc): index sets, Merkle branches, FRI rows, spot checks, the final layer, then the OR per
proof.  On the committed STARK and FRI proofs, on single-bit flips in every region of their layout and on wrong public values, every
decision equals sh_stark_verify / sh_fri_verify.  CPU only."""
import ctypes
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT, load_golden
from oracle import pyoracle as po
from verify_batch_layout import flips, fri_regions, stark_regions

P = po.MIMC_P


def _wire(vals):
    return b"".join((int(v) % P).to_bytes(32, "big") for v in vals)


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vbh") / "verify_batch_host")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "verify_batch_host.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    return exe


def _run(driver, d, args):
    out = subprocess.run([driver] + [str(a) for a in args[:1]] + [str(d)] + [str(a) for a in args[1:]], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.split("\n")


STARK_CASES = [c for c in load_golden("stark.json") if os.path.exists(os.path.join(GOLDEN, "stark_%s.flat.bin" % c["name"]))]


@pytest.mark.parametrize("c", STARK_CASES, ids=lambda c: c["name"])
def test_stark_items_decide_as_the_host_verifier(c, driver, tmp_path):
    from starks_amd import _lib, stark
    flat = open(os.path.join(GOLDEN, "stark_%s.flat.bin" % c["name"]), "rb").read()
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    steps, ext, width = c["steps"], c["ext"], c["width"]
    coefs, exps, counts, _ = stark.pack_step_polys([_Poly(d) for d in sp], width)
    degree = max(sum(exps[t * width:(t + 1) * width]) for t in range(len(coefs) // 32))  # every listed term counts (verify.hip)
    regions, end = stark_regions(steps, ext, width, degree, 80)
    assert end == len(flat)
    outs = [col[-1] for col in po.get_computational_trace(c["inputs"], steps, sp)]
    inb, outb = _wire(c["inputs"]), _wire(outs)
    cases = [("untouched", flat, inb, outb)]
    cases += [(name, bad, inb, outb) for name, bad in flips(flat, regions, 5, c["flat_len"])]
    wrong_out = list(outs)
    wrong_out[-1] += 1
    wrong_in = [c["inputs"][0] + 1] + list(c["inputs"][1:])
    cases += [("wrong_output", flat, inb, _wire(wrong_out)), ("wrong_input", flat, _wire(wrong_in), outb),
              ("unreduced_input", flat, (int(c["inputs"][0]) + P).to_bytes(32, "big") + inb[32:], outb)]
    for name, data in (("proofs", b"".join(x[1] for x in cases)), ("inputs", b"".join(x[2] for x in cases)),
                       ("outputs", b"".join(x[3] for x in cases)), ("coefs", coefs), ("exps", exps), ("counts", bytes(counts))):
        (tmp_path / name).write_bytes(data)
    got = _run(driver, tmp_path, ["stark", steps, ext, width, 80, len(cases)])
    L = _lib.lib()
    want = [L.sh_stark_verify(p, len(p), i, o, steps, ext, width, coefs, exps, counts, 80) for _, p, i, o in cases]
    assert want[0] == 0 and want[-1] == 0  # (x + p encodes x)
    assert want.count(-9) >= len(cases) - 3
    for (name, _, _, _), g, w in zip(cases, got, want):
        assert int(g) == w, (name, g, w)


FRI_CASES = [r for r in load_golden("fri.json") if os.path.exists(os.path.join(GOLDEN, r["name"] + ".flat.bin"))]


@pytest.mark.parametrize("rec", FRI_CASES, ids=lambda r: r["name"])
def test_fri_items_decide_as_the_host_verifier(rec, driver, tmp_path):
    from starks_amd import _lib
    flat = open(os.path.join(GOLDEN, rec["name"] + ".flat.bin"), "rb").read()
    w = int(rec["w"], 16)
    n = _lib.order_of_root(w)
    md, ex, sm = rec["maxdeg_plus_1"], rec["exclude_multiples_of"], rec["samples"]
    regions, end = fri_regions(n, md, sm)
    assert end == len(flat)
    root = bytes.fromhex(rec["eval_root"])
    cases = [("untouched", flat, root)] + [(name, bad, root) for name, bad in flips(flat, regions, 8, rec["flat_len"])]
    cases.append(("wrong_root", flat, bytes(32)))
    (tmp_path / "proofs").write_bytes(b"".join(x[1] for x in cases))
    (tmp_path / "roots").write_bytes(b"".join(x[2] for x in cases))
    (tmp_path / "root").write_bytes(w.to_bytes(32, "big"))
    got = _run(driver, tmp_path, ["fri", n, md, ex, sm, len(cases)])
    L = _lib.lib()
    want = [L.sh_fri_verify(p, len(p), r, n, w.to_bytes(32, "big"), md, ex, sm) for _, p, r in cases]
    assert want[0] == 0 and want.count(-9) >= len(cases) - 1
    for (name, _, _), g, v in zip(cases, got, want):
        assert int(g) == v, (name, g, v)


def test_shape_verdicts_match_the_host_verifier(driver, tmp_path):
    """The plan's verdict on a shape is the host verifier's on an honest proof of it: the final layer cap aside."""
    (tmp_path / "proofs").write_bytes(b"")
    (tmp_path / "roots").write_bytes(b"")
    (tmp_path / "root").write_bytes(pow(7, (P - 1) // 1024, P).to_bytes(32, "big"))
    assert _run(driver, tmp_path, ["fri", 1000, 256, 0, 40, 0])[0] == "shape -1"        # n not a power of two
    assert _run(driver, tmp_path, ["fri", 2048, 256, 0, 40, 0])[0] == "shape -2"        # root of order 1024
    assert _run(driver, tmp_path, ["fri", 1024, 256, 1, 40, 0])[0] == "shape -1"        # exclude 1: the sampling divides by zero
    assert _run(driver, tmp_path, ["fri", 1024, 1 << 20, 0, 40, 0])[0] == "shape -1"    # the rounds run out of domain
    assert _run(driver, tmp_path, ["fri", 1024, 16, 0, 40, 0]) == [""]                 # a final layer of 2^10 points: at the cap
    (tmp_path / "root").write_bytes(pow(7, (P - 1) // 2048, P).to_bytes(32, "big"))
    assert _run(driver, tmp_path, ["fri", 2048, 16, 0, 40, 0])[0] == "shape -6"         # 2^11 points: over it
    for name, data in (("coefs", bytes(32)), ("exps", bytes([1])), ("counts", bytes(ctypes.c_uint32(1))), ("inputs", b""), ("outputs", b"")):
        (tmp_path / name).write_bytes(data)
    assert _run(driver, tmp_path, ["stark", 24, 8, 1, 80, 0])[0] == "shape -1"         # steps not a power of two
    assert _run(driver, tmp_path, ["stark", 1 << 21, 8, 1, 80, 0])[0] == "shape -1"    # ext * steps >= 2^24


def test_algebraic_checks_alone_reject(driver, tmp_path):
    """Proofs whose every Merkle branch and root verifies, so that only one algebraic check can reject them: the final layer's degree
    bound (fri_deg512 verified against maxdeg_plus_1 = 300: the same layout), a FRI row (the first column folded at special_x + 1, the
    rest of the proof honest for that column) and the transition constraint (mimc_w2_s8 against step polynomials with one coefficient
    off by 1: the same shape).  The host verifier rejects each; the items decide the same, and accept the honest counterparts."""
    from starks_amd import _lib, stark
    from verify_batch_layout import wrong_fold_fri
    L = _lib.lib()

    def fri_case(d, flat, root, n, w, md, ex, sm, want):
        d.mkdir()
        (d / "proofs").write_bytes(flat)
        (d / "roots").write_bytes(root)
        (d / "root").write_bytes(w.to_bytes(32, "big"))
        assert L.sh_fri_verify(flat, len(flat), root, n, w.to_bytes(32, "big"), md, ex, sm) == want
        assert int(_run(driver, d, ["fri", n, md, ex, sm, 1])[0]) == want

    rec = [r for r in load_golden("fri.json") if r["name"] == "fri_deg512"][0]
    flat = open(os.path.join(GOLDEN, "fri_deg512.flat.bin"), "rb").read()
    w = int(rec["w"], 16)
    n = _lib.order_of_root(w)
    root = bytes.fromhex(rec["eval_root"])
    assert int(L.sh_fri_proof_len(n, 300, 40)) == len(flat)
    fri_case(tmp_path / "deg_ok", flat, root, n, w, 512, 0, 40, 0)
    fri_case(tmp_path / "deg_300", flat, root, n, w, 300, 0, 40, -9)
    n2 = 1024
    w2 = pow(7, (P - 1) // n2, P)
    coeffs = [pow(3, i, P) for i in range(200)]
    for nudge, want in ((0, 0), (1, -9)):
        wf, wroot = wrong_fold_fri(coeffs, n2, w2, 256, 8, 40, nudge)
        fri_case(tmp_path / ("fold_%d" % nudge), wf, wroot, n2, w2, 256, 8, 40, want)
    c = [c for c in STARK_CASES if c["name"] == "mimc_w2_s8"][0]
    flat = open(os.path.join(GOLDEN, "stark_mimc_w2_s8.flat.bin"), "rb").read()
    sp = [{tuple(k): v for k, v in d} for d in c["step_polys"]]
    outs = [col[-1] for col in po.get_computational_trace(c["inputs"], c["steps"], sp)]
    other = [dict(d) for d in sp]
    k0 = sorted(other[-1])[-1]
    other[-1][k0] = (other[-1][k0] + 1) % P
    for name, polys, want in (("steps_ok", sp, 0), ("steps_off", other, -9)):
        coefs, exps, counts, _ = stark.pack_step_polys([_Poly(d) for d in polys], 2)
        d = tmp_path / name
        d.mkdir()
        for fname, data in (("proofs", flat), ("inputs", _wire(c["inputs"])), ("outputs", _wire(outs)), ("coefs", coefs), ("exps", exps),
                            ("counts", bytes(counts))):
            (d / fname).write_bytes(data)
        assert L.sh_stark_verify(flat, len(flat), _wire(c["inputs"]), _wire(outs), 8, 8, 2, coefs, exps, counts, 80) == want
        assert int(_run(driver, d, ["stark", 8, 8, 2, 80, 1])[0]) == want
