#!/usr/bin/env python3
"""Digests of NTTs too long for the pure-Python reference (2^17 dense, 2^19 and 2^21 ... 2^24 points; the reference needs ~25 min and
several GB for 2^24), computed with the C oracle (oracle/oracle.c: the reference's recursive
radix-2 algorithm, fft.py:287-331).  The oracle itself is pinned to the live reference up to 2^20 points by
tests/golden/generate.py + tests/test_coracle.py, so these digests are reference-independent pins for the sizes the
reference cannot reach (BASELINE configs[3]).

    python3 tests/golden/generate_large.py          # writes tests/golden/ntt_large.json  (about 4 min, 4 GB)
    python3 tests/golden/generate_large.py --missing  # keeps the cases already in the file, adds the sizes it lacks
    python3 tests/golden/generate_large.py --fri      # writes tests/golden/fri_large.json (about 3 min, 3 GB): below
    python3 tests/golden/generate_large.py --merkle   # writes tests/golden/merkle_large.json (about 1 min, 2 GB)
    python3 tests/golden/generate_large.py --stark [12 14 16]  # writes / extends tests/golden/stark_large.json: see stark_main
    python3 tests/golden/generate_large.py --fast [-j N]  # the O(n log n) STARK oracle: stark_large.json (2^18, 2^20),
                                                         # stark_units.json, stark_variants.json (about 5 min on 8 cores): fast_main

2^17 is the domain of config 3's commit, whose default plan (9, 8) the reference-generated fixtures reach only through the
sparse first pass (a dense vector of that length: here).  2^19 is the domain of config 5's proofs (plan (9, 10)), 2^21 the first three-pass plan, 2^23 the domain of the metric's
2^20-step FRI commit (the plan with the 256 MiB row table): each of these plan shapes gets its own digest.

Input: x_i = BLAKE2s(seed_le64 || i_le64) mod p with seed 0x5eed; w = 7^((p-1)/n).
Recorded: SHA-256 of the forward transform's wire bytes, of the inverse transform of the INPUT (inv(x), not the round
trip), and the first two output elements of each.

--fri: the FRI commits bench.py times (the metric's second half, "FRI-commit ms for 2^20 trace", and the 2^14 / 2^16-step ones
beside it): coefficients c_i = BLAKE2s(seed_le64 || i_le64) mod p, seed 0xF51, i < steps (a degree < steps polynomial, as
bench.py:extras fills it), 8x extension, w = 7^((p-1)/(8 steps)), maxdeg_plus_1 = steps, exclude_multiples_of = 8, 40 samples:
SHA-256 of the flat proof oracle/oracle.c:fri_rec writes (the reference's commit loop, fri.py:189-266, with its iNTT -> NTT per
round and its Lagrange fold), its length, the first round's root2 and the final layer's first value.  The reference itself cannot
reach these sizes (2^14 steps take it 20 s, 2^20 would take hours); the C oracle is pinned to it on the 2^14-step MiMC commit and
seven smaller ones (tests/golden/fri.json, tests/test_coracle.py)."""
import hashlib
import itertools
import json
import os
import random
import struct
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import coracle  # noqa: E402

P = 2**256 - 2**32 * 351 + 1
SEED = 0x5eed


LOGNS = (17, 19, 21, 22, 23, 24, 25, 26)  # 25, 26: four-pass plans (1 and 2 GiB vectors)
FRI_LOGSTEPS = (14, 16, 18, 20, 22)  # 22: the largest commit the index sampling admits (domain 2^25, utils.py:69)
FRI_SEED = 0xF51


def fri_main():
    out = os.path.join(HERE, "fri_large.json")
    cases = []
    if "--missing" in sys.argv[1:] and os.path.exists(out):
        with open(out) as fh:
            cases = json.load(fh)["cases"]
    have = {c["logsteps"] for c in cases}
    for logsteps in FRI_LOGSTEPS:
        if logsteps in have:
            continue
        steps, ext = 1 << logsteps, 8
        n = steps * ext
        t0 = time.time()
        coeffs = b"".join((int.from_bytes(hashlib.blake2s(struct.pack("<QQ", FRI_SEED, i)).digest(), "big") % P).to_bytes(32, "big")
                          for i in range(steps))
        g2 = pow(7, (P - 1) // n, P)
        flat = coracle.fri_prove_flat(coeffs, g2, steps, ext, 40, n=n)
        case = {"logsteps": logsteps, "steps": steps, "ext": ext, "domain": n, "seed": FRI_SEED, "samples": 40,
                "exclude_multiples_of": ext, "maxdeg_plus_1": steps, "w": "%064x" % g2,
                "coeffs_sha256": hashlib.sha256(coeffs).hexdigest(), "proof_bytes": len(flat),
                "proof_sha256": hashlib.sha256(flat).hexdigest(), "first_root2": flat[:32].hex(),
                "final_layer_first": flat[len(flat) - 32 * 128:len(flat) - 32 * 127].hex(),
                "oracle_seconds": round(time.time() - t0, 1)}
        print(case, flush=True)
        cases.append(case)
    cases.sort(key=lambda c: c["logsteps"])
    with open(out, "w") as fh:
        json.dump({"generator": "tests/golden/generate_large.py --fri (oracle/oracle.c:fri_rec, pinned to the reference by fri.json)",
                   "cases": cases}, fh, indent=1)


STARK_LOGSTEPS = (12, 14, 16)


def stark_main():
    """--stark [LOGSTEPS ...]: whole STARK proofs of config 5's unit 0 (the reference's MiMC formulation, width 2, step polynomials
    [X1, X1 + X2^3], inputs [42, 3], 8x extension, 80 spot checks) at sizes far beyond the reference's own reach, written by the
    COEFFICIENT-FORM prover of oracle/pyoracle.py (the reference's construction, stark.py:27-279: schoolbook polynomial products and
    divisions, quadratic: 40 s for 2^12 steps, 9 min for 2^14, about 2.5 h for 2^16 = config 5's own size), which test_oracle_golden.py
    pins to the live reference on nine smaller cases.  The device prover evaluates the same polynomials on the domain instead; the GPU
    suite compares the flat proof bytes (tests/golden/stark_large.json)."""
    from oracle import pyoracle as po
    out = os.path.join(HERE, "stark_large.json")
    cases = []
    if os.path.exists(out):
        with open(out) as fh:
            cases = json.load(fh)["cases"]
    have = {c["logsteps"] for c in cases}
    want = [int(a) for a in sys.argv[1:] if a.isdigit()] or list(STARK_LOGSTEPS)
    sp = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]
    for logsteps in want:
        if logsteps in have:
            continue
        steps, ext, inputs = 1 << logsteps, 8, [42, 3]
        t0 = time.time()
        w = po.get_computational_trace(inputs, steps, sp)
        proof = po.mk_stark_proof(w, inputs, sp, steps, ext)
        flat = po.stark_flat(proof)
        case = {"logsteps": logsteps, "steps": steps, "ext": ext, "width": 2, "inputs": inputs, "unit": 0,
                "step_polys": [[[list(k), v] for k, v in sorted(d.items())] for d in sp], "samples": 80,
                "outputs": ["%064x" % col[-1] for col in w], "m_root": proof[0].hex(), "l_root": proof[1].hex(),
                "proof_bytes": len(flat), "proof_sha256": hashlib.sha256(flat).hexdigest(), "oracle_seconds": round(time.time() - t0, 1)}
        print(case, flush=True)
        # re-read: several sizes may be generated by concurrent processes
        if os.path.exists(out):
            with open(out) as fh:
                cases = json.load(fh)["cases"]
        cases = [c for c in cases if c["logsteps"] != logsteps] + [case]
        cases.sort(key=lambda c: c["logsteps"])
        with open(out, "w") as fh:
            json.dump({"generator": "tests/golden/generate_large.py --stark (oracle/pyoracle.py:mk_stark_proof, the coefficient-form prover "
                                    "pinned to the reference by stark.json)", "cases": cases}, fh, indent=1)


# ---- --fast: oracle/fastoracle.py:mk_stark_proof_fast (exact, O(n log n); tests/test_stark_oracle.py pins it to the reference's
# proofs and to pyoracle.mk_stark_proof) -----------------------------------------------------------------------------------------
FAST_GENERATOR = "oracle/fastoracle.py:mk_stark_proof_fast"
FAST_LOGSTEPS = (18, 20)          # stark_large.json: config 5's unit 0 beyond 2^16 steps (2^20 is bench.py's stark_prove leg)
UNITS = (1, 63, 64, 127, 128, 255, 256, 511)  # config 5 units on the shard boundaries of 2, 4 and 8 GPUs (512 units)
MIMC_SP = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]
VARIANT_SEED = 0x57A2


def _seeded(seed, i):
    return int.from_bytes(hashlib.blake2s(struct.pack("<QQ", seed, i)).digest(), "big") % P


def variant_inputs(seed, width, unit):
    """Inputs of unit `unit` of a stark_variants.json case (distinct for every unit of a batch)."""
    return [_seeded(seed, unit * width + j) for j in range(width)]


def _variant_polys(width, rng):
    """Random step polynomials of one width: 1-4 terms per dimension, coefficients among 1, 2, p - 1 and random ones; a constant
    term, a term touching every variable (degree = width), every dimension of degree >= 1 somewhere."""
    sp = []
    for j in range(width):
        terms = {}
        ex = [0] * width
        ex[(j + 1) % width] = rng.choice([1, 2, 3])  # dimension j moves with the next one
        terms[tuple(ex)] = rng.choice([1, 2, P - 1, rng.randrange(1, P)])
        for _ in range(rng.randint(0, 2)):
            ex = [0] * width
            for _ in range(rng.randint(1, 3)):
                ex[rng.randrange(width)] += 1
            terms[tuple(ex)] = rng.choice([1, 2, P - 1, rng.randrange(1, P)])
        sp.append(terms)
    sp[0][(0,) * width] = P - 1                      # a constant term
    sp[-1][(1,) * width] = rng.choice([1, P - 1])    # a term touching every variable
    return sp


def variant_cases():
    """The shapes of stark_variants.json.  rows = steps * ext / 4 * batch decides which kernel instance stark.hip launches
    (STARK_WIDE_THREADS, SHK_STARK_SPLIT_LOG there; tests/test_gpu_parity.py derives the regimes from the source and asserts that
    every cell has a case): for every width a narrow (rows <= 2^16), a middle (2^17 < rows < 2^19) and a WIDE (rows >= 2^19) batch;
    the band 2^16 < rows <= 2^17 for widths 1, 2 and 5; width 2 on both sides of each threshold."""
    rng = random.Random(VARIANT_SEED)
    cases = []

    def add(name, width, sp, steps, ext, batch):
        cases.append({"name": name, "width": width, "steps": steps, "ext": ext, "batch": batch, "seed": VARIANT_SEED + len(cases),
                      "step_polys": [[[list(k), v] for k, v in sorted(d.items())] for d in sp]})

    polys = {w: _variant_polys(w, rng) for w in range(1, 10)}
    exts = {1: (4, 8, 8), 2: (8, 4, 16), 3: (16, 8, 8), 4: (4, 16, 32), 5: (8, 8, 16), 6: (16, 8, 32), 7: (8, 16, 16),
            8: (16, 8, 32), 9: (16, 32, 16)}
    for w in range(1, 10):
        sp = polys[w]
        deg = max(sum(k) for d in sp for k in d)
        en, em, ew = exts[w]
        assert all(deg * (s - 1) + 1 < s * e for s, e in ((1 << 9, en), (1 << 11, em), (1 << 12, ew))), (w, deg)
        add("w%d_narrow" % w, w, sp, 1 << 9, en, 3)
        r = (1 << 11) * em // 4
        add("w%d_middle" % w, w, sp, 1 << 11, em, (1 << 17) // r + 5 + w)
        r = (1 << 12) * ew // 4
        add("w%d_wide" % w, w, sp, 1 << 12, ew, (1 << 19) // r + 1)
    # the lincomb band 2^16 < rows <= 2^17 (quotients narrow, lincomb middle) for the W = 1, W = 2 and generic instances
    for w in (1, 2, 5):
        add("w%d_band" % w, w, polys[w], 1 << 10, 8, 45)
    # width 2 on both sides of each threshold: one proof is 2^13 rows
    for tag, b in (("rows_2^16", 8), ("rows_2^17", 16), ("rows_2^17+1p", 17), ("rows_2^19-1p", 63), ("rows_2^19", 64)):
        add("w2_" + tag, 2, polys[2], 1 << 12, 8, b)
    # the library's 256-term limit: width 9, the first 256 monomials of degree <= 4 in turn, round robin over the dimensions
    mons = sorted({tuple(sum(1 for v in pick if v == i) for i in range(9)) for pick in itertools.combinations_with_replacement(
        range(10), 4)})  # variable 9 stands for "none": degrees 0 ... 4
    big = [{} for _ in range(9)]
    for t, ex in enumerate(mons[:256]):
        big[t % 9][ex] = rng.choice([1, P - 1, rng.randrange(1, P)])
    add("w9_256_terms", 9, big, 1 << 8, 16, 5)
    return cases


def _prove_one(job):
    """Worker: one proof by the fast oracle -> (sha256 hex, flat bytes length, m_root, l_root, outputs, seconds)."""
    from oracle import fastoracle as fo
    from oracle import pyoracle as po
    inputs, steps, ext, sp = job
    t0 = time.time()
    w = po.get_computational_trace(inputs, steps, sp)
    proof = fo.mk_stark_proof_fast(w, inputs, sp, steps, ext)
    flat = po.stark_flat(proof)
    return (hashlib.sha256(flat).hexdigest(), len(flat), proof[0].hex(), proof[1].hex(), ["%064x" % col[-1] for col in w],
            time.time() - t0)


def _dump(path, generator, cases):
    with open(path, "w") as fh:
        json.dump({"generator": generator, "cases": cases}, fh, indent=1)


def fast_main():
    """--fast [-j N]: the STARK fixtures the O(n log n) oracle writes.  It first reproduces the committed 2^12 / 2^14 / 2^16 cases of
    stark_large.json (written by the quadratic pyoracle prover) and stops unless every byte agrees; then it proves, in N worker
    processes, config 5's unit 0 at 2^18 and 2^20 steps (stark_large.json), units UNITS at 2^16 steps (stark_units.json) and the kernel
    variant matrix of variant_cases() (stark_variants.json).  Apart from oracle_seconds a re-run rewrites all three files byte for byte."""
    from multiprocessing import Pool
    from oracle import fastoracle as fo
    from oracle import pyoracle as po
    nproc = int(sys.argv[sys.argv.index("-j") + 1]) if "-j" in sys.argv else (os.cpu_count() or 1)
    large_path = os.path.join(HERE, "stark_large.json")
    with open(large_path) as fh:
        large = json.load(fh)
    old = [c for c in large["cases"] if c["logsteps"] not in FAST_LOGSTEPS]
    for c in old:
        w = po.get_computational_trace(c["inputs"], c["steps"], MIMC_SP)
        flat = po.stark_flat(fo.mk_stark_proof_fast(w, c["inputs"], MIMC_SP, c["steps"], c["ext"]))
        assert hashlib.sha256(flat).hexdigest() == c["proof_sha256"] and len(flat) == c["proof_bytes"], c["logsteps"]
        print("reproduced stark_large.json 2^%d" % c["logsteps"], flush=True)
        c.setdefault("generator", "oracle/pyoracle.py:mk_stark_proof")
    variants = variant_cases()
    jobs = [([42, 3], 1 << ls, 8, MIMC_SP) for ls in FAST_LOGSTEPS]
    jobs += [([42, 3 + j], 1 << 16, 8, MIMC_SP) for j in UNITS]
    for v in variants:
        sp = [{tuple(k): c for k, c in d} for d in v["step_polys"]]
        jobs += [(variant_inputs(v["seed"], v["width"], u), v["steps"], v["ext"], sp) for u in range(v["batch"])]
    with Pool(nproc) as pool:
        res = pool.map(_prove_one, jobs, chunksize=1)
    it = iter(res)
    new = []
    for ls in FAST_LOGSTEPS:
        sha, nb, m, l, outs, sec = next(it)
        new.append({"logsteps": ls, "steps": 1 << ls, "ext": 8, "width": 2, "inputs": [42, 3], "unit": 0,
                    "step_polys": [[[list(k), v] for k, v in sorted(d.items())] for d in MIMC_SP], "samples": 80, "outputs": outs,
                    "m_root": m, "l_root": l, "proof_bytes": nb, "proof_sha256": sha, "generator": FAST_GENERATOR,
                    "oracle_seconds": round(sec, 1)})
    large["cases"] = sorted(old + new, key=lambda c: c["logsteps"])
    units = []
    for j in UNITS:
        sha, nb, m, l, outs, sec = next(it)
        units.append({"unit": j, "steps": 1 << 16, "ext": 8, "width": 2, "inputs": [42, 3 + j], "samples": 80, "outputs": outs,
                      "m_root": m, "l_root": l, "proof_bytes": nb, "proof_sha256": sha, "generator": FAST_GENERATOR,
                      "oracle_seconds": round(sec, 1)})
    for v in variants:
        got = [next(it) for _ in range(v["batch"])]
        v["proof_bytes"] = got[0][1]
        v["unit_sha256"] = [g[0] for g in got]
        v["generator"] = FAST_GENERATOR
        v["oracle_seconds"] = round(sum(g[5] for g in got), 1)
    _dump(large_path, "tests/golden/generate_large.py --stark (oracle/pyoracle.py:mk_stark_proof, the coefficient-form prover "
                      "pinned to the reference by stark.json) and --fast (oracle/fastoracle.py:mk_stark_proof_fast, pinned to it)", large["cases"])
    _dump(os.path.join(HERE, "stark_units.json"), "tests/golden/generate_large.py --fast (%s): config 5 units (inputs [42, 3 + unit], "
          "step polynomials [X1, X1 + X2^3]) at 2^16 steps" % FAST_GENERATOR, units)
    _dump(os.path.join(HERE, "stark_variants.json"), "tests/golden/generate_large.py --fast (%s): generate_large.variant_cases(); "
          "unit u of a case has inputs generate_large.variant_inputs(seed, width, u) and the witness "
          "pyoracle.get_computational_trace(inputs, steps, step_polys)" % FAST_GENERATOR, variants)


def merkle_main():
    """--merkle: the Merkle commitment bench.py times (2^24 leaves x_i = BLAKE2s(seed_le64 || i_le64) mod p, seed 7, and the 2^20-leaf
    one of its --quick mode) hashed by oracle/oracle.c:or_merkelize (merkle_tree.py:36-56 with permute4): the root, three interior
    nodes and the SHA-256 of the whole 2n x 32-byte node array (slot 0 = zeros, as sh_merkelize writes it)."""
    out = os.path.join(HERE, "merkle_large.json")
    cases = []
    if "--missing" in sys.argv[1:] and os.path.exists(out):
        with open(out) as fh:
            cases = json.load(fh)["cases"]
    have = {c["logn"] for c in cases}
    for logn in (20, 24, 26):  # 26: 2 GiB of leaves, 4 GiB of nodes (about 2 min)
        if logn in have:
            continue
        n = 1 << logn
        t0 = time.time()
        leaves = b"".join((int.from_bytes(hashlib.blake2s(struct.pack("<QQ", 7, i)).digest(), "big") % P).to_bytes(32, "big")
                          for i in range(n))
        nodes = coracle.merkelize_bytes(leaves)
        case = {"logn": logn, "n": n, "seed": 7, "root": nodes[32:64].hex(), "node_2": nodes[64:96].hex(), "node_n_minus_1": nodes[32 * (n - 1):32 * n].hex(),
                "node_n": nodes[32 * n:32 * n + 32].hex(), "nodes_sha256": hashlib.sha256(bytes(32) + nodes[32:]).hexdigest(),
                "oracle_seconds": round(time.time() - t0, 1)}
        print(case, flush=True)
        cases.append(case)
        del leaves, nodes
    cases.sort(key=lambda c: c["logn"])
    with open(out, "w") as fh:
        json.dump({"generator": "tests/golden/generate_large.py --merkle (oracle/oracle.c:or_merkelize, pinned to the reference by merkle.json)",
                   "cases": cases}, fh, indent=1)


def main():
    if "--merkle" in sys.argv[1:]:
        return merkle_main()
    if "--fri" in sys.argv[1:]:
        return fri_main()
    if "--fast" in sys.argv[1:]:
        return fast_main()
    if "--stark" in sys.argv[1:]:
        return stark_main()
    out = os.path.join(HERE, "ntt_large.json")
    cases = []
    if "--missing" in sys.argv[1:] and os.path.exists(out):
        with open(out) as fh:
            cases = json.load(fh)["cases"]
    have = {c["logn"] for c in cases}
    for logn in LOGNS:
        if logn in have:
            continue
        n = 1 << logn
        t0 = time.time()
        raw = b"".join(hashlib.blake2s(struct.pack("<QQ", SEED, i)).digest() for i in range(n))
        w = pow(7, (P - 1) // n, P)
        fwd = coracle.fft_bytes(raw, n, w)
        case = {"logn": logn, "n": n, "seed": SEED, "w": "%064x" % w,
                "sha_fwd": hashlib.sha256(fwd).hexdigest(), "fwd_head": fwd[:64].hex(),
                "fwd_tail": fwd[-32:].hex()}
        del fwd
        inv = coracle.fft_bytes(raw, n, w, inverse=True)
        case.update({"sha_inv": hashlib.sha256(inv).hexdigest(), "inv_head": inv[:64].hex()})
        del inv, raw
        case["oracle_seconds"] = round(time.time() - t0, 1)
        print(case, flush=True)
        cases.append(case)
    cases.sort(key=lambda c: c["logn"])
    with open(out, "w") as fh:
        json.dump({"generator": "tests/golden/generate_large.py (oracle/oracle.c, pinned to the reference <= 2^20)",
                   "cases": cases}, fh, indent=1)


if __name__ == "__main__":
    main()
