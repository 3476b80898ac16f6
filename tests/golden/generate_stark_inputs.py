#!/usr/bin/env python3
"""Writes tests/golden/stark_inputs.json: the per-unit SHA-256 of the oracle's proofs (oracle/fastoracle.py, the O(n log n)
coefficient-form prover) for the cases of tests/stark_input_cases.py that are too many units for the oracle at test time -- one width-2
and one width-3 batch per quotient / lincomb regime (narrow, middle, wide), and the valid unit of the 2^12-step witness-check case.
    PYTHONDONTWRITEBYTECODE=1 python3 tests/golden/generate_stark_inputs.py
Uses oracle/ and tests/ only (build liboracle.so first: make -C oracle).  About 1 s of oracle time per 2^15-point unit; the cases run
in parallel processes.  The fixture holds hashes only; the systems, shapes and inputs are code (stark_input_cases.py).
tests/test_stark_inputs_host.py regenerates the small entries and one unit of every other one."""
import concurrent.futures
import json
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import stark_input_cases as sc  # noqa: E402


def _regime(index):
    case = sc.regime_cases()[index]
    t0 = time.time()
    shas = sc.regime_entry(case)
    return dict(name=case["name"], width=case["width"], steps=case["steps"], ext=case["ext"], batch=case["batch"], seed=case["seed"],
                unit_sha256=shas, oracle_seconds=round(time.time() - t0, 1))


def main():
    n = len(sc.regime_cases())
    with concurrent.futures.ProcessPoolExecutor(max_workers=min(n, os.cpu_count() or 1)) as pool:
        regimes = list(pool.map(_regime, range(n)))
    c = sc.SIZE_CASE
    out = dict(generator="tests/golden/generate_stark_inputs.py (oracle/fastoracle.mk_stark_proof_fast)", regimes=regimes,
               size_case=dict(name=c["name"], width=c["width"], steps=c["steps"], ext=c["ext"], unit1_sha256=sc.size_entry()))
    with open(sc.FIXTURE, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    for r in regimes:
        print("%-10s %3d units  %6.1f s" % (r["name"], r["batch"], r["oracle_seconds"]))


if __name__ == "__main__":
    main()
