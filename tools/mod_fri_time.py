#!/usr/bin/env python3
"""Time of the FRI commit over other moduli (GPU box): device time of sh_dev_mod_fri_prove on seeded limb-form coefficients at
n = 2^14, 2^16, 2^20 and 8 x 2^16 (maxdeg_plus_1 = n / 8, exclude_multiples_of = 8, n coefficients per polynomial) over BN254,
BLS12-381, Goldilocks and the MiMC prime, and in the same run the forward sh_dev_mod_ntt alone, sh_dev_fri_prove (the tuned MiMC
commit) of the same shape and the tuned forward sh_dev_ntt alone.  HIP events around REPS calls after a warm-up of every shape
(tables, workspaces, code objects), the smallest of ROUNDS windows, the paths alternating round by round.
`commit_less_transform_ratio` = (generic commit - generic transform) / (MiMC commit - MiMC transform): what the trees, the fold, the
sampling and the gather cost over p beside the tuned ones.  The hashing is the same work, so it should sit near 1; it is reported,
not gated.  Prints one JSON line and writes it to argv[1] (default profiles/r13_mod_fri.json).  `--trace` instead runs the 2^20
BN254 and tuned commits twice each in a child process under `rocprofv3 --kernel-trace --stats` and copies its kernel statistics to
profiles/r13_mod_fri_kernel_stats.csv."""
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import _lib  # noqa: E402

MIMC_P = 2**256 - 2**32 * 351 + 1
# name -> (modulus, 2-adicity, a base whose (p - 1) / 2^adicity-th power has full order): tests/modntt_cases.py
FIELDS = {
    "bn254": (21888242871839275222246405745257275088548364400416034343698204186575808495617, 28, 5),
    "bls12_381": (0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001, 32, 5),
    "goldilocks": (2**64 - 2**32 + 1, 32, 7),
    "mimc": (MIMC_P, 32, 3),
}
SHAPES = [(14, 1), (16, 1), (20, 1), (16, 8)]
ROUNDS = 5
EXCLUDE, SAMPLES = 8, 40


def reps_for(lg, batch):
    return max(4, min(32, (1 << 22) // (batch << lg)))


def ck(rc, where):
    _lib.check(rc, where)


def root(name, n):
    p, v, base = FIELDS[name]
    return pow(pow(base, (p - 1) >> v, p), (1 << v) // n, p)


def b32(x):
    return int(x).to_bytes(32, "big")


def window(L, ctx, fn, reps):
    ck(L.sh_timer_start(ctx), "timer")
    for _ in range(reps):
        fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value / reps


def calls(L, ctx, name, x, y, proof, n, batch):
    """(commit, forward transform) over FIELDS[name]; name None: the tuned MiMC pair"""
    md = n // 8
    if name is None:
        w = b32(root("mimc", n))
        return (lambda: ck(L.sh_dev_fri_prove(ctx, x, n, w, md, EXCLUDE, SAMPLES, batch, proof), "sh_dev_fri_prove"),
                lambda: ck(L.sh_dev_ntt(ctx, x, y, n, batch, w, 0), "sh_dev_ntt"))
    p, w = b32(FIELDS[name][0]), b32(root(name, n))
    return (lambda: ck(L.sh_dev_mod_fri_prove(ctx, p, x, n, n, w, md, EXCLUDE, SAMPLES, batch, proof), "sh_dev_mod_fri_prove"),
            lambda: ck(L.sh_dev_mod_ntt(ctx, p, x, y, n, batch, w, 0), "sh_dev_mod_ntt"))


def buffers(L, ctx, count, proof_bytes):
    x, y, proof = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, 32 * count, ctypes.byref(x)), "alloc")
    ck(L.sh_dev_alloc(ctx, 32 * count, ctypes.byref(y)), "alloc")
    ck(L.sh_dev_alloc(ctx, proof_bytes, ctypes.byref(proof)), "alloc")
    ck(L.sh_dev_fill_seeded(ctx, x, count, 1), "fill")
    return x, y, proof


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    big = max(batch << lg for lg, batch in SHAPES)
    plen = max(batch * L.sh_fri_proof_len(1 << lg, (1 << lg) // 8, SAMPLES) for lg, batch in SHAPES)
    x, y, proof = buffers(L, ctx, big, plen)
    res = {"tool": "tools/mod_fri_time.py", "rounds": ROUNDS, "maxdeg_plus_1": "n / 8", "exclude_multiples_of": EXCLUDE, "samples": SAMPLES,
           "stat": "min over rounds of (HIP-event ms of `reps` calls) / reps, after a warm-up; paths alternate per round; "
                   "n coefficients per polynomial on every path",
           "shapes": {}}
    for lg, batch in SHAPES:
        n, reps = 1 << lg, reps_for(lg, batch)
        fns = {}
        fns["mimc_tuned_commit"], fns["mimc_tuned_ntt"] = calls(L, ctx, None, x, y, proof, n, batch)
        for name in FIELDS:
            fns[name + "_commit"], fns[name + "_ntt"] = calls(L, ctx, name, x, y, proof, n, batch)
        for fn in fns.values():  # warm-up
            fn()
        ck(L.sh_sync(ctx), "sync")
        best = {}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t = window(L, ctx, fn, reps)
                best[k] = min(best.get(k, t), t)
        tuned = best["mimc_tuned_commit"] - best["mimc_tuned_ntt"]
        row = {"reps": reps, "ms": best,
               "commit_less_transform_ms": dict({k: best[k + "_commit"] - best[k + "_ntt"] for k in FIELDS}, mimc_tuned=tuned),
               "commit_less_transform_ratio": {k: (best[k + "_commit"] - best[k + "_ntt"]) / tuned for k in FIELDS},
               "commit_ratio_to_tuned": {k: best[k + "_commit"] / best["mimc_tuned_commit"] for k in FIELDS}}
        res["shapes"]["%dx2^%d" % (batch, lg)] = row
    ck(L.sh_sync(ctx), "sync")
    for p in (x, y, proof):
        L.sh_dev_free(ctx, p)
    ck(L.sh_ctx_trim(ctx), "trim")
    return res


def once():
    L, ctx = _lib.lib(), _lib.ctx()
    n = 1 << 20
    x, y, proof = buffers(L, ctx, n, L.sh_fri_proof_len(n, n // 8, SAMPLES))
    for name in ("bn254", None):
        commit, _ = calls(L, ctx, name, x, y, proof, n, 1)
        commit()
        commit()
    ck(L.sh_sync(ctx), "sync")


def trace():
    out_dir = tempfile.mkdtemp(prefix="mod_fri_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod_fri", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r13_mod_fri_kernel_stats.csv")
        shutil.copyfile(stats[0], dst)
        print("wrote", dst)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    if "--trace" in sys.argv:
        return trace()
    if "--once" in sys.argv:
        return once()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r13_mod_fri.json")
    line = json.dumps(measure())
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
