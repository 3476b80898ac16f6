#!/usr/bin/env python3
"""Time of the generic transform (GPU box): device time of sh_dev_mod_ntt forward + inverse on seeded limb-form vectors at 2^16, 2^20,
2^24 and 8 x 2^20 over BN254, BLS12-381, the MiMC prime, Goldilocks and BabyBear, and in the same run sh_dev_ntt (the tuned MiMC
transform) at the same shapes as yardstick.  HIP events around REPS forward + inverse pairs after a warm-up of every shape (tables,
workspaces, code objects), the smallest of ROUNDS windows, the two paths alternating round by round.  `ratio_to_tuned` is the
generic time over the tuned time of the same shape: the condition of the path is BN254 at most 4 x at 2^20 and 2^24.
Prints one JSON line and writes it to argv[1] (default profiles/r11_mod_ntt.json).  `--trace` instead runs each 2^24 BN254 and tuned
transform once in a child process under `rocprofv3 --kernel-trace --stats` and copies its kernel statistics to
profiles/r11_mod_ntt_kernel_stats.csv."""
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
    "mimc": (MIMC_P, 32, 3),
    "goldilocks": (2**64 - 2**32 + 1, 32, 7),
    "babybear": (2**31 - 2**27 + 1, 27, 11),
}
SHAPES = [(16, 1), (20, 1), (24, 1), (20, 8)]
ROUNDS = 5


def reps_for(lg, batch):
    return max(2, min(64, (1 << 24) // (batch << lg)))


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


def pair(L, ctx, name, x, y, n, batch):
    """one forward + inverse (x -> y -> y); name None: the tuned MiMC transform"""
    if name is None:
        w = b32(root("mimc", n))
        return lambda: (ck(L.sh_dev_ntt(ctx, x, y, n, batch, w, 0), "sh_dev_ntt"), ck(L.sh_dev_ntt(ctx, y, y, n, batch, w, 1), "sh_dev_ntt"))
    p, w = b32(FIELDS[name][0]), b32(root(name, n))
    return lambda: (ck(L.sh_dev_mod_ntt(ctx, p, x, y, n, batch, w, 0), "sh_dev_mod_ntt"),
                    ck(L.sh_dev_mod_ntt(ctx, p, y, y, n, batch, w, 1), "sh_dev_mod_ntt"))


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    big = 1 << 24
    x, y = ctypes.c_void_p(), ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, 32 * big, ctypes.byref(x)), "alloc")
    ck(L.sh_dev_alloc(ctx, 32 * big, ctypes.byref(y)), "alloc")
    ck(L.sh_dev_fill_seeded(ctx, x, big, 1), "fill")
    res = {"tool": "tools/mod_ntt_time.py", "rounds": ROUNDS,
           "stat": "min over rounds of (HIP-event ms of `reps` forward + inverse pairs) / reps, after a warm-up; paths alternate per round",
           "shapes": {}}
    for lg, batch in SHAPES:
        n, reps = 1 << lg, reps_for(lg, batch)
        fns = {"tuned_mimc": pair(L, ctx, None, x, y, n, batch)}
        for name in FIELDS:
            fns[name] = pair(L, ctx, name, x, y, n, batch)
        for fn in fns.values():  # warm-up
            fn()
        ck(L.sh_sync(ctx), "sync")
        best = {}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t = window(L, ctx, fn, reps)
                best[k] = min(best.get(k, t), t)
        row = {"reps": reps, "fwd_plus_inv_ms": best, "ratio_to_tuned": {k: best[k] / best["tuned_mimc"] for k in FIELDS},
               "elements_per_s": {k: 2 * batch * n / (best[k] * 1e-3) for k in best}}
        res["shapes"]["%dx2^%d" % (batch, lg)] = row
    res["bn254_ratio_2^20"] = res["shapes"]["1x2^20"]["ratio_to_tuned"]["bn254"]
    res["bn254_ratio_2^24"] = res["shapes"]["1x2^24"]["ratio_to_tuned"]["bn254"]
    res["condition_ratio_at_most_4"] = bool(res["bn254_ratio_2^20"] <= 4 and res["bn254_ratio_2^24"] <= 4)
    ck(L.sh_sync(ctx), "sync")
    for p in (x, y):
        L.sh_dev_free(ctx, p)
    ck(L.sh_ctx_trim(ctx), "trim")
    return res


def once():
    L, ctx = _lib.lib(), _lib.ctx()
    n = 1 << 24
    x, y = ctypes.c_void_p(), ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, 32 * n, ctypes.byref(x)), "alloc")
    ck(L.sh_dev_alloc(ctx, 32 * n, ctypes.byref(y)), "alloc")
    ck(L.sh_dev_fill_seeded(ctx, x, n, 1), "fill")
    for name in ("bn254", None):
        fn = pair(L, ctx, name, x, y, n, 1)
        fn()
        fn()
    ck(L.sh_sync(ctx), "sync")


def trace():
    out_dir = tempfile.mkdtemp(prefix="mod_ntt_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod_ntt", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r11_mod_ntt_kernel_stats.csv")
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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r11_mod_ntt.json")
    line = json.dumps(measure())
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
