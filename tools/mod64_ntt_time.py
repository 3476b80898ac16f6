#!/usr/bin/env python3
"""Time of the packed-word transform (GPU box): device time of sh_dev_mod64_ntt forward + inverse on seeded word-form vectors at 2^16,
2^20, 2^24, 2^28 and 8 x 2^20 over Goldilocks, BabyBear and the prime 2^64 - 1835007, and in the same run sh_dev_mod_ntt (the 32-byte
generic path) over Goldilocks at the shapes it supports (up to 2^26) as yardstick.  HIP events around REPS forward + inverse pairs
after a warm-up of every shape (tables, workspaces, code objects), the smallest of ROUNDS windows, the paths alternating round by
round.  `speedup_over_generic` is the generic time over the packed-word time of the same shape: the condition of the path is at least
4 x at 2^20, 2^24 and 8 x 2^20 over Goldilocks.  `hbm_fraction` is 16 B x batch n x passes x 2 / time over 8 TB/s (recorded, no
condition).  Then the Goldilocks shapes once more in two child processes under STARKHIP_MOD64_TILE_LOG=12 and 13 (`tile_log_ab`; the
knob is read once per process).  Prints one JSON line and writes it to argv[1] (default profiles/r12_mod64_ntt.json).  `--trace`
instead runs the 2^24 Goldilocks pair in a child process under `rocprofv3 --kernel-trace --stats` and copies its kernel statistics to
profiles/r12_mod64_ntt_kernel_stats.csv."""
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

# name -> (modulus, 2-adicity, a base whose (p - 1) / 2^adicity-th power has full order): tests/ntt64_cases.py
FIELDS = {
    "goldilocks": (2**64 - 2**32 + 1, 32, 7),
    "babybear": (2**31 - 2**27 + 1, 27, 11),
    "p64_1835007": (2**64 - 1835007, 18, 7),
}
SHAPES = [(16, 1), (20, 1), (24, 1), (28, 1), (20, 8)]
GENERIC_MAX_LOG = 26
ROUNDS = 5
HBM_BYTES_PER_S = 8e12


def reps_for(lg, batch):
    return max(2, min(64, (1 << 26) // (batch << lg)))


def passes_of(lg, tile_log):
    """the plan rule of include/starkhip.h"""
    return max(1, -(-lg // (tile_log - min(4, tile_log // 2))))


def tile_log():
    v = os.environ.get("STARKHIP_MOD64_TILE_LOG", "")
    return int(v) if v.isdigit() and 2 <= int(v) <= 13 else 12


def ck(rc, where):
    _lib.check(rc, where)


def root(name, n):
    p, v, base = FIELDS[name]
    return pow(pow(base, (p - 1) >> v, p), (1 << v) // n, p) if n <= 1 << v else None


def b32(x):
    return int(x).to_bytes(32, "big")


def window(L, ctx, fn, reps):
    ck(L.sh_timer_start(ctx), "timer")
    for _ in range(reps):
        fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value / reps


def pair64(L, ctx, name, x, y, n, batch):
    """one forward + inverse (x -> y -> y) on words"""
    p, w = FIELDS[name][0], root(name, n)
    return lambda: (ck(L.sh_dev_mod64_ntt(ctx, p, x, n, y, n, batch, w, 0), "sh_dev_mod64_ntt"),
                    ck(L.sh_dev_mod64_ntt(ctx, p, y, n, y, n, batch, w, 1), "sh_dev_mod64_ntt"))


def pair_generic(L, ctx, name, x, y, n, batch):
    """the same on 32-byte limbs through sh_dev_mod_ntt"""
    p, w = b32(FIELDS[name][0]), b32(root(name, n))
    return lambda: (ck(L.sh_dev_mod_ntt(ctx, p, x, y, n, batch, w, 0), "sh_dev_mod_ntt"),
                    ck(L.sh_dev_mod_ntt(ctx, p, y, y, n, batch, w, 1), "sh_dev_mod_ntt"))


def buffers(L, ctx, nbytes):
    x, y = ctypes.c_void_p(), ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(x)), "alloc")
    ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(y)), "alloc")
    ck(L.sh_dev_fill_seeded(ctx, x, nbytes // 32, 1), "fill")
    return x, y


def measure(fields, with_generic):
    L, ctx = _lib.lib(), _lib.ctx()
    x, y = buffers(L, ctx, 8 << 28)
    t = tile_log()
    shapes = {}
    for lg, batch in SHAPES:
        n, reps = 1 << lg, reps_for(lg, batch)
        fns = {}
        if with_generic and lg <= GENERIC_MAX_LOG and (batch << lg) <= 1 << GENERIC_MAX_LOG:
            fns["generic_goldilocks"] = pair_generic(L, ctx, "goldilocks", x, y, n, batch)
        for name in fields:
            if root(name, n) is not None:
                fns[name] = pair64(L, ctx, name, x, y, n, batch)
        for fn in fns.values():  # warm-up
            fn()
        ck(L.sh_sync(ctx), "sync")
        best = {}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                ms = window(L, ctx, fn, reps)
                best[k] = min(best.get(k, ms), ms)
        m = passes_of(lg, t)
        row = {"reps": reps, "passes": m, "fwd_plus_inv_ms": best,
               "hbm_fraction": {k: 16.0 * batch * n * m * 2 / (best[k] * 1e-3) / HBM_BYTES_PER_S for k in best if k in fields},
               "elements_per_s": {k: 2 * batch * n / (best[k] * 1e-3) for k in best}}
        if "generic_goldilocks" in best:
            row["speedup_over_generic"] = best["generic_goldilocks"] / best["goldilocks"]
        shapes["%dx2^%d" % (batch, lg)] = row
    ck(L.sh_sync(ctx), "sync")
    for p in (x, y):
        L.sh_dev_free(ctx, p)
    ck(L.sh_ctx_trim(ctx), "trim")
    return shapes


def child_ab():
    print(json.dumps({k: v["fwd_plus_inv_ms"]["goldilocks"] for k, v in measure(["goldilocks"], False).items()}))


def once():
    L, ctx = _lib.lib(), _lib.ctx()
    n = 1 << 24
    x, y = buffers(L, ctx, 8 * n)
    fn = pair64(L, ctx, "goldilocks", x, y, n, 1)
    fn()
    fn()
    ck(L.sh_sync(ctx), "sync")


def trace():
    out_dir = tempfile.mkdtemp(prefix="mod64_ntt_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod64_ntt", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r12_mod64_ntt_kernel_stats.csv")
        shutil.copyfile(stats[0], dst)
        print("wrote", dst)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    if "--trace" in sys.argv:
        return trace()
    if "--once" in sys.argv:
        return once()
    if "--child-ab" in sys.argv:
        return child_ab()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r12_mod64_ntt.json")
    res = {"tool": "tools/mod64_ntt_time.py", "rounds": ROUNDS, "tile_log": tile_log(),
           "stat": "min over rounds of (HIP-event ms of `reps` forward + inverse pairs) / reps, after a warm-up; paths alternate per round",
           "shapes": measure(list(FIELDS), True)}
    cond = {k: res["shapes"][k]["speedup_over_generic"] for k in ("1x2^20", "1x2^24", "8x2^20")}
    res["goldilocks_speedup_over_generic"] = cond
    res["condition_speedup_at_least_4"] = bool(all(v >= 4 for v in cond.values()))
    _lib.close()
    ab = {}
    for t in (12, 13):  # the knob is read once per process
        env = dict(os.environ, STARKHIP_MOD64_TILE_LOG=str(t))
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-ab"], capture_output=True, text=True, env=env, timeout=900,
                             check=True)
        ab[str(t)] = json.loads(out.stdout.strip().splitlines()[-1])
    res["tile_log_ab"] = {"goldilocks_fwd_plus_inv_ms": ab}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
