#!/usr/bin/env python3
"""Device time of the polynomial arithmetic (GPU box), HIP events after a warm-up, best of REPS, seeded operands in limb form:
  * sh_dev_poly_mul of two 2^23-coefficient polynomials;
  * sh_dev_poly_divmod of 2^24 coefficients by 2^23 and by 2^4;
  * sh_dev_zpoly and sh_dev_lagrange_interp at 2^12, 2^16 and 2^20 points;
  * sh_dev_ntt at 2^24 in the same process, as the yardstick.
"lagrange_2^20_over_2^16" is the scaling ratio (O(n log^2 n) predicts about 25, O(n^2) 256).
Prints one JSON line and writes it to argv[1] (default profiles/r09_poly_arith.json).  `--trace` instead runs every call once in a
child process under `rocprofv3 --kernel-trace --stats` and copies its kernel statistics to profiles/r09_poly_arith_kernel_stats.csv."""
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

P = 2**256 - 2**32 * 351 + 1
REPS = 3


def ck(rc, where):
    _lib.check(rc, where)


def timed(L, ctx, fn, reps):
    fn()  # warm-up: code objects, plans, workspaces
    ck(L.sh_sync(ctx), "sync")
    best = None
    for _ in range(reps):
        ck(L.sh_timer_start(ctx), "timer")
        fn()
        ms = ctypes.c_float()
        ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
        best = ms.value if best is None else min(best, ms.value)
    return best


def alloc(L, ctx, n):
    p = ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, 32 * n, ctypes.byref(p)), "sh_dev_alloc")
    return p


def at(p, k):
    return ctypes.c_void_p(p.value + 32 * k)


def measure(reps):
    L, ctx = _lib.lib(), _lib.ctx()
    big = 1 << 25
    x, y = alloc(L, ctx, big), alloc(L, ctx, big)
    ck(L.sh_dev_fill_seeded(ctx, x, big, 1), "fill")
    res = {"tool": "tools/poly_arith_time.py", "reps": reps, "stat": "min ms of HIP events after one warm-up"}
    root = pow(7, (P - 1) >> 24, P).to_bytes(32, "big")
    res["ntt_2^24_ms"] = timed(L, ctx, lambda: ck(L.sh_dev_ntt(ctx, x, y, 1 << 24, 1, root, 0), "ntt"), reps)
    h = 1 << 23
    res["mul_2^23x2^23_ms"] = timed(L, ctx, lambda: ck(L.sh_dev_poly_mul(ctx, x, h, at(x, h), h, y), "poly_mul"), reps)
    m = 1 << 24
    for lb in (23, 4):
        k = 1 << lb
        res["divmod_2^24_by_2^%d_ms" % lb] = timed(
            L, ctx, lambda: ck(L.sh_dev_poly_divmod(ctx, x, m, at(x, m), k, y, at(y, m)), "poly_divmod"), reps)
    for lg in (12, 16, 20):
        n = 1 << lg
        res["zpoly_2^%d_ms" % lg] = timed(L, ctx, lambda: ck(L.sh_dev_zpoly(ctx, x, n, y), "zpoly"), reps)
        res["lagrange_2^%d_ms" % lg] = timed(L, ctx, lambda: ck(L.sh_dev_lagrange_interp(ctx, x, at(x, n), n, y), "lagrange"), reps)
    res["lagrange_2^20_over_2^16"] = res["lagrange_2^20_ms"] / res["lagrange_2^16_ms"]
    res["zpoly_2^20_over_2^16"] = res["zpoly_2^20_ms"] / res["zpoly_2^16_ms"]
    res["paper_estimates_ms"] = {"mul_2^23x2^23": 4.0, "zpoly_2^20": 10.0}
    for p in (x, y):
        L.sh_dev_free(ctx, p)
    ck(L.sh_ctx_trim(ctx), "trim")
    return res


def trace():
    out_dir = tempfile.mkdtemp(prefix="poly_arith_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "poly_arith", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r09_poly_arith_kernel_stats.csv")
        shutil.copyfile(stats[0], dst)
        print("wrote", dst)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    if "--trace" in sys.argv:
        return trace()
    if "--once" in sys.argv:
        print(json.dumps(measure(1)))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r09_poly_arith.json")
    line = json.dumps(measure(REPS))
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
