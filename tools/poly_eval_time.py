#!/usr/bin/env python3
"""Time of polynomial evaluation (GPU box), HIP events after a warm-up, best of REPS, seeded operands in limb form:
  * the issue's targets: direct path, 1 point of 2^24 coefficients and 64 points of 2^20; tree path, m = n = 2^20, next to
    sh_dev_lagrange_interp at 2^20 in the same process; products per second and coefficient bytes read per second of the direct path;
  * Polynomial.__call__ on a WireList-backed 2^20-coefficient polynomial end to end (wire upload included), next to the host loop
    over the same polynomial, and both at 16 .. 4096 coefficients (the device threshold EVAL_DEVICE_MIN_COEFS);
  * the crossover: each (n, m) shape with STARKHIP_EVAL_PATH=direct and =tree, each path in a child process (the knob is read once
    per process), and which path the default rule picks.
Prints one JSON line and writes it to argv[1] (default profiles/r10_poly_eval.json).  `--trace` instead runs the target calls once in
a child process under `rocprofv3 --kernel-trace --stats` and copies its kernel statistics to profiles/r10_poly_eval_kernel_stats.csv."""
import ctypes
import glob
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import _lib  # noqa: E402

P = 2**256 - 2**32 * 351 + 1
REPS = 3
SHAPES = [(1 << 24, 1), (1 << 20, 1 << 4), (1 << 20, 1 << 6), (1 << 20, 1 << 8), (1 << 16, 1 << 10), (1 << 18, 1 << 10),
          (1 << 14, 1 << 12), (1 << 16, 1 << 12), (1 << 12, 1 << 14), (1 << 14, 1 << 14), (1 << 16, 1 << 16), (1 << 24, 1 << 7)]


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


def shapes(reps):
    """{"n,m": ms} of every SHAPES entry under the path this process was started with"""
    L, ctx = _lib.lib(), _lib.ctx()
    x, y = alloc(L, ctx, 1 << 24), alloc(L, ctx, 1 << 24)
    ck(L.sh_dev_fill_seeded(ctx, x, 1 << 24, 5), "fill")
    out = {}
    for n, m in SHAPES:
        out["%d,%d" % (n, m)] = timed(L, ctx, lambda: ck(L.sh_dev_poly_eval(ctx, x, n, 1, at(x, (1 << 24) - m), m, y), "eval"), reps)
    return out


def measure(reps):
    L, ctx = _lib.lib(), _lib.ctx()
    big = 1 << 25
    x, y = alloc(L, ctx, big), alloc(L, ctx, big)
    ck(L.sh_dev_fill_seeded(ctx, x, big, 1), "fill")
    res = {"tool": "tools/poly_eval_time.py", "reps": reps, "stat": "min ms of HIP events after one warm-up"}
    ev = lambda n, m: ck(L.sh_dev_poly_eval(ctx, x, n, 1, at(x, big - m), m, y), "eval")  # noqa: E731
    t = res["direct_1pt_2^24_ms"] = timed(L, ctx, lambda: ev(1 << 24, 1), reps)
    res["direct_1pt_2^24_GB_per_s"] = 32 * 2**24 / (t * 1e-3) / 1e9
    t = res["direct_64pt_2^20_ms"] = timed(L, ctx, lambda: ev(1 << 20, 64), reps)
    res["direct_64pt_2^20_products_per_s"] = 64 * 2**20 / (t * 1e-3)
    res["direct_64pt_2^20_GB_per_s"] = 32 * 2**20 * 16 / (t * 1e-3) / 1e9  # 16 point groups, each reads the coefficients once
    n = 1 << 20
    res["tree_2^20x2^20_ms"] = timed(L, ctx, lambda: ev(n, n), reps)
    res["lagrange_2^20_ms"] = timed(L, ctx, lambda: ck(L.sh_dev_lagrange_interp(ctx, x, at(x, n), n, y), "lagrange"), reps)
    res["tree_over_lagrange_2^20"] = res["tree_2^20x2^20_ms"] / res["lagrange_2^20_ms"]
    for p in (x, y):
        L.sh_dev_free(ctx, p)
    # Polynomial.__call__ end to end (host bytes in, element out), device against the host loop
    from starks_amd import IntegersModP, polynomial
    from starks_amd.wireseq import WireList
    import numpy as np
    F = IntegersModP(P)
    Poly = polynomial.polynomials_over(F)
    raw = np.random.default_rng(3).integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x7f
    raw = raw.tobytes()
    xv = random.Random(4).randrange(P)
    call = {}
    for lg in (4, 6, 8, 10, 12, 20):
        poly = Poly(WireList(raw[:32 << lg], F))
        saved = polynomial.EVAL_DEVICE_MIN_COEFS
        try:
            polynomial.EVAL_DEVICE_MIN_COEFS = 1
            poly(xv)
            t0 = time.perf_counter()
            dv = poly(xv)
            dev_ms = (time.perf_counter() - t0) * 1e3
            polynomial.EVAL_DEVICE_MIN_COEFS = 1 << 30
            t0 = time.perf_counter()
            hv = poly(xv)
            host_ms = (time.perf_counter() - t0) * 1e3
        finally:
            polynomial.EVAL_DEVICE_MIN_COEFS = saved
        assert int(dv) == int(hv)
        call["2^%d" % lg] = {"device_ms": dev_ms, "host_loop_ms": host_ms}
    res["call_end_to_end"] = call
    res["eval_device_min_coefs"] = polynomial.EVAL_DEVICE_MIN_COEFS
    ck(L.sh_ctx_trim(ctx), "trim")
    return res


def crossover(reps):
    out = {}
    for path in ("direct", "tree", ""):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shapes"], capture_output=True, text=True, timeout=500,
                           env=dict(os.environ, STARKHIP_EVAL_PATH=path))
        if r.returncode != 0:
            raise SystemExit("child (%s) failed: %s" % (path or "default", r.stderr[-2000:]))
        out[path or "default"] = json.loads(r.stdout.strip().splitlines()[-1])
    return {k: {p: out[p][k] for p in out} for k in out["direct"]}


def trace():
    out_dir = tempfile.mkdtemp(prefix="poly_eval_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "poly_eval", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r10_poly_eval_kernel_stats.csv")
        shutil.copyfile(stats[0], dst)
        print("wrote", dst)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def once():
    L, ctx = _lib.lib(), _lib.ctx()
    big = 1 << 25
    x, y = alloc(L, ctx, big), alloc(L, ctx, big)
    ck(L.sh_dev_fill_seeded(ctx, x, big, 1), "fill")
    for n, m in ((1 << 24, 1), (1 << 20, 64), (1 << 20, 1 << 20)):
        ck(L.sh_dev_poly_eval(ctx, x, n, 1, at(x, big - m), m, y), "eval")
    ck(L.sh_sync(ctx), "sync")


def main():
    if "--trace" in sys.argv:
        return trace()
    if "--once" in sys.argv:
        return once()
    if "--shapes" in sys.argv:
        print(json.dumps(shapes(REPS)))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r10_poly_eval.json")
    res = measure(REPS)
    res["crossover_ms"] = crossover(REPS)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
