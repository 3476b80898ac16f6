#!/usr/bin/env python3
"""Device time of the batch inversion and the four-point interpolation (GPU box), HIP events after a warm-up, best of REPS:
  * sh_dev_multi_inv at 2^16, 2^20, 2^24 and 2^26 elements (out of place, seeded values);
  * sh_dev_multi_interp_4 at 2^16 and 2^21 rows (2^21 = the rows of one fold of a 2^23-point FRI domain);
  * sh_dev_ntt at 2^24 in the same process, as the yardstick: its modmul-equivalent rate is (log2 n / 2) products per element.
The modmul-equivalents of the new calls are the products the kernels issue (inv_items.cuh): about 4 per element for multi_inv
(C = 4: 3/4 chunk + 1/4 tree up, then the down pass's 1 + 1/2 tree down + 3/2 backward walk) and 69 per row for multi_interp_4.
Prints one JSON line and writes it to argv[1] (default profiles/r08_poly_utils.json).  `--trace` runs each call once, for
`rocprofv3 --kernel-trace --stats -- python tools/poly_utils_time.py --trace`."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import _lib  # noqa: E402

P = 2**256 - 2**32 * 351 + 1
REPS = 5
MODMUL_PER_ELEMENT = 4.0
MODMUL_PER_ROW = 69.0


def ck(rc, where):
    _lib.check(rc, where)


def timed(L, ctx, fn, reps=REPS):
    fn()  # warm-up: code objects, workspaces
    ck(L.sh_sync(ctx), "sync")
    best = None
    for _ in range(reps):
        ck(L.sh_timer_start(ctx), "timer")
        fn()
        ms = ctypes.c_float()
        ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
        best = ms.value if best is None else min(best, ms.value)
    return best


def alloc(L, ctx, nbytes):
    p = ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(p)), "sh_dev_alloc")
    return p


def main():
    trace = "--trace" in sys.argv
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r08_poly_utils.json")
    L, ctx = _lib.lib(), _lib.ctx()
    reps = 1 if trace else REPS
    big = 1 << 26
    x, y = alloc(L, ctx, 32 * big), alloc(L, ctx, 32 * big)
    ck(L.sh_dev_fill_seeded(ctx, x, big, 1), "fill")
    res = {"tool": "tools/poly_utils_time.py", "reps": reps, "stat": "min ms of HIP events after one warm-up"}
    log_n = 24
    root = pow(7, (P - 1) >> log_n, P).to_bytes(32, "big")
    ntt_ms = timed(L, ctx, lambda: ck(L.sh_dev_ntt(ctx, x, y, 1 << log_n, 1, root, 0), "ntt"), reps)
    ntt_rate = (1 << log_n) * log_n / 2 / (ntt_ms * 1e-3)
    res["ntt_2^24"] = {"ms": ntt_ms, "modmul_eq_per_s": ntt_rate}
    for lg in (16, 20, 24, 26):
        n = 1 << lg
        ms = timed(L, ctx, lambda: ck(L.sh_dev_multi_inv(ctx, x, y, n), "multi_inv"), reps)
        rate = n * MODMUL_PER_ELEMENT / (ms * 1e-3)
        res["multi_inv_2^%d" % lg] = {"ms": ms, "elements_per_s": n / (ms * 1e-3), "modmul_eq_per_s": rate,
                                       "vs_ntt_modmul_rate": rate / ntt_rate, "GBps_algorithmic": 96.0 * n / (ms * 1e-3) / 1e9}
    for lg in (16, 21):
        rows = 1 << lg  # xs = x[0 .. 4 rows), ys = x[4 rows .. 8 rows), coeffs -> y
        ys = ctypes.c_void_p(x.value + 32 * 4 * rows)
        ms = timed(L, ctx, lambda: ck(L.sh_dev_multi_interp_4(ctx, x, ys, rows, y), "multi_interp_4"), reps)
        rate = rows * MODMUL_PER_ROW / (ms * 1e-3)
        res["multi_interp_4_2^%d_rows" % lg] = {"ms": ms, "rows_per_s": rows / (ms * 1e-3), "modmul_eq_per_s": rate,
                                                 "vs_ntt_modmul_rate": rate / ntt_rate}
    res["target_multi_inv_2^24_ms"] = 2.0
    res["target_met"] = res["multi_inv_2^24"]["ms"] <= 2.0
    for p in (x, y):
        L.sh_dev_free(ctx, p)
    line = json.dumps(res)
    print(line)
    if not trace:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
