#!/usr/bin/env python3
"""Time of polynomial evaluation over a run-time modulus (sh_mod_poly_eval; GPU box), four parts.

"device": HIP-event device time of whole sh_dev_mod_poly_eval calls over BN254 on the default path, the smallest of ROUNDS rounds
after a warm-up, at the README's sh_poly_eval shapes -- 1 point x 2^24 coefficients, 64 x 2^20, 2^20 x 2^20 -- each beside
sh_dev_poly_eval on the same shape and beside sh_dev_mod_ntt / sh_dev_ntt at the tree path's dominant transform (2 pow2(m); for the
direct shapes, which run no transform, the ratio at 2^20 is the yardstick), all in the same run; Goldilocks at 64 x 2^20.  Per shape:
mod_ms, mimc_ms, `ratio`, `ntt.ratio` and `holds` = ratio <= ntt.ratio.  Reported, not gated.

"call_end_to_end": Polynomial.__call__ over IntegersModP(BN254) on a 2^20-coefficient polynomial, wall clock, device against host loop.

"crossover_ms": both forced paths (STARKHIP_EVAL_PATH=direct and =tree, each in a fresh child process: the knob is read once per
process) and the default over the twelve crossover shapes of profiles/r10_poly_eval.json.  A call whose warm-up takes more than
SLOW_MS is timed once, not ROUNDS times (the forced tree at 1 point x 2^24 coefficients runs 2^23 rows).  "fit": the five constants
of the generic cost rule (csrc/modeval_items.cuh: ME_COST) fitted to those times by least squares on relative error -- the direct
path's floor and products per us, the tree's us per level, elements per us and us per row -- with the rule's choice under the fitted
constants beside the faster path per shape.

"routing": wall clock, end to end, of Polynomial.__call__ (n coefficients, one point) and poly_utils.multi_eval (n coefficients at 8
points and at n points) over IntegersModP(BN254), the device call against the host loop on the same inputs in the same run, at powers
of two; `threshold` = the smallest measured power of two (of n for __call__, of n m for multi_eval) from which the device call wins at
every larger measured size.  MOD_EVAL_DEVICE_MIN_COEFS (polynomial.py) and MOD_EVAL_DEVICE_MIN_WORK (poly_utils.py) cite them.

Prints one JSON line and writes it to argv[1] (default profiles/r22_mod_poly_eval.json); `--no-crossover` leaves out the forced
paths and the fit.  profiles/r22_mod_poly_eval_check.json is a second run of the same tool, made with the fitted constants in place."""
import ctypes
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import IntegersModP, _lib, poly_utils, polynomial  # noqa: E402

BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GOLDILOCKS = 2**64 - 2**32 + 1
MIMC_P = _lib.MIMC_P
ROUNDS = 5
SLOW_MS = 1000.0
HOST_CAP_S = 1.0
SHAPES = [(1 << 24, 1), (1 << 20, 1 << 4), (1 << 20, 1 << 6), (1 << 20, 1 << 8), (1 << 16, 1 << 10), (1 << 18, 1 << 10),
          (1 << 14, 1 << 12), (1 << 16, 1 << 12), (1 << 12, 1 << 14), (1 << 14, 1 << 14), (1 << 16, 1 << 16), (1 << 24, 1 << 7)]


def ck(rc, where):
    _lib.check(rc, where)


def once(L, ctx, fn):
    ck(L.sh_timer_start(ctx), "timer")
    fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value


def best(L, ctx, fns):
    """the smallest of ROUNDS rounds of each fn after one (timed) warm-up, the fns alternating round by round; a fn whose warm-up
    exceeds SLOW_MS keeps that one further round"""
    warm = [once(L, ctx, fn) for fn in fns]
    res = [float("inf")] * len(fns)
    for r in range(ROUNDS):
        for i, fn in enumerate(fns):
            if r == 0 or warm[i] <= SLOW_MS:
                res[i] = min(res[i], once(L, ctx, fn))
    return res


def alloc(L, ctx, n):
    p = ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, 32 * n, ctypes.byref(p)), "sh_dev_alloc")
    return p


def at(p, k):
    return ctypes.c_void_p(p.value + 32 * k)


def pow2_at_least(n):
    s = 2
    while s < n:
        s *= 2
    return s


def device_part(L, ctx):
    big = 1 << 25
    x, y, z = alloc(L, ctx, big), alloc(L, ctx, big), alloc(L, ctx, 1 << 22)
    ck(L.sh_dev_fill_seeded(ctx, x, big, 1), "fill")  # values below the MiMC prime: plain 256-bit inputs for every modulus
    out = []

    def ntt_ratio(p, size):
        m, w, k = _lib.mod_poly_args(p)
        lg = size.bit_length() - 1
        wm = pow(int.from_bytes(w, "big"), 1 << (k - lg), p).to_bytes(32, "big")
        wq = pow(7, (MIMC_P - 1) >> lg, MIMC_P).to_bytes(32, "big")
        a, b = best(L, ctx, [lambda: ck(L.sh_dev_mod_ntt(ctx, m, x, z, size, 1, wm, 0), "sh_dev_mod_ntt"),
                             lambda: ck(L.sh_dev_ntt(ctx, x, z, size, 1, wq, 0), "sh_dev_ntt")])
        return {"size_log": lg, "mod_ms": round(a, 4), "mimc_ms": round(b, 4), "ratio": round(a / b, 3)}

    def row(p, name, n, m, dominant):
        mod, w, k = _lib.mod_poly_args(p)
        a, b = best(L, ctx, [lambda: ck(L.sh_dev_mod_poly_eval(ctx, mod, w, k, x, n, 1, at(x, big - m), m, y), "sh_dev_mod_poly_eval"),
                             lambda: ck(L.sh_dev_poly_eval(ctx, x, n, 1, at(x, big - m), m, y), "sh_dev_poly_eval")])
        rec = {"modulus": name, "n": n, "m": m, "mod_ms": round(a, 4), "mimc_ms": round(b, 4), "ratio": round(a / b, 3),
               "ntt": ntt_ratio(p, dominant)}
        rec["holds"] = rec["ratio"] <= rec["ntt"]["ratio"]
        out.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)

    row(BN254, "bn254", 1 << 24, 1, 1 << 20)
    row(BN254, "bn254", 1 << 20, 64, 1 << 20)
    row(BN254, "bn254", 1 << 20, 1 << 20, 1 << 21)
    row(GOLDILOCKS, "goldilocks", 1 << 20, 64, 1 << 20)
    for p in (x, y, z):
        L.sh_dev_free(ctx, p)
    ck(L.sh_ctx_trim(ctx), "trim")
    return out


def shapes_child():
    """{"n,m": ms} of every SHAPES entry over BN254 under the path this process was started with"""
    L, ctx = _lib.lib(), _lib.ctx()
    x, y = alloc(L, ctx, 1 << 24), alloc(L, ctx, 1 << 24)
    ck(L.sh_dev_fill_seeded(ctx, x, 1 << 24, 5), "fill")
    mod, w, k = _lib.mod_poly_args(BN254)
    out = {}
    for n, m in SHAPES:
        out["%d,%d" % (n, m)] = best(L, ctx, [lambda: ck(L.sh_dev_mod_poly_eval(ctx, mod, w, k, x, n, 1, at(x, (1 << 24) - m), m, y), "eval")])[0]
        print(n, m, out["%d,%d" % (n, m)], file=sys.stderr, flush=True)
    return out


def crossover():
    out = {}
    for path in ("direct", "tree", ""):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shapes"], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, STARKHIP_EVAL_PATH=path))
        if r.returncode != 0:
            raise SystemExit("child (%s) failed: %s" % (path or "default", r.stderr[-2000:]))
        out[path or "default"] = json.loads(r.stdout.strip().splitlines()[-1])
    return {k: {p: out[p][k] for p in out} for k in out["direct"]}


def fit(cross):
    """least squares on relative error: direct_us = floor + n m / rate; tree_us = L lg + (N lg^2 + 3 R N lg) / E + r R"""
    import numpy as np

    def solve(rows, times):
        A = np.array(rows, dtype=float) / np.array(times, dtype=float)[:, None]
        b = np.ones(len(times))
        keep = list(range(A.shape[1]))
        while True:
            sol = np.linalg.lstsq(A[:, keep], b, rcond=None)[0]
            if (sol >= 0).all() or len(keep) == 1:
                break
            keep.pop(int(np.argmin(sol)))  # a negative term explains nothing here: drop it and fit the rest
        full = [0.0] * A.shape[1]
        for i, s in zip(keep, sol):
            full[i] = max(float(s), 0.0)
        return full

    keys = list(cross)
    nm = [tuple(int(v) for v in k.split(",")) for k in keys]
    d_us = [1e3 * cross[k]["direct"] for k in keys]
    t_us = [1e3 * cross[k]["tree"] for k in keys]
    floor, inv_rate = solve([[1.0, float(n) * m] for n, m in nm], d_us)
    trows = []
    for n, m in nm:
        N = pow2_at_least(m)
        lg, R = float(N.bit_length() - 1), float((n + N - 1) // N)
        trows.append([lg, N * lg * lg + 3.0 * R * N * lg, R])
    per_level, inv_elems, per_row = solve(trows, t_us)
    big = 1e30
    consts = {"direct_products_per_us": 1.0 / inv_rate if inv_rate else big, "direct_floor_us": floor, "tree_us_per_level": per_level,
              "tree_elements_per_us": 1.0 / inv_elems if inv_elems else big, "tree_us_per_row": per_row}
    table = []
    for (n, m), k, dr, tr in zip(nm, keys, trows, trows):
        pd = floor + inv_rate * n * m
        pt = per_level * tr[0] + inv_elems * tr[1] + per_row * tr[2]
        table.append({"shape": k, "direct_us": round(1e3 * cross[k]["direct"], 1), "direct_fit_us": round(pd, 1),
                      "tree_us": round(1e3 * cross[k]["tree"], 1), "tree_fit_us": round(pt, 1),
                      "faster": "direct" if cross[k]["direct"] <= cross[k]["tree"] else "tree", "rule": "direct" if pd <= pt else "tree"})
    return {"constants": consts, "shapes": table, "rule_agrees": sum(r["faster"] == r["rule"] for r in table), "of": len(table)}


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def host_call(coefs, x, F):
    y, pw = F(0), F(1)
    for a in coefs:
        y = y + pw * a
        pw = pw * x
    return y


def threshold(rows, key):
    thr = None
    for r in reversed(rows):
        if r["host_ms"] is None or r["device_ms"] < r["host_ms"]:
            thr = r[key]
        else:
            break
    return thr


def routing_part():
    p = BN254
    F = IntegersModP(p)
    rnd = random.Random(1)
    W = lambda v: _lib.to_wire(v, p)  # noqa: E731
    WL = polynomial.WireList

    def dev_call(coefs, x):
        return WL(polynomial.mod_eval_wire(p, W(coefs), W([x])), F)[0]

    def dev_multi(coefs, xs):
        return WL(polynomial.mod_eval_wire(p, W(coefs), W(xs)), F)

    def host_multi(coefs, xs):
        return [host_call(coefs, x, F) for x in xs]

    def sweep(make, dev, host, lgs, key, work):
        rows, host_on = [], True
        for lg in lgs:
            args = make(1 << lg)
            dev(*args)
            td = min(wall(lambda: dev(*args)) for _ in range(3))
            th = None
            if host_on:
                th = min(wall(lambda: host(*args)) for _ in range(2 if lg <= 6 else 1))
                host_on = th < HOST_CAP_S
            rows.append({key: work(1 << lg), "n": 1 << lg, "device_ms": round(1e3 * td, 3), "host_ms": None if th is None else round(1e3 * th, 3)})
        return {"sizes": rows, "threshold": threshold(rows, key)}

    elems = lambda n: [F(rnd.randrange(p)) for _ in range(n)]  # noqa: E731
    out = {
        "call": sweep(lambda n: (elems(n), F(rnd.randrange(p))), dev_call, lambda c, x: host_call(c, x, F), range(2, 15), "n", lambda n: n),
        "multi_eval_8_points": sweep(lambda n: (elems(n), elems(8)), dev_multi, host_multi, range(0, 13), "work", lambda n: 8 * n),
        "multi_eval_square": sweep(lambda n: (elems(n), elems(n)), dev_multi, host_multi, range(1, 10), "work", lambda n: n * n),
    }
    for k, v in out.items():
        print(json.dumps({k: v}), file=sys.stderr, flush=True)
    return out


def call_end_to_end():
    import numpy as np
    p, n = BN254, 1 << 20
    F = IntegersModP(p)
    raw = np.random.default_rng(3).integers(0, 256, size=(n, 32), dtype=np.uint8)
    raw[:, 0] &= 0x1f  # below 2^253 < p
    poly = polynomial.polynomials_over(F)(polynomial.WireList(raw.tobytes(), F))
    xv = random.Random(4).randrange(p)
    saved = polynomial.MOD_EVAL_DEVICE_MIN_COEFS
    try:
        polynomial.MOD_EVAL_DEVICE_MIN_COEFS = 1
        poly(xv)
        dev_ms = 1e3 * min(wall(lambda: poly(xv)) for _ in range(3))
        polynomial.MOD_EVAL_DEVICE_MIN_COEFS = 1 << 30
        t0 = time.perf_counter()
        hv = poly(xv)
        host_ms = 1e3 * (time.perf_counter() - t0)
        polynomial.MOD_EVAL_DEVICE_MIN_COEFS = 1
        assert int(poly(xv)) == int(hv)
    finally:
        polynomial.MOD_EVAL_DEVICE_MIN_COEFS = saved
    return {"log_n": 20, "device_ms": round(dev_ms, 3), "host_loop_ms": round(host_ms, 1)}


def main():
    if "--shapes" in sys.argv:
        print(json.dumps(shapes_child()))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dst = args[0] if args else os.path.join(ROOT, "profiles", "r22_mod_poly_eval.json")
    L, ctx = _lib.lib(), _lib.ctx()
    res = {"tool": "tools/mod_poly_eval_time.py", "rounds": ROUNDS, "device": device_part(L, ctx)}
    res["call_end_to_end"] = call_end_to_end()
    res["routing"] = routing_part()
    res["routing"]["MOD_EVAL_DEVICE_MIN_COEFS"] = polynomial.MOD_EVAL_DEVICE_MIN_COEFS
    res["routing"]["MOD_EVAL_DEVICE_MIN_WORK"] = poly_utils.MOD_EVAL_DEVICE_MIN_WORK
    ck(L.sh_ctx_trim(ctx), "trim")
    if "--no-crossover" not in sys.argv:
        res["crossover_ms"] = crossover()
        res["fit"] = fit(res["crossover_ms"])
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
