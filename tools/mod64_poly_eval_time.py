#!/usr/bin/env python3
"""Time of polynomial evaluation on packed 64-bit words (sh_mod64_poly_eval; GPU box), three parts.  Every time is HIP-event device time
of a whole sh_dev_ call: after one warm-up of every entry of a comparison the entries alternate for ROUNDS rounds, and the median (with
the smallest and largest round) is kept.  Inputs are canonical random words; the twin runs on the same values as limbs
(sh_dev_mod64_to_limbs, once, outside the timed region).

"device": sh_dev_mod64_poly_eval beside sh_dev_mod_poly_eval over the same field at the README's shapes over Goldilocks -- 1 point x
2^24 coefficients, 64 x 2^20, 2^20 x 2^20 -- and 64 x 2^20 over BabyBear, each with sh_dev_mod64_ntt : sh_dev_mod_ntt at the tree
path's dominant transform (2 pow2(m); for the direct shapes, which run no transform, at 2^20).  Per shape: `ratio` = packed / twin
(the condition: <= 1), `ntt.ratio`, and `aim` = HOLDS when ratio <= ntt.ratio, else MISSED.  The 1 x 2^24 row also states the
coefficient bytes per second.

"group": the direct path's points per lane.  For each library given as --group G=PATH (builds with -DM6E_GROUP_POINTS=G; each in a
fresh child process under STARKHIP_LIB) the forced direct path at 64 x 2^20, 2^10 points x 2^16 coefficients and 2^14 x 2^14 (a
grid that every build fills), and at m = G - 1 beside m = G over 2^20 coefficients (the shape rule runs m = G - 1 with one point per
lane).

"crossover_ms": both forced paths (STARKHIP_EVAL_PATH=direct and =tree, each in a fresh child process: the knob is read once per
process) and the default over the twelve crossover shapes of tools/mod_poly_eval_time.py.  A call whose warm-up takes more than SLOW_MS
is timed once more, not ROUNDS times.  "fit": the five constants of the packed cost rule (csrc/mod64eval_items.cuh: M6E_COST) fitted to
those times by least squares on relative error (mod_poly_eval_time.fit), with the rule's choice under the fitted constants beside the
faster path per shape; "fit_weighted": the same fit with every shape's relative error weighted by min / max of its two paths' times
(the constants M6E_COST rounds: see weighted_fit); "default_took": per shape the path whose time the default's is nearer to, "default_slower": the shapes where that
is the slower one, with both times.  "beyond_ms": the same three times at BEYOND, shapes outside the twelve that take no part in the
fits (2^25 coefficients at 2^12 points: 8192 rows), and part of "default_took" / "default_slower".

`--trace-child` runs four calls of each "device" shape over Goldilocks and nothing else: the program for
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mod64_poly_eval_time.py --trace-child`, whose kernel
statistics are profiles/r24_mod64_poly_eval_kernel_stats.csv.

Prints one JSON line and writes it to argv[1] (default profiles/r24_mod64_poly_eval.json); `--no-crossover` and `--no-device` leave
parts out.  profiles/r24_mod64_poly_eval_check.json is a second run of the same tool, made with the fitted constants in place."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from starks_amd import _lib  # noqa: E402
from mod_poly_eval_time import SHAPES, fit, pow2_at_least  # noqa: E402

MODULI = {"goldilocks": 2**64 - 2**32 + 1, "babybear": 15 * 2**27 + 1}
ROUNDS = 7
SLOW_MS = 1000.0
CAP = 1 << 24  # coefficient words per buffer
BEYOND = [(1 << 25, 1 << 12)]  # outside the fitted shapes: many rows at mid-sized m, where the weighted model underprices the tree
PTS = 1 << 20


def ck(rc, where):
    _lib.check(rc, where)


def once(L, ctx, fn):
    ck(L.sh_timer_start(ctx), "timer")
    fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value


def stats(x):
    return {"median_ms": round(statistics.median(x), 4), "min_ms": round(min(x), 4), "max_ms": round(max(x), 4)}


def alternating(L, ctx, fns):
    """statistics per fn over ROUNDS alternating rounds after one timed warm-up of each; a fn whose warm-up exceeds SLOW_MS runs one
    more round only"""
    warm = [once(L, ctx, fn) for fn in fns]
    t = [[] for _ in fns]
    for r in range(ROUNDS):
        for i, fn in enumerate(fns):
            if r == 0 or warm[i] <= SLOW_MS:
                t[i].append(once(L, ctx, fn))
    return [stats(x) for x in t]


def alloc(L, ctx, nbytes):
    p = ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(p)), "sh_dev_alloc")
    return p


def fill(L, ctx, d, count, p, seed):
    import numpy as np
    raw = np.random.default_rng(seed).integers(0, p, size=count, dtype=np.uint64).tobytes()
    ck(L.sh_dev_upload(ctx, raw, d, len(raw)), "sh_dev_upload")


def device_part(L, ctx):
    W, X, O = alloc(L, ctx, 8 * CAP), alloc(L, ctx, 8 * PTS), alloc(L, ctx, 8 * 2 * PTS)
    a, x, o = alloc(L, ctx, 32 * CAP), alloc(L, ctx, 32 * PTS), alloc(L, ctx, 32 * 2 * PTS)
    out = []
    for name, n, m, dominant in (("goldilocks", 1 << 24, 1, 1 << 20), ("goldilocks", 1 << 20, 64, 1 << 20),
                                 ("goldilocks", 1 << 20, 1 << 20, 1 << 21), ("babybear", 1 << 20, 64, 1 << 20)):
        p = MODULI[name]
        fill(L, ctx, W, CAP, p, 24)
        fill(L, ctx, X, PTS, p, 25)
        ck(L.sh_dev_mod64_to_limbs(ctx, W, a, CAP), "sh_dev_mod64_to_limbs")
        ck(L.sh_dev_mod64_to_limbs(ctx, X, x, PTS), "sh_dev_mod64_to_limbs")
        mod, w, k = _lib.mod64_poly_args(p)
        gm, gw, gk = _lib.mod_poly_args(p)
        s64, s32 = alternating(L, ctx, [lambda: ck(L.sh_dev_mod64_poly_eval(ctx, mod, w, k, W, n, 1, X, m, O), "sh_dev_mod64_poly_eval"),
                                        lambda: ck(L.sh_dev_mod_poly_eval(ctx, gm, gw, gk, a, n, 1, x, m, o), "sh_dev_mod_poly_eval")])
        lg = dominant.bit_length() - 1
        wr = pow(w, 1 << (k - lg), p)
        t64, t32 = alternating(L, ctx, [lambda: ck(L.sh_dev_mod64_ntt(ctx, mod, W, dominant, O, dominant, 1, wr, 0), "sh_dev_mod64_ntt"),
                                        lambda: ck(L.sh_dev_mod_ntt(ctx, gm, a, o, dominant, 1, wr.to_bytes(32, "big"), 0), "sh_dev_mod_ntt")])
        rec = {"modulus": name, "n": n, "m": m, "packed": s64, "twin": s32, "ratio": round(s64["median_ms"] / s32["median_ms"], 4),
               "ntt": {"size_log": lg, "packed": t64, "twin": t32, "ratio": round(t64["median_ms"] / t32["median_ms"], 4)}}
        rec["not_slower"] = rec["ratio"] <= 1.0
        rec["aim"] = "HOLDS" if rec["ratio"] <= rec["ntt"]["ratio"] else "MISSED"
        if m == 1:
            rec["coefficient_bytes_per_s"] = round(8 * n / (1e-3 * s64["median_ms"]), 0)
        out.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    for d in (W, X, O, a, x, o):
        L.sh_dev_free(ctx, d)
    ck(L.sh_ctx_trim(ctx), "trim")
    return out


def child_buffers(L, ctx, cap=CAP):
    p = MODULI["goldilocks"]
    W, X, O = alloc(L, ctx, 8 * cap), alloc(L, ctx, 8 * PTS), alloc(L, ctx, 8 * PTS)
    fill(L, ctx, W, cap, p, 5)
    fill(L, ctx, X, PTS, p, 6)
    return _lib.mod64_poly_args(p) + (W, X, O)


def shapes_child():
    """{"n,m": median ms} of every SHAPES entry over Goldilocks under the path this process was started with"""
    L, ctx = _lib.lib(), _lib.ctx()
    mod, w, k, W, X, O = child_buffers(L, ctx, max(n for n, _ in SHAPES + BEYOND))
    out = {}
    for n, m in SHAPES + BEYOND:
        s = alternating(L, ctx, [lambda: ck(L.sh_dev_mod64_poly_eval(ctx, mod, w, k, W, n, 1, X, m, O), "eval")])[0]
        out["%d,%d" % (n, m)] = s["median_ms"]
        print(n, m, s, file=sys.stderr, flush=True)
    return out


def group_child(G):
    """the direct path of the library this process loaded (G points per lane)"""
    L, ctx = _lib.lib(), _lib.ctx()
    mod, w, k, W, X, O = child_buffers(L, ctx)
    out = {"G": G}
    for key, n, m in (("64x2^20", 1 << 20, 64), ("2^10x2^16", 1 << 16, 1 << 10), ("2^14x2^14", 1 << 14, 1 << 14),
                      ("m=G-1,2^20", 1 << 20, G - 1), ("m=G,2^20", 1 << 20, G)):
        out[key] = alternating(L, ctx, [lambda: ck(L.sh_dev_mod64_poly_eval(ctx, mod, w, k, W, n, 1, X, m, O), "eval")])[0]
    return out


def child(args, env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **env))
    if r.returncode != 0:
        raise SystemExit("child %s %s failed: %s" % (args, env, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def crossover():
    """(the twelve shapes' times, BEYOND's times), each {"n,m": {"direct", "tree", "default"}}"""
    out = {path or "default": child(["--shapes"], {"STARKHIP_EVAL_PATH": path}) for path in ("direct", "tree", "")}
    table = {k: {p: out[p][k] for p in out} for k in out["direct"]}
    beyond = {"%d,%d" % s for s in BEYOND}
    return {k: v for k, v in table.items() if k not in beyond}, {k: v for k, v in table.items() if k in beyond}


def trace_child():
    """four calls of each "device" shape over Goldilocks, for `rocprofv3 --kernel-trace --stats -- python THIS --trace-child`"""
    L, ctx = _lib.lib(), _lib.ctx()
    mod, w, k, W, X, O = child_buffers(L, ctx)
    for n, m in ((1 << 24, 1), (1 << 20, 64), (1 << 20, 1 << 20)):
        for _ in range(4):
            ck(L.sh_dev_mod64_poly_eval(ctx, mod, w, k, W, n, 1, X, m, O), "eval")
        ck(L.sh_sync(ctx), "sync")


def weighted_fit(cross):
    """mod_poly_eval_time.fit with every shape's relative error weighted by min / max of its two paths' times: a shape on which one
    path is a hundred times the other says nothing about where the rule's decisions lie, and the model's one term per level cannot
    follow the tree from 10 levels to 23 at once"""
    import numpy as np

    def solve(rows, times, w):
        A = np.array(rows, dtype=float) / np.array(times, dtype=float)[:, None] * np.array(w)[:, None]
        keep = list(range(A.shape[1]))
        while True:
            sol = np.linalg.lstsq(A[:, keep], np.array(w), rcond=None)[0]
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
    w = [min(a, b) / max(a, b) for a, b in zip(d_us, t_us)]
    floor, inv_rate = solve([[1.0, float(n) * m] for n, m in nm], d_us, w)
    trows = []
    for n, m in nm:
        N = pow2_at_least(m)
        lg, R = float(N.bit_length() - 1), float((n + N - 1) // N)
        trows.append([lg, N * lg * lg + 3.0 * R * N * lg, R])
    per_level, inv_elems, per_row = solve(trows, t_us, w)
    big = 1e30
    consts = {"direct_products_per_us": 1.0 / inv_rate if inv_rate else big, "direct_floor_us": floor, "tree_us_per_level": per_level,
              "tree_elements_per_us": 1.0 / inv_elems if inv_elems else big, "tree_us_per_row": per_row}
    table = []
    for (n, m), k, tr, wk in zip(nm, keys, trows, w):
        pd = floor + inv_rate * n * m
        pt = per_level * tr[0] + inv_elems * tr[1] + per_row * tr[2]
        table.append({"shape": k, "weight": round(wk, 4), "direct_us": round(1e3 * cross[k]["direct"], 1), "direct_fit_us": round(pd, 1),
                      "tree_us": round(1e3 * cross[k]["tree"], 1), "tree_fit_us": round(pt, 1),
                      "faster": "direct" if cross[k]["direct"] <= cross[k]["tree"] else "tree", "rule": "direct" if pd <= pt else "tree"})
    return {"constants": consts, "shapes": table, "rule_agrees": sum(r["faster"] == r["rule"] for r in table), "of": len(table)}


def default_choice(cross):
    took, slower = {}, []
    for k, t in cross.items():
        took[k] = "direct" if abs(t["default"] - t["direct"]) <= abs(t["default"] - t["tree"]) else "tree"
        faster = "direct" if t["direct"] <= t["tree"] else "tree"
        if took[k] != faster:
            slower.append({"shape": k, "direct_ms": t["direct"], "tree_ms": t["tree"], "default_ms": t["default"]})
    return took, slower


def main():
    argv = sys.argv[1:]
    if "--shapes" in argv:
        print(json.dumps(shapes_child()))
        return
    if "--trace-child" in argv:
        trace_child()
        return
    if "--group-child" in argv:
        print(json.dumps(group_child(int(argv[argv.index("--group-child") + 1]))))
        return
    groups = [argv[i + 1] for i, a in enumerate(argv) if a == "--group"]
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--group")]
    dst = args[0] if args else os.path.join(ROOT, "profiles", "r24_mod64_poly_eval.json")
    res = {"tool": "tools/mod64_poly_eval_time.py", "rounds": ROUNDS}
    if "--no-device" not in argv:
        L, ctx = _lib.lib(), _lib.ctx()
        res["device"] = device_part(L, ctx)
    if groups:
        res["group"] = []
        for spec in groups:
            G, path = spec.split("=", 1)
            res["group"].append(child(["--group-child", G], {"STARKHIP_LIB": os.path.abspath(path), "STARKHIP_EVAL_PATH": "direct"}))
            print(json.dumps(res["group"][-1]), file=sys.stderr, flush=True)
    if "--no-crossover" not in argv:
        res["crossover_ms"], res["beyond_ms"] = crossover()
        res["fit"] = fit(res["crossover_ms"])
        res["fit_weighted"] = weighted_fit(res["crossover_ms"])
        res["default_took"], res["default_slower"] = default_choice(dict(res["crossover_ms"], **res["beyond_ms"]))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
