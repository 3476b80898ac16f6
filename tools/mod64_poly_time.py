#!/usr/bin/env python3
"""Time of the polynomial entries on packed 64-bit words against their 32-byte twins (GPU box).

HIP-event device time of whole sh_dev_mod64_* calls beside the sh_dev_mod_* call on the SAME values (the words zero-extended to
limbs by sh_dev_mod64_to_limbs) in the same run: after one warm-up of both (tables, code objects, workspaces) the two alternate
for ROUNDS rounds; per side the median, the smallest and the largest round are kept.  `ratio` = packed median / generic median: the
condition is ratio <= 1 at every shape.  Each row also carries the transform yardstick, sh_dev_mod64_ntt : sh_dev_mod_ntt at the
operation's dominant transform size, measured the same way.

Shapes (profiles/r21_mod_poly.json's sizes, the inversions larger), over Goldilocks:
  mul          2^20 x 2^20 coefficients (transform 2^21)        divmod       2^20 by 2^19 (transform 2^21)
  zpoly        2^20 points (transforms up to 2^20)              lagrange     2^20 points (transforms up to 2^21)
  multi_inv    2^24 values                                      multi_interp_4  2^22 rows
and over BabyBear: mul and multi_inv.

usage: mod64_poly_time.py [DST [SHAPE ...]]     SHAPE = goldilocks:mul, babybear:multi_inv, ...; none: all of them
One process per invocation, so a job can give every shape a time limit of its own; the rows of an invocation are merged into DST
(default profiles/r23_mod64_poly.json) by (modulus, op).  Prints the rows as one JSON line."""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import _lib  # noqa: E402

MODULI = {"goldilocks": 2**64 - 2**32 + 1, "babybear": 15 * 2**27 + 1}
ALL = ["goldilocks:mul", "goldilocks:divmod", "goldilocks:zpoly", "goldilocks:lagrange", "goldilocks:multi_inv",
       "goldilocks:multi_interp_4", "babybear:mul", "babybear:multi_inv"]
ROUNDS = 7
CAP = 1 << 24  # words per buffer


def ck(rc, where):
    _lib.check(rc, where)


def once(L, ctx, fn):
    ck(L.sh_timer_start(ctx), "timer")
    fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value


def pair(L, ctx, packed, generic):
    """(packed, generic) statistics over ROUNDS alternating rounds after one warm-up of both"""
    packed()
    generic()
    ck(L.sh_sync(ctx), "sync")
    t = ([], [])
    for _ in range(ROUNDS):
        t[0].append(once(L, ctx, packed))
        t[1].append(once(L, ctx, generic))
    return [{"median_ms": round(statistics.median(x), 4), "min_ms": round(min(x), 4), "max_ms": round(max(x), 4)} for x in t]


def run(L, ctx, shapes):
    import numpy as np
    W, G = [], []  # packed and generic buffers: A, B, O1, O2
    for _ in range(4):
        for lst, size in ((W, 8), (G, 32)):
            p = ctypes.c_void_p()
            ck(L.sh_dev_alloc(ctx, size * CAP, ctypes.byref(p)), "sh_dev_alloc")
            lst.append(p)
    rng = np.random.default_rng(23)
    for k in (0, 1):  # random 64-bit words, and the same values as limbs
        raw = rng.integers(0, 2**64, size=CAP, dtype=np.uint64).tobytes()
        ck(L.sh_dev_upload(ctx, raw, W[k], len(raw)), "sh_dev_upload")
        ck(L.sh_dev_mod64_to_limbs(ctx, W[k], G[k], CAP), "sh_dev_mod64_to_limbs")
    ck(L.sh_sync(ctx), "sync")
    out = []
    for shape in shapes:
        name, op = shape.split(":")
        p = MODULI[name]
        m, w, k = _lib.mod64_poly_args(p)
        gm, gw, gk = _lib.mod_poly_args(p)
        n20, n19 = 1 << 20, 1 << 19
        A, B, O1, O2 = W
        a, b, o1, o2 = G
        calls = {
            "mul": (n20, 2 * n20, lambda: L.sh_dev_mod64_poly_mul(ctx, m, w, k, A, n20, B, n20, O1),
                    lambda: L.sh_dev_mod_poly_mul(ctx, gm, gw, gk, a, n20, b, n20, o1)),
            "divmod": (n20, 2 * n20, lambda: L.sh_dev_mod64_poly_divmod(ctx, m, w, k, A, n20, B, n19, O1, O2),
                       lambda: L.sh_dev_mod_poly_divmod(ctx, gm, gw, gk, a, n20, b, n19, o1, o2)),
            "zpoly": (n20, n20, lambda: L.sh_dev_mod64_zpoly(ctx, m, w, k, A, n20, O1), lambda: L.sh_dev_mod_zpoly(ctx, gm, gw, gk, a, n20, o1)),
            "lagrange": (n20, 2 * n20, lambda: L.sh_dev_mod64_lagrange_interp(ctx, m, w, k, A, B, n20, O1),
                         lambda: L.sh_dev_mod_lagrange_interp(ctx, gm, gw, gk, a, b, n20, o1)),
            "multi_inv": (1 << 24, 0, lambda: L.sh_dev_mod64_multi_inv(ctx, m, A, O1, 1 << 24),
                          lambda: L.sh_dev_mod_multi_inv(ctx, gm, a, o1, 1 << 24)),
            "multi_interp_4": (1 << 22, 0, lambda: L.sh_dev_mod64_multi_interp_4(ctx, m, A, B, 1 << 22, O1),
                               lambda: L.sh_dev_mod_multi_interp_4(ctx, gm, a, b, 1 << 22, o1)),
        }
        n, dominant, packed, generic = calls[op]
        s64, s32 = pair(L, ctx, lambda: ck(packed(), "sh_dev_mod64_* " + op), lambda: ck(generic(), "sh_dev_mod_* " + op))
        rec = {"modulus": name, "op": op, "n": n, "packed": s64, "generic": s32, "ratio": round(s64["median_ms"] / s32["median_ms"], 4)}
        if dominant:
            lg = dominant.bit_length() - 1
            wr = pow(w, 1 << (k - lg), p)
            t64, t32 = pair(L, ctx, lambda: ck(L.sh_dev_mod64_ntt(ctx, m, A, dominant, O1, dominant, 1, wr, 0), "sh_dev_mod64_ntt"),
                            lambda: ck(L.sh_dev_mod_ntt(ctx, gm, a, o1, dominant, 1, wr.to_bytes(32, "big"), 0), "sh_dev_mod_ntt"))
            rec["ntt"] = {"size_log": lg, "packed": t64, "generic": t32, "ratio": round(t64["median_ms"] / t32["median_ms"], 4)}
        out.append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    for p in W + G:
        L.sh_dev_free(ctx, p)
    ck(L.sh_ctx_trim(ctx), "trim")
    return out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_mod64_poly.json")
    shapes = sys.argv[2:] or ALL
    for s in shapes:
        if s not in ALL:
            sys.exit("unknown shape " + s)
    rows = run(_lib.lib(), _lib.ctx(), shapes)
    res = {"tool": "tools/mod64_poly_time.py", "rounds": ROUNDS, "device": []}
    if os.path.exists(dst):
        with open(dst) as fh:
            res["device"] = json.load(fh).get("device", [])
    keys = {(r["modulus"], r["op"]) for r in rows}
    res["device"] = [r for r in res["device"] if (r["modulus"], r["op"]) not in keys] + rows
    with open(dst, "w") as fh:
        fh.write(json.dumps(res) + "\n")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
