#!/usr/bin/env python3
"""Time of the polynomial entries over a run-time modulus (GPU box), two parts, one process.

"device": HIP-event device time of whole sh_dev_mod_* calls, the smallest of ROUNDS rounds after a warm-up of every shape (tables,
code objects, workspaces), beside the MiMC entry of the same shape and, as the yardstick, sh_dev_mod_ntt / sh_dev_ntt at the
operation's dominant transform size, all in the same run:
  * over BN254 at n = 2^16 and 2^20: product (n x n coefficients, transform 2n), divmod (2n by n, transform 4n), zpoly and
    lagrange_interp (n points, transforms up to n and 2n), multi_inv (n values), multi_interp_4 (n rows); the product also at 2^23;
  * over Goldilocks through the same code at 2^16.
Per shape: mod_ms, mimc_ms, `ratio` = mod_ms / mimc_ms, and `ntt_ratio` of the dominant size.  Reported, not gated.

"routing": wall-clock time, end to end, of the Python call sites over IntegersModP(BN254) on the same inputs in the same run -- the
device call (explicit form behind Polynomial / poly_utils: wire conversion, upload, call, download, WireList) against the host loop --
at powers of two from 4 up, the host loop measured until one call exceeds HOST_CAP_S.  `threshold` of an operation = the smallest
measured power of two from which the device call wins at every larger measured size; the MOD_DEVICE_MIN constants of
starks_amd/polynomial.py and poly_utils.py cite it.

Prints one JSON line and writes it to argv[1] (default profiles/r21_mod_poly.json)."""
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import IntegersModP, _lib, poly_utils, polynomial  # noqa: E402

BN254 = 21888242871839275222246405745257275088548364400416034343698204186575808495617
GOLDILOCKS = 2**64 - 2**32 + 1
MIMC_P = _lib.MIMC_P
ROUNDS = 5
HOST_CAP_S = 1.5


def ck(rc, where):
    _lib.check(rc, where)


def once(L, ctx, fn):
    ck(L.sh_timer_start(ctx), "timer")
    fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value


def best(L, ctx, fns):
    """the smallest of ROUNDS rounds of each fn after one warm-up, the fns alternating round by round"""
    for fn in fns:
        fn()
    ck(L.sh_sync(ctx), "sync")
    res = [float("inf")] * len(fns)
    for _ in range(ROUNDS):
        for i, fn in enumerate(fns):
            res[i] = min(res[i], once(L, ctx, fn))
    return res


def device_part(L, ctx):
    cap = 1 << 25
    bufs = []
    for _ in range(4):
        p = ctypes.c_void_p()
        ck(L.sh_dev_alloc(ctx, 32 * cap, ctypes.byref(p)), "sh_dev_alloc")
        bufs.append(p)
    A, B, O1, O2 = bufs
    ck(L.sh_dev_fill_seeded(ctx, A, cap, 1), "fill")   # values below the MiMC prime: plain 256-bit inputs for every modulus
    ck(L.sh_dev_fill_seeded(ctx, B, cap, 2), "fill")
    out = []

    def shapes(p, lgs, with_big):
        m, w, k = _lib.mod_poly_args(p)
        w_int = int.from_bytes(w, "big")

        def ntt_ratio(size):
            lg = size.bit_length() - 1
            wm = pow(w_int, 1 << (k - lg), p).to_bytes(32, "big")
            wq = pow(7, (MIMC_P - 1) >> lg, MIMC_P).to_bytes(32, "big")
            a, b = best(L, ctx, [lambda: ck(L.sh_dev_mod_ntt(ctx, m, A, O1, size, 1, wm, 0), "sh_dev_mod_ntt"),
                                 lambda: ck(L.sh_dev_ntt(ctx, A, O2, size, 1, wq, 0), "sh_dev_ntt")])
            return {"size_log": lg, "mod_ms": round(a, 4), "mimc_ms": round(b, 4), "ratio": round(a / b, 3)}

        def row(op, lg, mod_fn, mimc_fn, dominant):
            a, b = best(L, ctx, [lambda: ck(mod_fn(), op), lambda: ck(mimc_fn(), op)])
            rec = {"modulus": "bn254" if p == BN254 else "goldilocks", "op": op, "log_n": lg, "mod_ms": round(a, 4), "mimc_ms": round(b, 4),
                   "ratio": round(a / b, 3)}
            if dominant:
                rec["ntt"] = ntt_ratio(dominant)
            out.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)

        for lg in lgs:
            n = 1 << lg
            row("poly_mul", lg, lambda: L.sh_dev_mod_poly_mul(ctx, m, w, k, A, n, B, n, O1), lambda: L.sh_dev_poly_mul(ctx, A, n, B, n, O1), 2 * n)
            row("poly_divmod", lg, lambda: L.sh_dev_mod_poly_divmod(ctx, m, w, k, A, 2 * n, B, n, O1, O2),
                lambda: L.sh_dev_poly_divmod(ctx, A, 2 * n, B, n, O1, O2), 4 * n)
            row("zpoly", lg, lambda: L.sh_dev_mod_zpoly(ctx, m, w, k, A, n, O1), lambda: L.sh_dev_zpoly(ctx, A, n, O1), n)
            row("lagrange_interp", lg, lambda: L.sh_dev_mod_lagrange_interp(ctx, m, w, k, A, B, n, O1),
                lambda: L.sh_dev_lagrange_interp(ctx, A, B, n, O1), 2 * n)
            row("multi_inv", lg, lambda: L.sh_dev_mod_multi_inv(ctx, m, A, O1, n), lambda: L.sh_dev_multi_inv(ctx, A, O1, n), 0)
            row("multi_interp_4", lg, lambda: L.sh_dev_mod_multi_interp_4(ctx, m, A, B, n, O1), lambda: L.sh_dev_multi_interp_4(ctx, A, B, n, O1), 0)
        if with_big:
            n = 1 << 23
            row("poly_mul", 23, lambda: L.sh_dev_mod_poly_mul(ctx, m, w, k, A, n, B, n, O1), lambda: L.sh_dev_poly_mul(ctx, A, n, B, n, O1), 2 * n)

    shapes(BN254, [16, 20], True)
    shapes(GOLDILOCKS, [16], False)
    for p in bufs:
        L.sh_dev_free(ctx, p)
    ck(L.sh_ctx_trim(ctx), "trim")
    return out


def wall(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def routing_part():
    p = BN254
    F = IntegersModP(p)
    Poly = polynomial.polynomials_over(F)
    rnd = random.Random(1)
    W = lambda v: _lib.to_wire(v, p)  # noqa: E731
    WL = polynomial.WireList

    def dev_mul(a, b):
        return Poly(WL(polynomial.mod_mul_wire(p, W(a.coefficients), W(b.coefficients)), F))

    def dev_divmod(a, b):
        q, r = polynomial.mod_divmod_wire(p, W(a.coefficients), W(b.coefficients))
        return Poly(WL(q, F)), Poly(WL(r, F))

    ops = {
        "mul": (lambda n: (Poly([rnd.randrange(p) for _ in range(n)]), Poly([rnd.randrange(p) for _ in range(n)])),
                dev_mul, lambda a, b: a._schoolbook(b)),
        "divmod": (lambda n: (Poly([rnd.randrange(p) for _ in range(2 * n)]), Poly([rnd.randrange(p) for _ in range(n)])),
                   dev_divmod, None),
        "zpoly": (lambda n: ([F(rnd.randrange(p)) for _ in range(n)],),
                  lambda xs: Poly(WL(poly_utils.mod_zpoly_wire(p, W(xs)), F)), lambda xs: Poly(poly_utils._host_zpoly(F, list(xs)))),
        "lagrange_interp": (lambda n: ([F(rnd.randrange(p)) for _ in range(n)], [F(rnd.randrange(p)) for _ in range(n)]),
                            lambda xs, ys: Poly(WL(poly_utils.mod_lagrange_interp_wire(p, W(xs), W(ys)), F)),
                            lambda xs, ys: poly_utils._host_lagrange_interp(F, xs, ys)),
        "multi_inv": (lambda n: ([F(rnd.randrange(p)) for _ in range(n)],),
                      lambda v: WL(poly_utils.mod_multi_inv_wire(p, W(v)), F), lambda v: poly_utils._host_multi_inv(F, list(v))),
        "multi_interp_4": (lambda n: ([[F(rnd.randrange(p)) for _ in range(4)] for _ in range(n)],
                                      [[F(rnd.randrange(p)) for _ in range(4)] for _ in range(n)]),
                           lambda xs, ys: WL(poly_utils.mod_multi_interp_4_wire(p, b"".join(W(r) for r in xs), b"".join(W(r) for r in ys), len(xs)), F),
                           lambda xs, ys: poly_utils._host_multi_interp_4(F, xs, ys)),
    }
    saved = dict(polynomial.MOD_DEVICE_MIN), dict(poly_utils.MOD_DEVICE_MIN)
    for d in (polynomial.MOD_DEVICE_MIN, poly_utils.MOD_DEVICE_MIN):
        for key in d:
            d[key] = None  # the host loops below must not route
    out = {}
    try:
        for name, (make, dev, host) in ops.items():
            if host is None:  # divmod: the class's own loop with routing off
                host = lambda a, b: divmod(a, b)  # noqa: E731
            rows, host_on = [], True
            for lg in range(2, 15):
                n = 1 << lg
                args = make(n)
                dev(*args)  # warm-up: tables of this size
                td = min(wall(lambda: dev(*args)) for _ in range(3))
                th = None
                if host_on:
                    th = min(wall(lambda: host(*args)) for _ in range(2 if n <= 64 else 1))
                    host_on = th < HOST_CAP_S
                rows.append({"n": n, "device_ms": round(1e3 * td, 3), "host_ms": None if th is None else round(1e3 * th, 3)})
                if not host_on and n >= 256:
                    break
            thr = None
            for r in reversed(rows):
                if r["host_ms"] is None or r["device_ms"] < r["host_ms"]:
                    thr = r["n"]
                else:
                    break
            out[name] = {"sizes": rows, "threshold": thr}
            print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    finally:
        polynomial.MOD_DEVICE_MIN.update(saved[0])
        poly_utils.MOD_DEVICE_MIN.update(saved[1])
    return out


def main():
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r21_mod_poly.json")
    L, ctx = _lib.lib(), _lib.ctx()
    res = {"tool": "tools/mod_poly_time.py", "rounds": ROUNDS, "device": device_part(L, ctx), "routing": routing_part()}
    line = json.dumps(res)
    print(line)
    with open(dst, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
