#!/usr/bin/env python3
"""Time of the packed-word witness generator (GPU box): device time of
  (a) sh_dev_mod64_stark_witness, and
  (b) the route to the same words without it: sh_dev_mod_stark_witness plus the two sh_dev_mod64_from_limbs calls (witness and inputs),
in the same run, on
  * the width-2 cubic (MiMC) system X1' = X1, X2' = X2^3 + X1 at 2^16 steps for 1, 64 and 512 units (2 counted products per step, one
    lane per unit) over Goldilocks, and for 1 unit over BIG18 = 2^64 - 1835007 as well,
  * the 256-term width-9 system of tests/golden/stark_variants.json (w9_256_terms) at 2^12 steps for 5 units over Goldilocks (56 counted
    products per step on the longest of 16 lanes, the exchange included: witness_items.cuh), and
  * the whole packed chain generate -> sh_dev_mod64_stark_prove at 2^16 steps x 64 units, ext 8, over Goldilocks, both ways.
HIP events around the calls after a warm-up of every shape (term images, code objects), the smallest of ROUNDS rounds, the routes
alternating round by round.  Everything is measured in one child process per store form (STARKHIP_WITNESS_STORE=pass / inline: the knob
is read once per process), and (a) on the 256-term system in one more child per store form and forced group 1, 2, 4, 8, 16
(STARKHIP_WITNESS_GROUP).  One process has the GPU open at a time.
Per shape and route: ms, `us_per_product` = ms / ((steps - 1) * counted products per step) -- what M6W_SLICE_PRODUCTS
(csrc/mod64witness_items.cuh) is sized by -- and `ratio_b_over_a`.  Reported, not gated.
Prints one JSON line and writes it to argv[1] (default profiles/r20_mod64_witness.json).  `--child full|w9` prints one child's numbers."""
import ctypes
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from starks_amd import _lib, stark  # noqa: E402

GOLDILOCKS = 2**64 - 2**32 + 1
BIG18 = 2**64 - 1835007
ROUNDS = 5
MIMC = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]
CHAIN = (1 << 16, 8, 64)  # steps, ext, units


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


def ck(rc, where):
    _lib.check(rc, where)


def b32(x):
    return int(x).to_bytes(32, "big")


def once(L, ctx, fn):
    ck(L.sh_timer_start(ctx), "timer")
    fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value


def alloc(L, ctx, nbytes):
    p = ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(p)), "sh_dev_alloc")
    return p


def w9_system():
    import stark_variants as sv
    with open(os.path.join(ROOT, "tests", "golden", "stark_variants.json")) as fh:
        c = [x for x in json.load(fh)["cases"] if x["name"] == "w9_256_terms"][0]
    return sv.step_polys(c), [sv.unit_inputs(c, u) for u in range(5)]


def shapes(which):
    sp9, in9 = w9_system()
    w9 = ("w9_256_terms:5x2^12", GOLDILOCKS, sp9, 1 << 12, in9, 56)
    if which == "w9":
        return [w9]
    out = [("mimc_w2:%dx2^16" % u, GOLDILOCKS, MIMC, 1 << 16, [[2 + b, 5 + b] for b in range(u)], 2) for u in (1, 64, 512)]
    out.insert(1, ("mimc_w2:1x2^16:big18", BIG18, MIMC, 1 << 16, [[2, 5]], 2))
    return out + [w9]


class Routes(object):
    """the buffers and the two routes of one shape: a() leaves words in self.wa, b() in self.wb"""

    def __init__(self, L, ctx, p, sp, steps, inputs):
        self.L, self.ctx, self.p, self.steps = L, ctx, p, steps
        self.width, self.units = len(sp), len(inputs)
        self.cols = self.width * self.units
        self.coefs, self.exps, self.counts, self.degree = stark.pack_step_polys([_Poly(d) for d in sp], self.width, p=p)
        vals = [v % p for u in inputs for v in u]
        self.iw, self.il = alloc(L, ctx, 8 * self.cols), alloc(L, ctx, 32 * self.cols)
        self.wa, self.wb = alloc(L, ctx, 8 * self.cols * steps), alloc(L, ctx, 8 * self.cols * steps)
        self.wl, self.iwb = alloc(L, ctx, 32 * self.cols * steps), alloc(L, ctx, 8 * self.cols)
        words = struct.pack("<%dQ" % len(vals), *vals)
        limbs = b"".join(v.to_bytes(32, "little") for v in vals)
        ck(L.sh_dev_upload(ctx, words, self.iw, len(words)), "upload")
        ck(L.sh_dev_upload(ctx, limbs, self.il, len(limbs)), "upload")

    def a(self):
        ck(self.L.sh_dev_mod64_stark_witness(self.ctx, self.p, self.iw, self.steps, self.width, self.coefs, self.exps, self.counts,
                                             self.units, self.wa), "sh_dev_mod64_stark_witness")

    def b(self):
        L, ctx = self.L, self.ctx
        ck(L.sh_dev_mod_stark_witness(ctx, b32(self.p), self.il, self.steps, self.width, self.coefs, self.exps, self.counts, self.units,
                                      self.wl), "sh_dev_mod_stark_witness")
        ck(L.sh_dev_mod64_from_limbs(ctx, self.p, self.wl, self.wb, self.cols * self.steps), "sh_dev_mod64_from_limbs")
        ck(L.sh_dev_mod64_from_limbs(ctx, self.p, self.il, self.iwb, self.cols), "sh_dev_mod64_from_limbs")

    def same_words(self):
        n = 8 * self.cols * self.steps
        x, y = ctypes.create_string_buffer(n), ctypes.create_string_buffer(n)
        ck(self.L.sh_dev_download(self.ctx, self.wa, x, n), "download")
        ck(self.L.sh_dev_download(self.ctx, self.wb, y, n), "download")
        return x.raw == y.raw

    def free(self):
        ck(self.L.sh_sync(self.ctx), "sync")
        for ptr in (self.iw, self.il, self.wa, self.wb, self.wl, self.iwb):
            self.L.sh_dev_free(self.ctx, ptr)


def best_of(L, ctx, fns):
    for fn in fns.values():  # warm-up
        fn()
    ck(L.sh_sync(ctx), "sync")
    best = {}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            t = once(L, ctx, fn)
            best[name] = min(best.get(name, t), t)
    return best


def measure(which):
    L, ctx = _lib.lib(), _lib.ctx()
    tag = "%s g=%s" % (os.environ.get("STARKHIP_WITNESS_STORE", "pass"), os.environ.get("STARKHIP_WITNESS_GROUP", "default"))
    res = {}
    for key, p, sp, steps, inputs, products in shapes(which):
        r = Routes(L, ctx, p, sp, steps, inputs)
        fns = {"a": r.a} if which == "w9" else {"a": r.a, "b": r.b}
        best = best_of(L, ctx, fns)
        if which != "w9":
            assert r.same_words(), key
        res[key] = {"modulus": p, "steps": steps, "units": r.units, "products_per_step": products, "ms": {k: round(v, 4) for k, v in best.items()}}
        if which != "w9":  # a forced group has its own product count: only ms there
            res[key]["us_per_product"] = {k: round(1000.0 * v / ((steps - 1) * products), 4) for k, v in best.items()}
            res[key]["ratio_b_over_a"] = round(best["b"] / best["a"], 2)
        print("%s %s: %s" % (tag, key, res[key]["ms"]), file=sys.stderr, flush=True)
        r.free()
    if which == "full":
        steps, ext, units = CHAIN
        r = Routes(L, ctx, GOLDILOCKS, MIMC, steps, [[2 + b, 5 + b] for b in range(units)])
        plen = stark.proof_len(steps, ext, 2, r.degree)
        dp = alloc(L, ctx, plen * units)

        def prove(wit, inp):
            ck(L.sh_dev_mod64_stark_prove(ctx, GOLDILOCKS, wit, inp, steps, ext, 2, r.coefs, r.exps, r.counts, 80, units, dp),
               "sh_dev_mod64_stark_prove")

        def chain_a():
            r.a()
            prove(r.wa, r.iw)

        def chain_b():
            r.b()
            prove(r.wb, r.iwb)
        best = best_of(L, ctx, {"a": chain_a, "b": chain_b, "prove_only": lambda: prove(r.wa, r.iw)})
        ck(L.sh_stark_status(ctx), "sh_stark_status")
        res["chain:mimc_w2:64x2^16:ext8"] = {"modulus": GOLDILOCKS, "steps": steps, "ext": ext, "units": units,
                                            "ms": {k: round(v, 4) for k, v in best.items()}, "ratio_b_over_a": round(best["b"] / best["a"], 2)}
        print("%s chain: %s" % (tag, best), file=sys.stderr, flush=True)
        r.free()
        L.sh_dev_free(ctx, dp)
    return res


def child(which, form, group):
    env = dict(os.environ)
    for k in ("STARKHIP_WITNESS_GROUP", "STARKHIP_WITNESS_SLICE"):
        env.pop(k, None)
    env["STARKHIP_WITNESS_STORE"] = form
    if group:
        env["STARKHIP_WITNESS_GROUP"] = str(group)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which], stdout=subprocess.PIPE, text=True, env=env, timeout=400)
    if r.returncode != 0:  # nothing more is started on the GPU after a child that failed
        raise SystemExit("child %s %s %s failed (%d)" % (which, form, group, r.returncode))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    if "--child" in sys.argv:
        print(json.dumps(measure(sys.argv[sys.argv.index("--child") + 1])))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r20_mod64_witness.json")
    out = {"tool": "tools/mod64_witness_time.py", "rounds": ROUNDS, "lib": os.path.basename(_lib.LIB_PATH),
           "stat": "min over rounds of the HIP-event ms of the route's calls, after a warm-up; routes alternate per round",
           "routes": {"a": "sh_dev_mod64_stark_witness", "b": "sh_dev_mod_stark_witness + 2 x sh_dev_mod64_from_limbs"},
           "not_measured": "moduli other than Goldilocks and BIG18; widths other than 2 and 9; route (b) under forced groups; "
                           "forced slices; host forms (copies included)",
           "store": {}, "w9_groups_ms": {}}
    for form in ("pass", "inline"):
        out["store"][form] = child("full", form, 0)
        out["w9_groups_ms"][form] = {"default": out["store"][form]["w9_256_terms:5x2^12"]["ms"]["a"]}
        for g in (1, 2, 4, 8, 16):
            out["w9_groups_ms"][form][str(g)] = child("w9", form, g)["w9_256_terms:5x2^12"]["ms"]["a"]
    line = json.dumps(out, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
