#!/usr/bin/env python3
"""Time of the witness generator over other moduli (GPU box): device time of sh_dev_mod_stark_witness on
  * the width-2 cubic (MiMC) system X1' = X1, X2' = X2^3 + X1 at 2^16 steps for 1, 64 and 512 units (2 counted products per step, one
    lane per unit), and
  * the 256-term width-9 system of tests/golden/stark_variants.json (w9_256_terms) at 2^12 steps for 5 units (56 counted products per
    step on the longest of 16 lanes, the exchange included: witness_items.cuh),
over BN254, Goldilocks and the MiMC prime, beside sh_dev_stark_witness (the tuned MiMC-prime kernel) on the same systems in the same run.
HIP events around one call after a warm-up of every shape (term image, code objects), the smallest of ROUNDS rounds, the paths
alternating round by round.  The same is measured in a child process under STARKHIP_WITNESS_STORE=inline (the knob is read once per
process): the conversion on the kernel's store path instead of in a closing pass.
Per shape and path: ms, `us_per_product` = ms / ((steps - 1) * counted products per step) -- what MWI_SLICE_PRODUCTS
(csrc/modwitness_items.cuh) is sized by -- and `ratio_to_tuned` = ms / the tuned kernel's ms in the same run.  Reported, not gated.
Prints one JSON line and writes it to argv[1] (default profiles/r17_mod_witness.json).  `--child` prints one store form's numbers."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from starks_amd import _lib, stark  # noqa: E402

MIMC_P = 2**256 - 2**32 * 351 + 1
FIELDS = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "goldilocks": 2**64 - 2**32 + 1,
    "mimc": MIMC_P,
}
ROUNDS = 5
MIMC = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]


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


def shapes():
    import stark_variants as sv
    with open(os.path.join(ROOT, "tests", "golden", "stark_variants.json")) as fh:
        c = [x for x in json.load(fh)["cases"] if x["name"] == "w9_256_terms"][0]
    out = [("mimc_w2:%dx2^16" % u, MIMC, 1 << 16, [[2 + b, 5 + b] for b in range(u)], 2) for u in (1, 64, 512)]
    out.append(("w9_256_terms:5x2^12", sv.step_polys(c), 1 << 12, [sv.unit_inputs(c, u) for u in range(5)], 56))
    return out


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    res = {}
    for key, sp, steps, inputs, products in shapes():
        width, units = len(sp), len(inputs)
        nbytes = 32 * width * units * steps
        dg, dt, di = alloc(L, ctx, nbytes), alloc(L, ctx, nbytes), alloc(L, ctx, 32 * width * units)
        fns = {}
        for name, p in FIELDS.items():
            coefs, exps, counts, _ = stark.pack_step_polys([_Poly(d) for d in sp], width, p=p)

            def generic(pb=b32(p), coefs=coefs, exps=exps, counts=counts):
                ck(L.sh_dev_mod_stark_witness(ctx, pb, di, steps, width, coefs, exps, counts, units, dg), "sh_dev_mod_stark_witness")
            fns[name] = generic
        tcoefs, texps, tcounts, _ = stark.pack_step_polys([_Poly(d) for d in sp], width)
        fns["tuned"] = lambda: ck(L.sh_dev_stark_witness(ctx, di, steps, width, tcoefs, texps, tcounts, units, dt), "sh_dev_stark_witness")
        limbs = b"".join(int(v % MIMC_P).to_bytes(32, "little") for u in inputs for v in u)  # plain limbs: valid inputs of both entries
        ck(L.sh_dev_upload(ctx, limbs, di, len(limbs)), "upload")
        for fn in fns.values():  # warm-up
            fn()
        ck(L.sh_sync(ctx), "sync")
        # dg holds the MiMC-prime trace of the generic entry, dt the tuned one: the same bytes (canonical limbs)
        a, b = ctypes.create_string_buffer(32 * width * steps), ctypes.create_string_buffer(32 * width * steps)
        ck(L.sh_dev_download(ctx, dg, a, len(a)), "download")
        ck(L.sh_dev_download(ctx, dt, b, len(b)), "download")
        assert a.raw == b.raw, key
        best = {}
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                t = once(L, ctx, fn)
                best[name] = min(best.get(name, t), t)
        res[key] = {"steps": steps, "units": units, "products_per_step": products, "ms": {k: round(v, 3) for k, v in best.items()},
                    "us_per_product": {k: round(1000.0 * v / ((steps - 1) * products), 3) for k, v in best.items()},
                    "ratio_to_tuned": {k: round(v / best["tuned"], 3) for k, v in best.items() if k != "tuned"}}
        print("%s %s: %s" % (os.environ.get("STARKHIP_WITNESS_STORE", "pass"), key, res[key]["ms"]), file=sys.stderr, flush=True)
        ck(L.sh_sync(ctx), "sync")
        for ptr in (dg, dt, di):
            L.sh_dev_free(ctx, ptr)
    return res


def main():
    if "--child" in sys.argv:
        print(json.dumps(measure()))
        return
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r17_mod_witness.json")
    out = {"tool": "tools/mod_witness_time.py", "rounds": ROUNDS, "lib": os.path.basename(_lib.LIB_PATH),
           "stat": "min over rounds of the HIP-event ms of one call, after a warm-up; paths alternate per round",
           "store": {}}
    for form in ("pass", "inline"):
        env = dict(os.environ)
        for k in ("STARKHIP_WITNESS_GROUP", "STARKHIP_WITNESS_SLICE"):
            env.pop(k, None)
        env["STARKHIP_WITNESS_STORE"] = form
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], stdout=subprocess.PIPE, text=True, env=env, timeout=900)
        if r.returncode != 0:
            raise SystemExit("child failed (%d)" % r.returncode)
        out["store"][form] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(out, sort_keys=True)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
