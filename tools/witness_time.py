#!/usr/bin/env python3
"""Device witness generation (GPU box), HIP events after a warm-up, every comparison in one process:
  * MiMC (x <- x^3 + k, width 2), 2^16 steps, 32 / 64 / 512 units: sh_dev_stark_witness against sh_dev_fill_mimc_units;
  * the w9_256_terms system of tests/golden/stark_variants.json, 2^12 steps, 5 units: the default group against
    STARKHIP_WITNESS_GROUP=1, each in a child process of its own (the knob is read once per process);
  * VGPRs and scratch of every width instance of witness_kernel (hipcc -Rpass-analysis=kernel-resource-usage).
Prints one JSON line and writes it to argv[1] when given.  `--child` runs the w9 timing alone (used by the parent)."""
import ctypes, json, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from starks_amd import _lib, stark  # noqa: E402

REPS = 3
MIMC = [{(1, 0): 1}, {(1, 0): 1, (0, 3): 1}]


class _Poly(object):
    def __init__(self, d):
        self.coefficients = d


def ck(rc, where):
    _lib.check(rc, where)


def timed(L, ctx, fn):
    fn()  # warm-up: terms upload, code objects
    ck(L.sh_sync(ctx), "sync")
    best = None
    for _ in range(REPS):
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


def w9_ms():
    import stark_variants as sv
    L, ctx = _lib.lib(), _lib.ctx()
    c = [x for x in json.load(open(os.path.join(ROOT, "tests", "golden", "stark_variants.json")))["cases"] if x["name"] == "w9_256_terms"][0]
    steps, units = 1 << 12, 5
    coefs, exps, counts, _ = stark.pack_step_polys([_Poly(d) for d in sv.step_polys(c)], 9)
    di, dw = alloc(L, ctx, 32 * 9 * units), alloc(L, ctx, 32 * 9 * units * steps)
    ck(L.sh_dev_from_wire(ctx, b"".join(b"".join(v.to_bytes(32, "big") for v in sv.unit_inputs(c, u)) for u in range(units)), di, 9 * units),
       "up")
    ms = timed(L, ctx, lambda: ck(L.sh_dev_stark_witness(ctx, di, steps, 9, coefs, exps, counts, units, dw), "witness"))
    for p in (di, dw):
        L.sh_dev_free(ctx, p)
    return ms


def resources():
    out = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-std=c++17", "-c",
                          os.path.join(ROOT, "starks_amd", "csrc", "witness.hip"), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True)
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: \S*witness_kernelILi(\d+)E", line)
        if m:
            cur = "W=" + m.group(1)
            res[cur] = {}
        elif cur and "VGPRs:" in line and "AGPR" not in line:
            res[cur]["vgprs"] = int(line.split()[-2])
        elif cur and "ScratchSize" in line:
            res[cur]["scratch_bytes"] = int(line.split()[-2])
    return res


def main():
    if "--child" in sys.argv:
        print(json.dumps({"ms": w9_ms()}))
        return
    L, ctx = _lib.lib(), _lib.ctx()
    steps = 1 << 16
    coefs, exps, counts, _ = stark.pack_step_polys([_Poly(d) for d in MIMC], 2)
    out = {"what": "device witness generation, best of %d after a warm-up (HIP events)" % REPS, "mimc_2p16": {}}
    for units in (32, 64, 512):
        dw, dg, di = alloc(L, ctx, 64 * steps * units), alloc(L, ctx, 64 * steps * units), alloc(L, ctx, 64 * units)
        fill = timed(L, ctx, lambda: ck(L.sh_dev_fill_mimc_units(ctx, dw, di, steps, 0, units, 42), "fill"))
        gen = timed(L, ctx, lambda: ck(L.sh_dev_stark_witness(ctx, di, steps, 2, coefs, exps, counts, units, dg), "witness"))
        a, b = ctypes.create_string_buffer(64 * steps), ctypes.create_string_buffer(64 * steps)
        ck(L.sh_dev_download(ctx, dw, a, len(a)), "dl")
        ck(L.sh_dev_download(ctx, dg, b, len(b)), "dl")
        assert a.raw == b.raw
        out["mimc_2p16"][str(units)] = {"fill_mimc_units_ms": round(fill, 3), "stark_witness_ms": round(gen, 3),
                                        "ratio": round(gen / fill, 3)}
        for p in (dw, dg, di):
            L.sh_dev_free(ctx, p)
    w9 = {}
    for name, env in (("default_group", {}), ("group_1", {"STARKHIP_WITNESS_GROUP": "1"})):
        e = dict(os.environ)
        e.pop("STARKHIP_WITNESS_GROUP", None)
        e.update(env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=e, timeout=600)
        if r.returncode != 0:
            raise SystemExit("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        w9[name + "_ms"] = round(json.loads(r.stdout.strip().splitlines()[-1])["ms"], 3)
    w9["speedup"] = round(w9["group_1_ms"] / w9["default_group_ms"], 2)
    out["w9_256_terms_2p12_5_units"] = w9
    out["kernel_resources"] = resources()
    line = json.dumps(out, sort_keys=True)
    print(line)
    if len(sys.argv) > 1 and not sys.argv[1].startswith("--"):
        with open(sys.argv[1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
