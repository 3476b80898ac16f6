#!/usr/bin/env python3
"""Time of the batch STARK verifier over other moduli (GPU box): device time of sh_dev_mod_stark_verify on 512 proofs of one shape --
width 2, the cubic MiMC step (X1' = X1, X2' = X1 + X2^3), ext 8, 80 spot checks -- at 2^12 and 2^16 steps over BN254, Goldilocks and
the MiMC prime, and in the same run (b) sh_dev_stark_verify (the MiMC verifier) on the MiMC batch of the same shape as the yardstick,
(c) sh_dev_mod_stark_prove at the same shape (the proving rate the verifier must stay above) and (d) sh_mod_stark_verify on one host
core.
The 512 proofs are one proof, proved on the device by sh_dev_mod_stark_prove from a witness generated on the host, and replicated on
the device: a verifier's work does not depend on which valid proof it reads.  Every status must be SH_OK, or the tool fails.  HIP
events around REPS calls after a warm-up of every path, the smallest of ROUNDS windows, the paths alternating round by round.
Prints one JSON line and writes it to argv[1] (default profiles/r16_mod_stark_verify.json).  `--trace [CSV]` instead runs the generic
and the MiMC verifier three times each on the 512 x 2^16 MiMC batch in a child process under `rocprofv3 --kernel-trace --stats` and
copies the verifiers' rows of its kernel statistics to CSV (default profiles/r16_mod_stark_verify_kernel_stats.csv): the index-set and
branch kernels are shared, so the cost over the MiMC verifier sits in mv_spot_kernel / mv_fri_rows_kernel / mv_final_kernel against
their vb_ counterparts."""
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import _lib  # noqa: E402

MIMC_P = 2**256 - 2**32 * 351 + 1
FIELDS = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "goldilocks": 2**64 - 2**32 + 1,
    "mimc": MIMC_P,
}
LOGS = [12, 16]
PROOFS, ROUNDS, EXT, WIDTH, DEGREE, SAMPLES = 512, 5, 8, 2, 3, 80
INPUTS = [2, 5]


def ck(rc, where):
    _lib.check(rc, where)


def b32(x):
    return int(x).to_bytes(32, "big")


def at(ptr, off):
    return ctypes.c_void_p(ptr.value + off)


def alloc(L, ctx, nbytes):
    p = ctypes.c_void_p()
    ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(p)), "alloc")
    return p


def window(L, ctx, fn, reps):
    ck(L.sh_timer_start(ctx), "timer")
    for _ in range(reps):
        fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value / reps


def terms():
    """X1' = X1; X2' = X2^3 + X1, in sorted monomial order"""
    coefs = b32(1) * 3
    exps = bytes([1, 0, 0, 3, 1, 0])
    return coefs, exps, (ctypes.c_uint32 * 2)(1, 2)


def witness_of(p, steps):
    a, b = INPUTS
    col = [b]
    for _ in range(steps - 1):
        b = (a + b * b * b) % p
        col.append(b)
    return [[a] * steps, col]


def limbs(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def replicate(L, ctx, ptr, unit, count):
    have = 1
    while have < count:
        m = min(have, count - have)
        ck(L.sh_dev_copy(ctx, ptr, at(ptr, unit * have), unit * m), "copy")
        have += m


class Batch(object):
    """PROOFS copies of one proof over one modulus on the device, with their inputs and outputs"""

    def __init__(self, L, ctx, name, lg):
        self.L, self.ctx, self.name, self.steps = L, ctx, name, 1 << lg
        self.p_int, self.p = FIELDS[name], b32(FIELDS[name])
        self.terms = terms()
        steps = self.steps
        w = witness_of(self.p_int, steps)
        self.outs = [col[-1] for col in w]
        self.plen = L.sh_stark_proof_len(steps, EXT, WIDTH, DEGREE, SAMPLES)
        self.wit, self.inp = alloc(L, ctx, 32 * WIDTH * steps), alloc(L, ctx, 32 * WIDTH * PROOFS)
        self.out = alloc(L, ctx, 32 * WIDTH * PROOFS)
        self.proofs, self.status = alloc(L, ctx, self.plen * PROOFS), alloc(L, ctx, 4 * PROOFS)
        raw = limbs([v for col in w for v in col])
        ck(L.sh_dev_upload(ctx, raw, self.wit, len(raw)), "upload")
        ck(L.sh_dev_upload(ctx, limbs(INPUTS), self.inp, 32 * WIDTH), "upload")
        ck(L.sh_dev_upload(ctx, limbs(self.outs), self.out, 32 * WIDTH), "upload")
        self.prove()
        if L.sh_stark_status(ctx) != 0:
            raise SystemExit("the prover calls the host's witness over %s invalid" % name)
        for ptr, unit in ((self.proofs, self.plen), (self.inp, 32 * WIDTH), (self.out, 32 * WIDTH)):
            replicate(L, ctx, ptr, unit, PROOFS)
        if name == "mimc":  # the MiMC verifier's inputs and outputs in its own limb form
            self.inp_m, self.out_m = alloc(L, ctx, 32 * WIDTH * PROOFS), alloc(L, ctx, 32 * WIDTH * PROOFS)
            ck(L.sh_dev_from_wire(ctx, b"".join(b32(v) for v in INPUTS) * PROOFS, self.inp_m, WIDTH * PROOFS), "from_wire")
            ck(L.sh_dev_from_wire(ctx, b"".join(b32(v) for v in self.outs) * PROOFS, self.out_m, WIDTH * PROOFS), "from_wire")
        ck(L.sh_sync(ctx), "sync")

    def prove(self):
        ck(self.L.sh_dev_mod_stark_prove(self.ctx, self.p, self.wit, self.inp, self.steps, EXT, WIDTH, *self.terms, SAMPLES, 1, self.proofs),
           "sh_dev_mod_stark_prove")

    def verify(self):
        ck(self.L.sh_dev_mod_stark_verify(self.ctx, self.p, self.proofs, self.inp, self.out, 1, self.steps, EXT, WIDTH, *self.terms, SAMPLES,
                                          PROOFS, self.status), "sh_dev_mod_stark_verify")

    def verify_mimc(self):
        ck(self.L.sh_dev_stark_verify(self.ctx, self.proofs, self.inp_m, self.out_m, 1, self.steps, EXT, WIDTH, *self.terms, SAMPLES, PROOFS,
                                      self.status), "sh_dev_stark_verify")

    def all_accepted(self):
        st = (ctypes.c_int32 * PROOFS)()
        ck(self.L.sh_dev_download(self.ctx, self.status, st, 4 * PROOFS), "download")
        return all(s == 0 for s in st)

    def host_ms(self, reps=5):
        """sh_mod_stark_verify on proof 0, one host core: the median of `reps` calls"""
        flat = ctypes.create_string_buffer(self.plen)
        ck(self.L.sh_dev_download(self.ctx, self.proofs, flat, self.plen), "download")
        inb, outb = b"".join(b32(v) for v in INPUTS), b"".join(b32(v) for v in self.outs)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            rc = self.L.sh_mod_stark_verify(self.p, flat.raw, self.plen, inb, outb, self.steps, EXT, WIDTH, *self.terms, SAMPLES)
            ts.append(1e3 * (time.perf_counter() - t0))
            if rc != 0:
                raise SystemExit("the host verifier rejects a proof of %s at %d steps: %d" % (self.name, self.steps, rc))
        return sorted(ts)[len(ts) // 2]

    def free(self):
        for p in (self.wit, self.inp, self.out, self.proofs, self.status) + ((self.inp_m, self.out_m) if self.name == "mimc" else ()):
            self.L.sh_dev_free(self.ctx, p)


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    res = {"tool": "tools/mod_stark_verify_time.py", "proofs": PROOFS, "rounds": ROUNDS, "ext": EXT, "width": WIDTH, "degree": DEGREE,
           "samples": SAMPLES,
           "stat": "min over rounds of (HIP-event ms of `reps` calls) / reps, after a warm-up; paths alternate per round; prove: one "
                   "proof per call; host: median wall-clock ms of sh_mod_stark_verify on one proof, one core",
           "shapes": {}}
    for lg in LOGS:
        batches = {name: Batch(L, ctx, name, lg) for name in FIELDS}
        fns = {}
        for name, b in batches.items():
            fns[name + "_verify"], fns[name + "_prove"] = b.verify, b.prove
        fns["mimc_tuned_verify"] = batches["mimc"].verify_mimc
        reps = {k: (4 if k.endswith("_prove") else 8) for k in fns}
        for k, fn in fns.items():  # warm-up, and every proof of every batch must be accepted
            fn()
            if k.endswith("_verify") and not batches[k.split("_")[0]].all_accepted():
                raise SystemExit("%s rejects an honest proof at 2^%d steps" % (k, lg))
        ck(L.sh_sync(ctx), "sync")
        best = {}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                fn()  # untimed: a change of modulus uploads the term image again (one synchronisation and a blocking copy)
                t = window(L, ctx, fn, reps[k])
                best[k] = min(best.get(k, t), t)
        row = {"ms_per_call": best, "host_ms_per_proof": {name: b.host_ms() for name, b in batches.items()}}
        row["verify_proofs_per_s"] = {k[:-7]: PROOFS / best[k] * 1e3 for k in best if k.endswith("_verify")}
        row["prove_ms_per_proof"] = {name: best[name + "_prove"] for name in FIELDS}
        row["verify_over_prove_rate"] = {name: row["verify_proofs_per_s"][name] * best[name + "_prove"] / 1e3 for name in FIELDS}
        row["ratio_to_mimc_verifier"] = {name: best[name + "_verify"] / best["mimc_tuned_verify"] for name in FIELDS}
        row["device_over_one_host_core"] = {name: row["host_ms_per_proof"][name] * PROOFS / best[name + "_verify"] for name in FIELDS}
        res["shapes"]["%dx2^%d" % (PROOFS, lg)] = row
        for b in batches.values():
            b.free()
    ck(L.sh_ctx_trim(ctx), "trim")
    return res


def once():
    L, ctx = _lib.lib(), _lib.ctx()
    b = Batch(L, ctx, "mimc", 16)
    for _ in range(3):
        b.verify()
        b.verify_mimc()
    ck(L.sh_sync(ctx), "sync")
    if not b.all_accepted():
        raise SystemExit("an honest proof was rejected")


def trace(dst):
    out_dir = tempfile.mkdtemp(prefix="mod_stark_verify_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod_stark_verify", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        with open(stats[0]) as src, open(dst, "w") as out:
            for i, line in enumerate(src):  # the header and the verifiers' kernels (the prover's made the batch)
                if i == 0 or "vb_" in line or "mv_" in line:
                    out.write(line)
        print("wrote", dst)
        print(open(dst).read())
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--trace" in sys.argv:
        return trace(args[0] if args else os.path.join(ROOT, "profiles", "r16_mod_stark_verify_kernel_stats.csv"))
    if "--once" in sys.argv:
        return once()
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r16_mod_stark_verify.json")
    line = json.dumps(measure())
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
