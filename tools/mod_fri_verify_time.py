#!/usr/bin/env python3
"""Time of the batch FRI verifier over other moduli (GPU box): device time of sh_dev_mod_fri_verify on 512 proofs of one shape at
n = 2^14, 2^16 and 2^20 (maxdeg_plus_1 = n / 8, exclude_multiples_of = 8, 40 samples) over BN254, Goldilocks and the MiMC prime, and in
the same run sh_dev_fri_verify (the MiMC verifier) on the same MiMC batch as the yardstick, sh_dev_mod_fri_prove at the same shape
(the proving rate the verifier must stay above) and sh_mod_fri_verify on one host core.
The 512 proofs are CHUNK[lg] distinct ones proved on the device by sh_dev_mod_fri_prove (seeded coefficients of degree below n / 8)
and repeated: a verifier's work does not depend on which valid proof it reads.  Their roots come from sh_dev_merkelize_plain over
sh_dev_mod_ntt's evaluations.  Every status must be SH_OK, or the tool fails.  HIP events around REPS calls after a warm-up of every
shape, the smallest of ROUNDS windows, the paths alternating round by round.
Prints one JSON line and writes it to argv[1] (default profiles/r14_mod_fri_verify.json).  `--trace` instead runs the generic and the
MiMC verifier three times each on the 512 x 2^16 MiMC batch in a child process under `rocprofv3 --kernel-trace --stats` and copies the
verifiers' rows of its kernel statistics to profiles/r14_mod_fri_verify_kernel_stats.csv: the index-set and branch kernels are shared,
so the cost over the MiMC verifier sits in mv_fri_rows_kernel / mv_final_kernel against vb_fri_rows_kernel / vb_final_kernel."""
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
# name -> (modulus, 2-adicity, a base whose (p - 1) / 2^adicity-th power has full order): tests/modntt_cases.py
FIELDS = {
    "bn254": (21888242871839275222246405745257275088548364400416034343698204186575808495617, 28, 5),
    "goldilocks": (2**64 - 2**32 + 1, 32, 7),
    "mimc": (MIMC_P, 32, 3),
}
LOGS = [14, 16, 20]
CHUNK = {14: 64, 16: 16, 20: 2}  # distinct proofs per shape
PROOFS, ROUNDS, EXCLUDE, SAMPLES = 512, 5, 8, 40


def ck(rc, where):
    _lib.check(rc, where)


def root(name, n):
    p, v, base = FIELDS[name]
    return pow(pow(base, (p - 1) >> v, p), (1 << v) // n, p)


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


class Batch(object):
    """PROOFS proofs of one shape over one modulus on the device, with their roots"""

    def __init__(self, L, ctx, name, lg):
        self.L, self.ctx, self.name, self.n = L, ctx, name, 1 << lg
        n, k, md = self.n, CHUNK[lg], self.n // 8
        self.md, self.k, self.p, self.w = md, k, b32(FIELDS[name][0]), b32(root(name, n))
        self.plen = L.sh_fri_proof_len(n, md, SAMPLES)
        self.coeffs = alloc(L, ctx, 32 * md * k)
        ck(L.sh_dev_fill_seeded(ctx, self.coeffs, md * k, 7 + lg), "fill")  # values below the MiMC prime, any of them may be >= p
        self.proofs, self.roots, self.status = alloc(L, ctx, self.plen * PROOFS), alloc(L, ctx, 32 * PROOFS), alloc(L, ctx, 4 * PROOFS)
        self.prove()
        # the committed roots: the trees over the evaluations of the zero-padded coefficients
        vals, nodes = alloc(L, ctx, 32 * n * k), alloc(L, ctx, 64 * n * k)
        ck(L.sh_dev_upload(ctx, bytes(32 * n * k), vals, 32 * n * k), "upload")
        for b in range(k):
            ck(L.sh_dev_copy(ctx, at(self.coeffs, 32 * md * b), at(vals, 32 * n * b), 32 * md), "copy")
        ck(L.sh_dev_mod_ntt(ctx, self.p, vals, vals, n, k, self.w, 0), "sh_dev_mod_ntt")
        ck(L.sh_dev_merkelize_plain(ctx, vals, n, k, nodes), "sh_dev_merkelize_plain")
        for b in range(k):
            ck(L.sh_dev_copy(ctx, at(nodes, 64 * n * b + 32), at(self.roots, 32 * b), 32), "copy")
        have = k
        while have < PROOFS:  # repeat the chunk up to PROOFS
            m = min(have, PROOFS - have)
            ck(L.sh_dev_copy(ctx, self.proofs, at(self.proofs, self.plen * have), self.plen * m), "copy")
            ck(L.sh_dev_copy(ctx, self.roots, at(self.roots, 32 * have), 32 * m), "copy")
            have += m
        ck(L.sh_sync(ctx), "sync")
        for p in (vals, nodes):
            L.sh_dev_free(ctx, p)

    def prove(self):
        ck(self.L.sh_dev_mod_fri_prove(self.ctx, self.p, self.coeffs, self.md, self.n, self.w, self.md, EXCLUDE, SAMPLES, self.k,
                                       self.proofs), "sh_dev_mod_fri_prove")

    def verify(self):
        ck(self.L.sh_dev_mod_fri_verify(self.ctx, self.p, self.proofs, self.roots, self.n, self.w, self.md, EXCLUDE, SAMPLES, PROOFS,
                                        self.status), "sh_dev_mod_fri_verify")

    def verify_mimc(self):
        ck(self.L.sh_dev_fri_verify(self.ctx, self.proofs, self.roots, self.n, self.w, self.md, EXCLUDE, SAMPLES, PROOFS, self.status),
           "sh_dev_fri_verify")

    def all_accepted(self):
        st = (ctypes.c_int32 * PROOFS)()
        ck(self.L.sh_dev_download(self.ctx, self.status, st, 4 * PROOFS), "download")
        return all(s == 0 for s in st)

    def host_ms(self, reps=5):
        """sh_mod_fri_verify on proof 0, one host core: the median of `reps` calls"""
        flat, mroot = ctypes.create_string_buffer(self.plen), ctypes.create_string_buffer(32)
        ck(self.L.sh_dev_download(self.ctx, self.proofs, flat, self.plen), "download")
        ck(self.L.sh_dev_download(self.ctx, self.roots, mroot, 32), "download")
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            rc = self.L.sh_mod_fri_verify(self.p, flat.raw, self.plen, mroot.raw, self.n, self.w, self.md, EXCLUDE, SAMPLES)
            ts.append(1e3 * (time.perf_counter() - t0))
            if rc != 0:
                raise SystemExit("the host verifier rejects a proof of %s at n = %d: %d" % (self.name, self.n, rc))
        return sorted(ts)[len(ts) // 2]

    def free(self):
        for p in (self.coeffs, self.proofs, self.roots, self.status):
            self.L.sh_dev_free(self.ctx, p)


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    res = {"tool": "tools/mod_fri_verify_time.py", "proofs": PROOFS, "rounds": ROUNDS, "maxdeg_plus_1": "n / 8", "exclude_multiples_of": EXCLUDE,
           "samples": SAMPLES, "distinct_proofs": {"2^%d" % lg: k for lg, k in CHUNK.items()},
           "stat": "min over rounds of (HIP-event ms of `reps` calls) / reps, after a warm-up; paths alternate per round; host: median "
                   "wall-clock ms of sh_mod_fri_verify on one proof, one core",
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
                raise SystemExit("%s rejects an honest proof at n = 2^%d" % (k, lg))
        ck(L.sh_sync(ctx), "sync")
        best = {}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t = window(L, ctx, fn, reps[k])
                best[k] = min(best.get(k, t), t)
        row = {"ms_per_call": best, "host_ms_per_proof": {name: b.host_ms() for name, b in batches.items()}}
        row["verify_proofs_per_s"] = {k[:-7]: PROOFS / best[k] * 1e3 for k in best if k.endswith("_verify")}
        row["prove_proofs_per_s"] = {name: CHUNK[lg] / best[name + "_prove"] * 1e3 for name in FIELDS}
        row["verify_over_prove_rate"] = {name: row["verify_proofs_per_s"][name] / row["prove_proofs_per_s"][name] for name in FIELDS}
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


def trace():
    out_dir = tempfile.mkdtemp(prefix="mod_fri_verify_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod_fri_verify", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r14_mod_fri_verify_kernel_stats.csv")
        with open(stats[0]) as src, open(dst, "w") as out:
            for i, line in enumerate(src):  # the header and the verifiers' kernels (the prover's made the batch)
                if i == 0 or "vb_" in line or "mv_" in line:
                    out.write(line)
        print("wrote", dst)
        print(open(dst).read())
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    if "--trace" in sys.argv:
        return trace()
    if "--once" in sys.argv:
        return once()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r14_mod_fri_verify.json")
    line = json.dumps(measure())
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
