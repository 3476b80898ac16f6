#!/usr/bin/env python3
"""Time of the FRI commit on packed 64-bit words (GPU box): device time of sh_dev_mod64_fri_prove against sh_dev_mod_fri_prove (the
generic 32-byte commit, the yardstick) over Goldilocks and BabyBear IN THE SAME RUN, on the same seeded values -- word form for one,
limb form for the other --, at n = 2^14, 2^16, 2^20 and 8 x 2^16 (maxdeg_plus_1 = n / 8, exclude_multiples_of = 8, n coefficients per
polynomial), and each path's forward transform alone beside it (sh_dev_mod64_ntt, sh_dev_mod_ntt), so that the (commit - transform)
figures -- the trees, the fold, the sampling, the gather -- can be compared.  HIP events around REPS calls after a warm-up of every shape
(tables, workspaces, code objects), the smallest of ROUNDS windows, the paths alternating round by round.  Before timing, the two
proofs of every shape are downloaded once and compared.  Nothing is gated: the ratios are reported.  Prints one JSON line and writes it
to argv[1] (default profiles/r18_mod64_fri.json).  `--trace` instead runs the 2^20 Goldilocks commits twice each in a child process under
`rocprofv3 --kernel-trace --stats` and copies its kernel statistics to profiles/r18_mod64_fri_kernel_stats.csv."""
import ctypes
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import _lib  # noqa: E402

# name -> (modulus, 2-adicity, a base whose (p - 1) / 2^adicity-th power has full order): tests/ntt64_cases.py
FIELDS = {
    "goldilocks": (2**64 - 2**32 + 1, 32, 7),
    "babybear": (2**31 - 2**27 + 1, 27, 11),
}
SHAPES = [(14, 1), (16, 1), (20, 1), (16, 8)]
ROUNDS = 5
EXCLUDE, SAMPLES = 8, 40


def reps_for(lg, batch):
    return max(4, min(32, (1 << 22) // (batch << lg)))


def ck(rc, where):
    _lib.check(rc, where)


def root(name, n):
    p, v, base = FIELDS[name]
    return pow(pow(base, (p - 1) >> v, p), (1 << v) // n, p)


def b32(x):
    return int(x).to_bytes(32, "big")


def window(L, ctx, fn, reps):
    ck(L.sh_timer_start(ctx), "timer")
    for _ in range(reps):
        fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value / reps


class Buffers(object):
    """seed: `count` seeded 256-bit values; words / limbs: the same values modulo p in word form and in limb form; yw / yl: transform
    outputs; pw / pl: the two proofs"""

    def __init__(self, L, ctx, count, proof_bytes):
        self.L, self.ctx, self.count = L, ctx, count
        self.all = []
        self.seed, self.limbs, self.yl = (self._alloc(32 * count) for _ in range(3))
        self.words, self.yw = (self._alloc(8 * count) for _ in range(2))
        self.pw, self.pl = (self._alloc(proof_bytes) for _ in range(2))
        ck(L.sh_dev_fill_seeded(ctx, self.seed, count, 1), "fill")

    def _alloc(self, nbytes):
        p = ctypes.c_void_p()
        ck(self.L.sh_dev_alloc(self.ctx, nbytes, ctypes.byref(p)), "alloc")
        self.all.append(p)
        return p

    def reduce(self, p):
        ck(self.L.sh_dev_mod64_from_limbs(self.ctx, p, self.seed, self.words, self.count), "sh_dev_mod64_from_limbs")
        ck(self.L.sh_dev_mod64_to_limbs(self.ctx, self.words, self.limbs, self.count), "sh_dev_mod64_to_limbs")

    def free(self):
        for p in self.all:
            self.L.sh_dev_free(self.ctx, p)


def calls(L, ctx, name, B, n, batch):
    """packed commit, packed transform, generic commit, generic transform over FIELDS[name]"""
    md, p, w = n // 8, FIELDS[name][0], root(name, n)
    pb, wb = b32(p), b32(w)
    return {
        name + "_packed_commit": lambda: ck(L.sh_dev_mod64_fri_prove(ctx, p, B.words, n, n, w, md, EXCLUDE, SAMPLES, batch, B.pw),
                                            "sh_dev_mod64_fri_prove"),
        name + "_packed_ntt": lambda: ck(L.sh_dev_mod64_ntt(ctx, p, B.words, n, B.yw, n, batch, w, 0), "sh_dev_mod64_ntt"),
        name + "_generic_commit": lambda: ck(L.sh_dev_mod_fri_prove(ctx, pb, B.limbs, n, n, wb, md, EXCLUDE, SAMPLES, batch, B.pl),
                                             "sh_dev_mod_fri_prove"),
        name + "_generic_ntt": lambda: ck(L.sh_dev_mod_ntt(ctx, pb, B.limbs, B.yl, n, batch, wb, 0), "sh_dev_mod_ntt"),
    }


def digest(L, ctx, ptr, nbytes):
    out = ctypes.create_string_buffer(nbytes)
    ck(L.sh_dev_download(ctx, ptr, out, nbytes), "download")
    return hashlib.sha256(out.raw).hexdigest()


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    big = max(batch << lg for lg, batch in SHAPES)
    plen = max(batch * L.sh_fri_proof_len(1 << lg, (1 << lg) // 8, SAMPLES) for lg, batch in SHAPES)
    B = Buffers(L, ctx, big, plen)
    res = {"tool": "tools/mod64_fri_time.py", "rounds": ROUNDS, "maxdeg_plus_1": "n / 8", "exclude_multiples_of": EXCLUDE, "samples": SAMPLES,
           "stat": "min over rounds of (HIP-event ms of `reps` calls) / reps, after a warm-up; paths alternate per round; "
                   "n coefficients per polynomial on every path; both paths of a field in one run on the same values",
           "shapes": {}}
    for lg, batch in SHAPES:
        n, reps = 1 << lg, reps_for(lg, batch)
        row = {"reps": reps, "ms": {}, "commit_less_transform_ms": {}, "packed_over_generic": {}, "proofs_equal": {}}
        for name in FIELDS:
            B.reduce(FIELDS[name][0])
            fns = calls(L, ctx, name, B, n, batch)
            for fn in fns.values():  # warm-up
                fn()
            nbytes = batch * L.sh_fri_proof_len(n, n // 8, SAMPLES)
            row["proofs_equal"][name] = digest(L, ctx, B.pw, nbytes) == digest(L, ctx, B.pl, nbytes)
            best = {}
            for _ in range(ROUNDS):
                for k, fn in fns.items():
                    t = window(L, ctx, fn, reps)
                    best[k] = min(best.get(k, t), t)
            row["ms"].update(best)
            pk = best[name + "_packed_commit"] - best[name + "_packed_ntt"]
            gn = best[name + "_generic_commit"] - best[name + "_generic_ntt"]
            row["commit_less_transform_ms"][name] = {"packed": pk, "generic": gn}
            row["packed_over_generic"][name] = {"commit": best[name + "_packed_commit"] / best[name + "_generic_commit"],
                                                "transform": best[name + "_packed_ntt"] / best[name + "_generic_ntt"],
                                                "commit_less_transform": pk / gn}
        res["shapes"]["%dx2^%d" % (batch, lg)] = row
    ck(L.sh_sync(ctx), "sync")
    B.free()
    ck(L.sh_ctx_trim(ctx), "trim")
    return res


def once():
    L, ctx = _lib.lib(), _lib.ctx()
    n = 1 << 20
    B = Buffers(L, ctx, n, L.sh_fri_proof_len(n, n // 8, SAMPLES))
    B.reduce(FIELDS["goldilocks"][0])
    fns = calls(L, ctx, "goldilocks", B, n, 1)
    for k in ("goldilocks_packed_commit", "goldilocks_generic_commit"):
        fns[k]()
        fns[k]()
    ck(L.sh_sync(ctx), "sync")


def trace():
    out_dir = tempfile.mkdtemp(prefix="mod64_fri_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod64_fri", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=900)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r18_mod64_fri_kernel_stats.csv")
        shutil.copyfile(stats[0], dst)
        print("wrote", dst)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    if "--trace" in sys.argv:
        return trace()
    if "--once" in sys.argv:
        return once()
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r18_mod64_fri.json")
    line = json.dumps(measure())
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
