#!/usr/bin/env python3
"""Time of the STARK prover on packed 64-bit words (GPU box): device time of sh_dev_mod64_stark_prove against sh_dev_mod_stark_prove (the
generic 32-byte prover, the yardstick) over Goldilocks IN THE SAME RUN, on the same witnesses -- word form for one, limb form for the
other --, of the width-2 cubic system (X1' = X1, X2' = X2^3 + X1; ext 8, 80 spot checks) at 2^12, 2^16 and 2^20 steps and 64 x 2^12
steps, and the transforms of a proof alone on both paths beside it (the steps-point inverse, the forward transform onto steps * ext
points, the steps-point forward transform of X P'(X)), so that the (proof - transforms) figures -- the quotients, the trees, the
combination, the gather and the commit rounds -- can be compared.  Witnesses are valid traces, generated on the device from the inputs
(sh_dev_mod_stark_witness) and converted with sh_dev_mod64_from_limbs.  HIP events around REPS calls after a warm-up of every shape
(tables, workspaces, code objects), the smallest of ROUNDS windows, the paths alternating round by round.  Before timing, the two proofs
of every shape are downloaded once and compared.
The packed transforms run the short-input extension the prover runs (sh_dev_mod64_ntt takes n_in < n); the generic ones a FULL-SIZE
n-point extension (sh_dev_mod_ntt has no short-input form): generic_transforms is an upper bound, the generic (proof - transforms) a
LOWER bound, and `proof_less_transforms` packed / generic an UPPER bound.  Nothing is gated: the ratios are reported.  Prints one JSON
line and writes it to argv[1] (default profiles/r19_mod64_stark.json).  `--trace [csv]` instead runs the 2^16-step proofs four times each
in a child process under `rocprofv3 --kernel-trace --stats` and copies its kernel statistics to the csv (default
profiles/r19_mod64_stark_kernel_stats.csv)."""
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

P = 2**64 - 2**32 + 1  # Goldilocks
SHAPES = [(12, 1), (16, 1), (20, 1), (12, 64)]  # (log2 steps, batch)
EXT, WIDTH, SAMPLES, ROUNDS = 8, 2, 80, 5
TERMS = [((1, 0), 1), ((0, 3), 1), ((1, 0), 1)]  # X1' = X1; X2' = X2^3 + X1 (sorted monomial order per dimension)
COUNTS = [1, 2]


def reps_for(lg, batch):
    return max(3, min(32, (1 << 19) // (batch << lg)))


def ck(rc, where):
    _lib.check(rc, where)


def b32(x):
    return int(x).to_bytes(32, "big")


def window(L, ctx, fn, reps):
    ck(L.sh_timer_start(ctx), "timer")
    for _ in range(reps):
        fn()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    return ms.value / reps


def digest(L, ctx, ptr, nbytes):
    out = ctypes.create_string_buffer(nbytes)
    ck(L.sh_dev_download(ctx, ptr, out, nbytes), "download")
    return hashlib.sha256(out.raw).hexdigest()


def setup(L, ctx, lg, batch):
    """-> ({path name: call}, the two proof buffers, bytes of the proofs, the device buffers to free) for one shape"""
    coefs = b"".join(b32(c) for _, c in TERMS)
    exps = b"".join(bytes(k) for k, _ in TERMS)
    counts = (ctypes.c_uint32 * WIDTH)(*COUNTS)
    steps = 1 << lg
    n, cols = steps * EXT, batch * WIDTH
    plen = L.sh_stark_proof_len(steps, EXT, WIDTH, 3, SAMPLES)
    bufs = [ctypes.c_void_p() for _ in range(10)]
    wg, ig, ww, iw, pg, pw, qg, eg, qw, ew = bufs
    for ptr, nbytes in ((wg, 32 * cols * steps), (ig, 32 * cols), (ww, 8 * cols * steps), (iw, 8 * cols), (pg, plen * batch),
                        (pw, plen * batch), (qg, 32 * cols * steps), (eg, 32 * cols * n), (qw, 8 * cols * steps), (ew, 8 * cols * n)):
        ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)), "alloc")
    inputs = b"".join(int(v).to_bytes(32, "little") for b in range(batch) for v in (2 + b, 5 + b))
    ck(L.sh_dev_upload(ctx, inputs, ig, len(inputs)), "upload")
    pb = b32(P)
    ck(L.sh_dev_mod_stark_witness(ctx, pb, ig, steps, WIDTH, coefs, exps, counts, batch, wg), "sh_dev_mod_stark_witness")
    ck(L.sh_dev_mod64_from_limbs(ctx, P, wg, ww, cols * steps), "sh_dev_mod64_from_limbs")
    ck(L.sh_dev_mod64_from_limbs(ctx, P, ig, iw, cols), "sh_dev_mod64_from_limbs")
    g2 = pow(7, (P - 1) // n, P)
    g1 = pow(g2, EXT, P)
    g2b, g1b = b32(g2), b32(g1)
    ck(L.sh_dev_fill_seeded(ctx, eg, cols * n, 1), "fill")

    def packed():
        ck(L.sh_dev_mod64_stark_prove(ctx, P, ww, iw, steps, EXT, WIDTH, coefs, exps, counts, SAMPLES, batch, pw), "sh_dev_mod64_stark_prove")

    def generic():
        ck(L.sh_dev_mod_stark_prove(ctx, pb, wg, ig, steps, EXT, WIDTH, coefs, exps, counts, SAMPLES, batch, pg), "sh_dev_mod_stark_prove")

    def packed_ntts():  # exactly the prover's three: the extension reads `steps` coefficients per column
        ck(L.sh_dev_mod64_ntt(ctx, P, ww, steps, qw, steps, cols, g1, 1), "sh_dev_mod64_ntt")
        ck(L.sh_dev_mod64_ntt(ctx, P, qw, steps, ew, n, cols, g2, 0), "sh_dev_mod64_ntt")
        ck(L.sh_dev_mod64_ntt(ctx, P, qw, steps, qw, steps, cols, g1, 0), "sh_dev_mod64_ntt")

    def generic_ntts():
        ck(L.sh_dev_mod_ntt(ctx, pb, wg, qg, steps, cols, g1b, 1), "sh_dev_mod_ntt")
        ck(L.sh_dev_mod_ntt(ctx, pb, qg, qg, steps, cols, g1b, 0), "sh_dev_mod_ntt")
        # the extension as a FULL-SIZE transform of whatever eg holds (the time does not depend on the values): the public entry has no
        # short-input form, so this is an upper bound of the prover's short-input first pass
        ck(L.sh_dev_mod_ntt(ctx, pb, eg, eg, n, cols, g2b, 0), "sh_dev_mod_ntt")

    fns = {"packed_proof": packed, "generic_proof": generic, "packed_transforms": packed_ntts, "generic_transforms": generic_ntts}
    return fns, (pw, pg), plen * batch, bufs


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    res = {"tool": "tools/mod64_stark_time.py", "modulus": "goldilocks", "rounds": ROUNDS, "ext": EXT, "width": WIDTH, "samples": SAMPLES,
           "step": "X1' = X1, X2' = X2^3 + X1",
           "stat": "min over rounds of (HIP-event ms of `reps` calls) / reps, after a warm-up; paths alternate per round; both provers in "
                   "one run on the same witnesses",
           "note": "generic_transforms times the extension as a full-size n-point transform (the public entry has no short-input form), "
                   "packed_transforms the short-input one the prover runs: proof_less_transforms_ms.generic is a LOWER bound and "
                   "packed_over_generic.proof_less_transforms an UPPER bound",
           "lib": os.path.basename(_lib.LIB_PATH), "shapes": {}}
    for lg, batch in SHAPES:
        reps = reps_for(lg, batch)
        fns, (pw, pg), nbytes, bufs = setup(L, ctx, lg, batch)
        for fn in fns.values():  # warm-up
            fn()
        ck(L.sh_stark_status(ctx), "sh_stark_status")  # the witnesses are valid traces
        equal = digest(L, ctx, pw, nbytes) == digest(L, ctx, pg, nbytes)
        best = {}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t = window(L, ctx, fn, reps)
                best[k] = min(best.get(k, t), t)
        ck(L.sh_stark_status(ctx), "sh_stark_status")
        mid_p, mid_g = best["packed_proof"] - best["packed_transforms"], best["generic_proof"] - best["generic_transforms"]
        res["shapes"]["%dx2^%d" % (batch, lg)] = {
            "reps": reps, "proofs_equal": equal, "ms": best, "proof_less_transforms_ms": {"packed": mid_p, "generic": mid_g},
            "packed_over_generic": {"proof": best["packed_proof"] / best["generic_proof"],
                                    "transforms": best["packed_transforms"] / best["generic_transforms"],
                                    "proof_less_transforms": mid_p / mid_g if mid_g > 0 else None},
            "generic_over_packed_proof": best["generic_proof"] / best["packed_proof"]}
        ck(L.sh_sync(ctx), "sync")
        for ptr in bufs:
            L.sh_dev_free(ctx, ptr)
        ck(L.sh_ctx_trim(ctx), "trim")
    return res


def once():
    """what --trace runs in its child: the packed and the generic proof of 2^16 steps, three times each after one warm-up call"""
    L, ctx = _lib.lib(), _lib.ctx()
    fns, _, _, bufs = setup(L, ctx, 16, 1)
    for key in ("packed_proof", "generic_proof"):
        for _ in range(4):
            fns[key]()
    ck(L.sh_stark_status(ctx), "sh_stark_status")
    for ptr in bufs:
        L.sh_dev_free(ctx, ptr)


def trace(dst):
    out_dir = tempfile.mkdtemp(prefix="mod64_stark_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod64_stark", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=600)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copyfile(stats[0], dst)
        print("wrote", dst)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--trace" in sys.argv:
        return trace(os.path.abspath(args[0]) if args else os.path.join(ROOT, "profiles", "r19_mod64_stark_kernel_stats.csv"))
    if "--once" in sys.argv:
        return once()
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r19_mod64_stark.json")
    line = json.dumps(measure())
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
