#!/usr/bin/env python3
"""Time of the STARK prover over other moduli (GPU box): device time of sh_dev_mod_stark_prove on device-resident witnesses of the
width-2 cubic system (X1' = X1, X2' = X2^3 + X1; ext 8, 80 spot checks) over BN254 at 2^12, 2^16 and 2^20 steps and 64 x 2^12 steps,
and over Goldilocks and the MiMC prime at 2^16 steps; in the same run sh_dev_stark_prove (the tuned MiMC prover) on the same shapes,
and the transforms of a proof alone on both paths (the steps-point inverse, the short-input forward transform onto steps * ext points,
the steps-point forward transform of X P'(X)).  Witnesses are valid traces over their own modulus, generated on the device from the
inputs (sh_dev_stark_witness for the tuned path, sh_dev_mod_stark_witness for the generic one).  HIP events around REPS calls after a warm-up of every shape (tables, workspaces,
code objects), the smallest of ROUNDS windows, the paths alternating round by round.
`proof_ratio_to_tuned` = generic proof / tuned proof; `middle_ratio` = (generic proof - generic transforms) / (tuned proof - tuned
transforms): what the quotients, the trees, the combination, the gather and the commit rounds cost over p beside the tuned ones.
The generic transforms are timed with a FULL-SIZE n-point extension (sh_dev_mod_ntt has no short-input form), the tuned ones with the
short-input sh_dev_lde the prover runs: the generic middle and `middle_ratio` are therefore LOWER bounds.  Reported, not gated.  Prints
one JSON line and writes it to argv[1] (default profiles/r15_mod_stark.json).  `--trace` instead runs the 2^16-step BN254 and tuned
proofs four times each in a child process under `rocprofv3 --kernel-trace --stats` and copies its kernel statistics to
profiles/r15_mod_stark_kernel_stats.csv."""
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from starks_amd import _lib  # noqa: E402

MIMC_P = 2**256 - 2**32 * 351 + 1
FIELDS = {
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "goldilocks": 2**64 - 2**32 + 1,
    "mimc": MIMC_P,
}
# (field, log2 steps, batch)
SHAPES = [("bn254", 12, 1), ("bn254", 16, 1), ("bn254", 20, 1), ("bn254", 12, 64), ("goldilocks", 16, 1), ("mimc", 16, 1)]
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


def setup(L, ctx, name, lg, batch):
    """-> ({path name: call}, the device buffers to free) for one shape"""
    coefs = b"".join(b32(c) for _, c in TERMS)
    exps = b"".join(bytes(k) for k, _ in TERMS)
    counts = (ctypes.c_uint32 * WIDTH)(*COUNTS)
    p, steps = FIELDS[name], 1 << lg
    n, cols = steps * EXT, batch * WIDTH
    plen = L.sh_stark_proof_len(steps, EXT, WIDTH, 3, SAMPLES)
    bufs = [ctypes.c_void_p() for _ in range(7)]
    wg, ig, wm, im, proof, q, pe = bufs
    for ptr, nbytes in ((wg, 32 * cols * steps), (ig, 32 * cols), (wm, 32 * cols * steps), (im, 32 * cols), (proof, plen * batch),
                        (q, 32 * cols * steps), (pe, 32 * cols * n)):
        ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)), "alloc")
    # the generic path's witness over p, the tuned path's over the MiMC prime
    inputs = b"".join(int(v).to_bytes(32, "little") for b in range(batch) for v in (2 + b, 5 + b))
    ck(L.sh_dev_upload(ctx, inputs, ig, len(inputs)), "upload")
    ck(L.sh_dev_upload(ctx, inputs, im, len(inputs)), "upload")
    ck(L.sh_dev_mod_stark_witness(ctx, b32(p), ig, steps, WIDTH, coefs, exps, counts, batch, wg), "sh_dev_mod_stark_witness")
    ck(L.sh_dev_stark_witness(ctx, im, steps, WIDTH, coefs, exps, counts, batch, wm), "sh_dev_stark_witness")
    g2p = pow(7, (p - 1) // n, p)
    g2m = pow(7, (MIMC_P - 1) // n, MIMC_P)
    pb, g2pb, g1pb = b32(p), b32(g2p), b32(pow(g2p, EXT, p))
    g2mb, g1mb = b32(g2m), b32(pow(g2m, EXT, MIMC_P))
    ck(L.sh_dev_fill_seeded(ctx, q, cols * steps, 2), "fill")
    ck(L.sh_dev_fill_seeded(ctx, pe, cols * n, 1), "fill")

    def generic():
        ck(L.sh_dev_mod_stark_prove(ctx, pb, wg, ig, steps, EXT, WIDTH, coefs, exps, counts, SAMPLES, batch, proof), "sh_dev_mod_stark_prove")

    def tuned():
        ck(L.sh_dev_stark_prove(ctx, wm, im, steps, EXT, WIDTH, coefs, exps, counts, SAMPLES, batch, proof), "sh_dev_stark_prove")

    def generic_ntts():
        ck(L.sh_dev_mod_ntt(ctx, pb, wg, q, steps, cols, g1pb, 1), "sh_dev_mod_ntt")
        ck(L.sh_dev_mod_ntt(ctx, pb, q, q, steps, cols, g1pb, 0), "sh_dev_mod_ntt")
        # the extension as a FULL-SIZE transform of whatever pe holds (the time does not depend on the values): the public entry has no
        # short-input form, so this is an upper bound of the prover's short-input first pass
        ck(L.sh_dev_mod_ntt(ctx, pb, pe, pe, n, cols, g2pb, 0), "sh_dev_mod_ntt")

    def tuned_ntts():
        # the inverse over G1 and the short-input transform over G2, on whatever q holds (sh_dev_lde overwrites its input)
        ck(L.sh_dev_lde(ctx, q, pe, steps, EXT, cols, g2mb), "sh_dev_lde")
        ck(L.sh_dev_ntt(ctx, q, q, steps, cols, g1mb, 0), "sh_dev_ntt")

    return {"generic_proof": generic, "tuned_proof": tuned, "generic_transforms": generic_ntts, "tuned_transforms": tuned_ntts}, bufs


def measure():
    L, ctx = _lib.lib(), _lib.ctx()
    res = {"tool": "tools/mod_stark_time.py", "rounds": ROUNDS, "ext": EXT, "width": WIDTH, "samples": SAMPLES, "step": "X1' = X1, X2' = X2^3 + X1",
           "stat": "min over rounds of (HIP-event ms of `reps` calls) / reps, after a warm-up; paths alternate per round",
           "note": "generic_transforms times the extension as a full-size n-point transform (the public entry has no short-input form), "
                   "tuned_transforms the short-input one the prover runs: middle_ms.generic and middle_ratio are LOWER bounds",
           "lib": os.path.basename(_lib.LIB_PATH), "shapes": {}}
    for name, lg, batch in SHAPES:
        reps = reps_for(lg, batch)
        fns, bufs = setup(L, ctx, name, lg, batch)
        for fn in fns.values():  # warm-up
            fn()
        ck(L.sh_stark_status(ctx), "sh_stark_status")  # both witnesses are valid traces
        best = {}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                t = window(L, ctx, fn, reps)
                best[k] = min(best.get(k, t), t)
        ck(L.sh_stark_status(ctx), "sh_stark_status")
        mid_g, mid_t = best["generic_proof"] - best["generic_transforms"], best["tuned_proof"] - best["tuned_transforms"]
        res["shapes"]["%s:%dx2^%d" % (name, batch, lg)] = {
            "reps": reps, "ms": best, "proof_ratio_to_tuned": best["generic_proof"] / best["tuned_proof"],
            "middle_ms": {"generic": mid_g, "tuned": mid_t}, "middle_ratio": mid_g / mid_t if mid_t > 0 else None}
        ck(L.sh_sync(ctx), "sync")
        for ptr in bufs:
            L.sh_dev_free(ctx, ptr)
        ck(L.sh_ctx_trim(ctx), "trim")
    return res


def once():
    """what --trace runs in its child: the BN254 and the tuned proof of 2^16 steps, three times each after one warm-up call"""
    L, ctx = _lib.lib(), _lib.ctx()
    fns, bufs = setup(L, ctx, "bn254", 16, 1)
    for key in ("generic_proof", "tuned_proof"):
        for _ in range(4):
            fns[key]()
    ck(L.sh_stark_status(ctx), "sh_stark_status")
    for ptr in bufs:
        L.sh_dev_free(ctx, ptr)


def trace():
    out_dir = tempfile.mkdtemp(prefix="mod_stark_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "mod_stark", "--",
               sys.executable, os.path.abspath(__file__), "--once"]
        subprocess.run(cmd, check=True, timeout=600)
        stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv under %s" % out_dir)
        dst = os.path.join(ROOT, "profiles", "r15_mod_stark_kernel_stats.csv")
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
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "r15_mod_stark.json")
    line = json.dumps(measure())
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
