#!/usr/bin/env python3
"""Batch verification of BASELINE config 5 (GPU box): 512 MiMC STARK units of 2^16 steps proved as 2 x 256 (StarkUnitProver), gathered
into one device buffer, then sh_dev_stark_verify on all 512 timed with HIP events after a warm-up call of the same shape; beside it
sh_stark_verify (host, one thread) on a sample of the same proofs.  Prints one JSON line (and writes it to argv[1] when given)."""
import ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from starks_amd import _lib, batch, stark

STEPS, EXT, CHUNK, UNITS, REPS, HOST_SAMPLE = 1 << 16, 8, 256, 512, 5, 16
L, ctx = _lib.lib(), _lib.ctx()


def ck(rc, where):
    _lib.check(rc, where)


pr = batch.StarkUnitProver(STEPS, EXT, CHUNK)
plen, wbytes = pr.plen, 64 * STEPS  # witness bytes per unit: [2][steps] limb form
dp, dw, ds = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
for ptr, nbytes in ((dp, plen * UNITS), (dw, wbytes * UNITS), (ds, 4 * UNITS)):
    ck(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)), "sh_dev_alloc")
for first in range(0, UNITS, CHUNK):
    pr.generate(first, CHUNK)
    pr.prove(CHUNK)
    pr.status()
    ck(L.sh_dev_copy(ctx, pr.dp, ctypes.c_void_p(dp.value + plen * first), plen * CHUNK), "copy proofs")
    ck(L.sh_dev_copy(ctx, pr.dw, ctypes.c_void_p(dw.value + wbytes * first), wbytes * CHUNK), "copy witness")
ck(L.sh_sync(ctx), "sync")
last = ctypes.c_void_p(dw.value + 32 * (STEPS - 1))


def verify():
    ck(L.sh_dev_stark_verify(ctx, dp, dw, last, STEPS, STEPS, EXT, 2, pr.coefs, pr.exps, pr.counts, 80, UNITS, ds), "sh_dev_stark_verify")


verify()  # warm-up: workspaces, step-polynomial terms, code objects
ck(L.sh_sync(ctx), "sync")
times = []
for _ in range(REPS):
    ck(L.sh_timer_start(ctx), "timer")
    verify()
    ms = ctypes.c_float()
    ck(L.sh_timer_stop(ctx, ctypes.byref(ms)), "timer")
    times.append(ms.value)
status = (ctypes.c_int32 * UNITS)()
ck(L.sh_dev_download(ctx, ds, status, 4 * UNITS), "download")
accepted = sum(1 for s in status if s == 0)
# the host verifier on HOST_SAMPLE of the proofs (one thread)
proofs = ctypes.create_string_buffer(plen * HOST_SAMPLE)
ck(L.sh_dev_download(ctx, dp, proofs, plen * HOST_SAMPLE), "download")
host_ms, host_agree = [], 0
for u in range(HOST_SAMPLE):
    w, i = batch.mimc_stark_unit(u, STEPS)
    ib = b"".join(v.to_bytes(32, "big") for v in i)
    ob = b"".join(col[-1].to_bytes(32, "big") for col in w)
    p = proofs.raw[u * plen:(u + 1) * plen]
    t0 = time.perf_counter()
    rc = L.sh_stark_verify(p, plen, ib, ob, STEPS, EXT, 2, pr.coefs, pr.exps, pr.counts, 80)
    host_ms.append(1e3 * (time.perf_counter() - t0))
    host_agree += rc == status[u]
for ptr in (dp, dw, ds):
    L.sh_dev_free(ctx, ptr)
pr.close()
best = min(times)
host = sorted(host_ms)[len(host_ms) // 2]
out = {
    "what": "sh_dev_stark_verify on %d config-5 proofs (2^16 steps, ext 8, width 2, 80 spot checks)" % UNITS,
    "device_ms": [round(t, 4) for t in times], "device_ms_best": round(best, 4),
    "device_proofs_per_s": round(UNITS / best * 1e3), "accepted": accepted,
    "host_ms_per_proof_median": round(host, 3), "host_proofs_per_s_one_core": round(1e3 / host, 1),
    "host_sample": HOST_SAMPLE, "host_statuses_equal": host_agree, "host_cores": os.cpu_count(),
    "speedup_vs_one_core": round(host * UNITS / best, 1),
}
line = json.dumps(out)
print(line)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write(line + "\n")
