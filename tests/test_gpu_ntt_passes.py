"""Every NTT pass kernel of starks_amd/csrc/ntt.hip on the MI355X, one instantiation at a time, against exact integers.

The harness (tests/native/ntt_ops.hip, built with ntt.hip and kernels.hip alone) runs the whole grid of tests/ntt_cases.py in one
process: every ntt_pass_kernel<LOG_R, LOG_T, LAST> in the code object plain and through the padded XCD grid (67 .. 268 tiles), every
ntt_narrow_pass_kernel with whole and partial tiles, every tile shape over 512 workgroups, and per radix the argument forms -- the
three sources of the inter-pass twiddle (a third of the tables random field elements, so that any index error shows), short sources,
src == dst, middle passes, digit reversals of 0 .. 3 unequal digits, scale -- then ntt_tiny_kernel, shk_tw2, shk_powers and
shk_pad_copy.  Each case is compared with the definition of its pass over Python integers as residues mod p, exactly, and reports
its first wrong (vector, column / row, k).  The cases that run in the cell the default knobs choose also assert that the library's
chooser names that cell.

Then whole transforms through the C ABI over a batch grid (sh_ntt_batch with full and short sources, sh_dev_ntt in place), every
vector against the C oracle, and once more in a child process where every tile pass takes the XCD mapping.

The fixture prints the harness's build time and the grid's run time (pytest -s); the limits are below."""
import ctypes
import os
import random
import subprocess
import sys
import time

import pytest

import ntt_cases as nc

pytestmark = pytest.mark.gpu

# Measured on the MI355X: the 632 jobs run in 3.1 s (the harness builds in 35 s there; its limit is ntt_cases.BUILD_TIMEOUT).  The
# limit is that + 117 s of margin: the process moves 1.8 GB of outputs through hipMemcpy and the file system of a shared machine.
GRID_TIMEOUT = 120


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("STARKHIP_")}
    env.update(extra)
    return env


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """one harness process for the whole grid; if it fails every case fails, and nothing is run again"""
    d = tmp_path_factory.mktemp("ntt_gpu")
    t0 = time.time()
    exe = nc.build(d)
    t1 = time.time()
    outs, chosen = nc.run(exe, [c["name"] for c in nc.cases()], d, timeout=GRID_TIMEOUT, env=_clean_env())
    print("\nntt_ops: built in %.1f s, %d cases run in %.1f s" % (t1 - t0, len(outs), time.time() - t1))
    return outs, chosen


@pytest.mark.parametrize("name", [c["name"] for c in nc.cases()])
def test_harness_case(results, name):
    outs, chosen = results
    c = nc.case(name)
    why = nc.check(c, nc.read_output(outs[name]))
    assert why is None, "%s (%s): %s" % (name, sorted(nc.cells_of(c), key=str), why)
    if c["op"] == "pass":
        want = nc.choose_cell(nc.DEFAULT_KNOBS, c["log_R"], c["last"], c["total"], c["log_n"], c["log_S"], c["pass_index"])
        assert chosen[name] == want, "the library would run %s in %s, the documented rules say %s" % (name, chosen[name], want)
        if c["default"]:
            assert (c["form"], c["tile_log"], c["xcd"]) == want


# ---- whole transforms through the C ABI ----------------------------------------------------------------------------------------------
ABI_GRID = [(1, 1000), (2, 4097), (4, 65537), (256, 1031), (1 << 10, 67), (1 << 11, 67), (1 << 12, 33), (1 << 16, 9)]


@pytest.fixture(scope="module")
def api():
    from starks_amd import _lib
    return _lib.lib(), _lib.ctx()


def _batch_wire(n, batch, seed):
    """[batch][n] wire values: random, the edge set at the first and last positions of the first and last vector"""
    rng = random.Random(seed)
    buf = bytearray(rng.randbytes(32 * n * batch))
    for b in {0, batch - 1}:
        v = [None] * n
        nc._place_edges(v, b)
        for i, x in enumerate(v):
            if x is not None:
                buf[32 * (b * n + i):32 * (b * n + i) + 32] = x.to_bytes(32, "big")
    return bytes(buf)


def _first_bad(got, want, n):
    i = next(i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32])
    return "first wrong element: vector %d, index %d" % (i // n, i % n)


@pytest.mark.parametrize("n,batch", ABI_GRID, ids=["n%d_b%d" % nb for nb in ABI_GRID])
def test_abi_batch_grid(api, n, batch):
    """sh_ntt_batch (full and short sources) and sh_dev_ntt with d_in == d_out: forward and inverse over the roots 7^((p-1)/n) raised
    to 1, 3 and n - 1, every vector of the batch against the C oracle"""
    from oracle import coracle
    L, ctx = api
    wire = _batch_wire(n, batch, "abi/%d/%d" % (n, batch))
    shorts = sorted({n_in for n_in in (1, n // 8 + 1, n - 1) if 0 < n_in < n})
    dbuf = ctypes.c_void_p()
    assert L.sh_dev_alloc(ctx, 32 * n * batch, ctypes.byref(dbuf)) == 0
    try:
        for e in (sorted({e % n for e in (1, 3, n - 1)}) if n > 1 else [0]):
            w = pow(nc.root_of(n), e, nc.P) if n > 1 else 1
            for inverse in (False, True):
                for k, n_in in enumerate([n] + shorts):
                    if n_in < n and len(shorts) > 1 and (k + e + inverse) % len(shorts) and n >= 256:
                        continue  # from 256 points one short source per (root, direction), taking turns
                    src = b"".join(wire[32 * n * b:32 * (n * b + n_in)] for b in range(batch)) if n_in < n else wire
                    want = b"".join(coracle.fft_bytes(src[32 * n_in * b:32 * n_in * (b + 1)], n, w, inverse) for b in range(batch))
                    out = ctypes.create_string_buffer(32 * n * batch)
                    assert L.sh_ntt_batch(ctx, src, n_in, out, n, batch, w.to_bytes(32, "big"), int(inverse)) == 0
                    assert out.raw == want, "sh_ntt_batch n_in %d root^%d inverse %d: %s" % (n_in, e, inverse, _first_bad(out.raw, want, n))
                    if n_in == n:
                        assert L.sh_dev_from_wire(ctx, wire, dbuf, n * batch) == 0
                        assert L.sh_dev_ntt(ctx, dbuf, dbuf, n, batch, w.to_bytes(32, "big"), int(inverse)) == 0
                        assert L.sh_dev_to_wire(ctx, dbuf, out, n * batch) == 0
                        assert out.raw == want, "sh_dev_ntt in place root^%d inverse %d: %s" % (e, inverse, _first_bad(out.raw, want, n))
    finally:
        assert L.sh_dev_free(ctx, dbuf) == 0


def test_abi_batch_grid_every_pass_xcd_mapped():
    """the 2^10, 2^11 and 2^12 rows of the batch grid in a child process with STARKHIP_XCD_SWZ=2 and the narrow form off (2^11 points as
    one radix-2^11 pass): 67 and 132 tiles per pass, so the library's own launches take the padded grid"""
    from conftest import ROOT
    env = _clean_env(STARKHIP_XCD_SWZ="2", STARKHIP_NTT_NARROW_TILES="0", STARKHIP_NTT_RADICES="11")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "-k",
                          "test_abi_batch_grid and (n1024_b67 or n2048_b67 or n4096_b33)"], capture_output=True, text=True,
                         timeout=120, env=env, cwd=ROOT)  # measured: 3.1 s
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "3 passed" in out.stdout
