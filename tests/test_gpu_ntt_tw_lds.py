"""The NTT tile passes with their twiddle table in LDS (starks_amd/csrc/ntt_kernels.cuh: tile_tw_in_lds) on the MI355X: whole
transforms on two contexts at once against the C oracle, byte for byte, and the resident workgroups per CU of every such cell."""
import ctypes
import os
import random
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2**256 - 351 * 2**32 + 1
# 2^16 x 8: 512 tiles a pass, the smallest shape whose two radix-2^8 passes run in the <8,2,*> tile cells by default (32 + 8 KiB of LDS,
# four workgroups per CU); 2^17 x 4: <9,2,false> (64 + 16 KiB, two per CU: the cell that fills the LDS exactly) and <8,2,true>
SHAPES = [(1 << 16, 8), (1 << 17, 4)]


def _default_cells(n, batch):
    """the cells the default chooser gives the passes of `batch` n-point transforms: the plan as knobs.hpp documents it (2^9 .. 2^16: two
    passes, radices as equal as possible, the larger first; 2^17 .. 2^19: radix 2^9 then the rest), each pass through the host model of
    the chooser in tests/ntt_cases.py (which tests/test_gpu_ntt_passes.py holds against the library's own choice)"""
    import ntt_cases as nc
    log_n = n.bit_length() - 1
    radices = [(log_n + 1) // 2, log_n // 2] if log_n <= 16 else [9, log_n - 9]
    cells, done = [], 0
    for d, r in enumerate(radices):
        last = d == len(radices) - 1
        done += r
        form, tile_log, _ = nc.choose_cell(nc.DEFAULT_KNOBS, r, last, batch * (n >> r), log_n, log_n - done, d)
        cells.append((form, r, tile_log - r, last))
    return cells


def test_forward_and_inverse_on_two_contexts_at_once():
    """Context A transforms forward while context B transforms the same vectors back, then the other way round, nothing synchronised
    in between (the table in LDS is written behind one barrier and read by every wave of the workgroup without another: a race there
    would show under a second stream, as round 4's did); every output byte against oracle.coracle.  One run, no repetition."""
    from oracle import coracle
    from starks_amd import _lib
    L = _lib.lib()
    # the shapes must reach the cells they are here for, under the knobs of this process
    assert not [k for k in os.environ if k.startswith("STARKHIP_") and k != "STARKHIP_LIB"]
    assert _default_cells(1 << 16, 8) == [("tile", 8, 2, False), ("tile", 8, 2, True)]
    assert _default_cells(1 << 17, 4) == [("tile", 9, 2, False), ("tile", 8, 2, True)]
    assert [int(L.sh_ntt_passes(n, 1)) for n, _ in SHAPES] == [2, 2]
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    bufs, jobs = [], []
    try:
        for n, batch in SHAPES:
            w = pow(7, (P - 1) // n, P)
            wire = random.Random("tw_lds/%d/%d" % (n, batch)).randbytes(32 * n * batch)
            want = [b"".join(coracle.fft_bytes(wire[32 * n * b:32 * n * (b + 1)], n, w, bool(inv)) for b in range(batch)) for inv in (0, 1)]
            src = []
            for c in ctxs:
                d = ctypes.c_void_p()
                assert L.sh_dev_alloc(c, 32 * n * batch, ctypes.byref(d)) == 0
                bufs.append((c, d))
                assert L.sh_dev_from_wire(c, wire, d, n * batch) == 0
                src.append(d)
            for first in (0, 1):  # A forward + B inverse, then A inverse + B forward
                for k, c in enumerate(ctxs):
                    inv = first ^ k
                    d = ctypes.c_void_p()
                    assert L.sh_dev_alloc(c, 32 * n * batch, ctypes.byref(d)) == 0
                    bufs.append((c, d))
                    assert L.sh_dev_ntt(c, src[k], d, n, batch, w.to_bytes(32, "big"), inv) == 0
                    jobs.append((c, d, n, batch, inv, want[inv]))
        for c, d, n, batch, inv, want in jobs:
            out = ctypes.create_string_buffer(32 * n * batch)
            assert L.sh_dev_to_wire(c, d, out, n * batch) == 0
            assert out.raw == want, "n %d x %d inverse %d on context %d" % (n, batch, inv, ctxs.index(c))
    finally:
        for c, d in bufs:
            assert L.sh_dev_free(c, d) == 0


def test_the_table_costs_no_workgroup_per_cu(tmp_path):
    """tests/native/ntt_occupancy.hip asks the runtime for the resident workgroups per CU of the library's own kernels, every cell
    with its table in LDS (15 x 2 pass kinds), at the size of the tile image alone and of image + table: equal for every cell, and
    what 16 waves per CU allow (1024 / threads) -- the table fits in what the tile left over, also where the sum is exactly 160 KiB."""
    from starks_amd import _lib
    exe = tmp_path / "ntt_occupancy"
    libdir, libname = os.path.split(os.path.abspath(_lib.LIB_PATH))  # the library under test (STARKHIP_LIB or the tree's)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "starks_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "ntt_occupancy.hip"), "-L", libdir, "-l:" + libname,
                           "-Wl,-rpath," + libdir, "-o", str(exe)], timeout=300)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    assert len(rows) == 30
    for log_r, log_t, last, image, both, at_image, at_both in rows:
        assert both == image + (32 << log_r)
        assert at_both == at_image == 1024 >> (log_r + log_t - 2), (log_r, log_t, last, image, both, at_image, at_both)
