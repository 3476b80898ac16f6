"""The NTT tile passes' twiddle table in LDS (starks_amd/csrc/ntt_kernels.cuh: tile_tw_in_lds, tw_lds_slot, tile_tw_fill_chunk),
enumerated on the host by tests/native/tw_lds_map_host.cpp: which cells keep the table in LDS, that the copy fills every slot once,
that every read finds the pair the global-memory path reads, and how the reads fall on the LDS banks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "starks_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "tw_lds_map_host.cpp")


def _build(tmp_path, *defines):
    exe = tmp_path / ("tw_lds_map_host" + "".join(defines))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC] + list(defines) +
                          [SRC, "-o", str(exe)], stderr=subprocess.DEVNULL)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_twiddle_table_in_lds_holds_what_the_global_path_reads(tmp_path):
    """Every existing tile cell (34), both pass kinds, every register group, thread and twiddle product.  15 cells qualify: the
    1024-element tile of radix 2^8 (the flagship's <8,2,*>: 32 + 8 KiB, four per CU = 160 KiB), the 2048-element tiles to radix 2^9
    (<8,3,*>: 64 + 8 KiB; <9,2,*>: 64 + 16 KiB, two per CU = 160 KiB) and the 4096-element tiles to radix 2^9; radix 2^10 and 2^11 do
    not, and neither do the 512- and 1024-element tiles of the radices below 2^8, whose kernels fit a fifth wave per SIMD and then fill
    the CU with tile images alone (tests/test_gpu_ntt_tw_lds.py asks the runtime).  Banking, per 16-lane group of ds_read_b128: the cap
    is 2 distinct pairs on one bank quarter; the layout holds it wherever a lane group reads at most 8 pairs, and in every read, the
    16-pair reads of the row pass's first group included (4 pairs to a quarter whatever the layout), no bank is asked for more than
    ONE address -- the reads are conflict-free."""
    out = _build(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == ("34 cells, 15 with twiddles in LDS, 821248 chunk reads, at most 1 addresses per bank, 2 pairs per bank "
                                  "quarter (4 where a lane group reads 16 pairs), 0 failures")


def test_build_switch_restores_the_global_loads(tmp_path):
    """-DSHK_TW_LDS=0: no cell qualifies and every cell asks for the tile image alone"""
    out = _build(tmp_path, "-DSHK_TW_LDS=0")
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("34 cells, 0 with twiddles in LDS, 0 chunk reads,") and out.stdout.strip().endswith("0 failures")
