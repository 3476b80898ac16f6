"""The addresses the NTT tile passes derive from one value per thread (starks_amd/csrc/ntt_kernels.cuh: tile_tw_byte, tile_tw_pair_xor,
tile_out_k_step), enumerated on the host by tests/native/ntt_addr_host.cpp with the header's own helpers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "starks_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "ntt_addr_host.cpp")


def test_pair_addresses_and_output_rows(tmp_path):
    """Every cell that keeps its twiddles in LDS (15), both pass kinds, every register group, thread and butterfly: the four reads of a
    pair -- one address per level, XOR the pair constant, XOR 16 c -- land on 16 * tw_lds_slot(exponent, c), the same 821248 chunk reads
    tests/test_tw_lds_map_host.py counts.  And for radix 2^2 .. 2^11 the frequency of the last group's element h is that of h = 0 plus
    {0, R/2, R/4, 3R/4}[h] for every row base: (4 + 8 + ... + 2048) = 4092 rows."""
    exe = tmp_path / "ntt_addr_host"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1", "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "15 cells with twiddles in LDS, 821248 chunk reads, 4092 output rows, 0 failures"
