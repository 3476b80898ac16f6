"""Registers, scratch and the static VALU instruction count of the NTT kernels, from one cross-compile of starks_amd/csrc/ntt.hip to
gfx950 assembly (about a minute, no GPU).  The tile passes' time is their VALU instruction count, and the cells'
LDS rule rests on which kernels fit 96 registers: both are pinned here.  Mnemonics are counted by their prefix `v_` only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "starks_amd", "csrc")

# (LOG_R, LOG_T, LAST) of the ntt_pass_kernel instances above 96 VGPRs (and at most 128) in the build before the address and fold
# instructions were trimmed; every other NTT kernel -- the other tile passes, the narrow passes, the tiny kernel -- is at most 96.
ABOVE_96 = {(4, 5, 0), (4, 6, 0), (5, 4, 0), (5, 5, 0), (5, 6, 0), (5, 6, 1), (5, 7, 0), (5, 7, 1), (6, 3, 0), (6, 4, 0), (6, 5, 0),
            (6, 5, 1), (6, 6, 0), (7, 2, 0), (7, 3, 0), (7, 3, 1), (7, 4, 0), (7, 5, 0), (7, 5, 1), (8, 1, 0), (8, 2, 0), (8, 2, 1),
            (8, 3, 0), (8, 4, 0), (9, 1, 0), (9, 1, 1), (9, 2, 0), (9, 2, 1), (9, 3, 0), (9, 3, 1), (10, 0, 0), (10, 1, 0), (10, 1, 1),
            (10, 2, 0), (10, 2, 1), (11, 0, 0), (11, 1, 0), (11, 1, 1)}
# static `v_` instructions of the 2^24 transform's three kernels: 5946 / 5959 / 4477 before; the pair addresses, the wave-uniform row
# strides, the three-instruction fold and the products' first column took 145 / 160 / 117 out
VALU_CEILING = {(8, 3, 0): 5801, (8, 2, 0): 5799, (8, 2, 1): 4360}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: (VGPRs, scratch bytes, static v_ count)}"""
    out = tmp_path_factory.mktemp("ntt_asm") / "ntt.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-S", "ntt.hip",
                           "-o", str(out)], cwd=CSRC)
    K, cur = {}, None
    with open(out) as fh:
        for line in fh:
            s = line.strip()
            m = re.match(r"^(_Z\w+):", line)
            if m and cur is None:
                cur = m.group(1)
                K[cur] = [None, None, 0]
            elif cur is not None:
                if s.startswith(".amdhsa_next_free_vgpr"):
                    K[cur][0] = int(s.split()[1])
                elif s.startswith(".amdhsa_private_segment_fixed_size"):
                    K[cur][1] = int(s.split()[1])
                elif s.startswith(".end_amdhsa_kernel"):
                    cur = None
                elif s.startswith("v_"):
                    K[cur][2] += 1
    return K


def _cell(name):
    m = re.match(r"_Z15ntt_pass_kernelILi(\d+)ELi(\d+)ELb([01])EEv11NttPassArgs$", name)
    return (int(m.group(1)), int(m.group(2)), int(m.group(3))) if m else None


def test_every_ntt_kernel_is_there(kernels):
    assert len(kernels) == 101 and sum(_cell(k) is not None for k in kernels) == 68   # 68 tile + 32 narrow + tiny
    assert all(v[0] is not None and v[1] is not None for v in kernels.values())


def test_no_scratch(kernels):
    assert {k: v[1] for k, v in kernels.items() if v[1] != 0} == {}


def test_register_classes(kernels):
    bad = {}
    for k, (vgpr, _, _) in kernels.items():
        want = 128 if _cell(k) in ABOVE_96 else 96
        if not (vgpr <= want and (want == 96 or vgpr > 96)):
            bad[k] = (vgpr, want)
    assert bad == {}, "kernel: (VGPRs, class): %s" % bad


def test_headline_valu_count(kernels):
    got = {_cell(k): v[2] for k, v in kernels.items() if _cell(k) in VALU_CEILING}
    print(got)
    assert set(got) == set(VALU_CEILING)
    assert all(got[c] <= VALU_CEILING[c] for c in got), got
