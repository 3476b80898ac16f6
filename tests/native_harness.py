"""Building and driving the elementwise native harnesses (tests/native/fp256_ops.hip, tests/native/blake2s_ops.hip).  Both take
"--device|--host JOBS", one job per line "op n grid block in out", and write n result records per job."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "starks_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


def build(src, exe, defines=(), csrc=None, timeout=600):
    """hipcc for gfx950 with the library's flags (-O3, the inline asm on) plus `defines`; `src` is one source or a list of them"""
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I", csrc or CSRC] + ["-D" + d for d in defines]
    srcs = [src] if isinstance(src, str) else list(src)
    subprocess.check_call(cmd + srcs + ["-o", str(exe)], timeout=timeout)
    return str(exe)


def run_jobs(exe, mode, jobs, workdir, inputs, timeout=600):
    """jobs: (op, part, grid, block, tag) -> {tag: result bytes}.  inputs(op, part) -> (record count, input bytes).  One process runs
    every job, under its own time limit."""
    lines, outs = [], {}
    for op, part, grid, block, tag in jobs:
        n, data = inputs(op, part)
        inp = os.path.join(str(workdir), "%s.%s.in" % (op, part))
        if not os.path.exists(inp):
            with open(inp, "wb") as fh:
                fh.write(data)
        out = os.path.join(str(workdir), "%s.out" % tag)
        lines.append("%s %d %d %d %s %s" % (op, n, grid, block, inp, out))
        outs[tag] = out
    jf = os.path.join(str(workdir), "jobs.%s.%s" % (os.path.basename(str(exe)), mode))
    with open(jf, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    p = subprocess.run([str(exe), "--" + mode, jf], capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, "%s --%s exited %d: %s%s" % (os.path.basename(str(exe)), mode, p.returncode, p.stdout, p.stderr)
    res = {}
    for tag, out in outs.items():
        with open(out, "rb") as fh:
            res[tag] = fh.read()
    return res
