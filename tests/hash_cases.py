"""Messages, launch layouts and expected bytes for every form of starks_amd/csrc/blake2s.cuh and for sample_indices_quad, as run by
tests/native/blake2s_ops.hip.  Shared by tests/test_blake2s_host.py (CPU: the portable paths, and the compile check of every build)
and tests/test_gpu_blake2s.py (GPU: every build on the device).

Every digest is hashlib.blake2s of the message, and every index set starks_amd.utils.get_pseudorandom_indices of its arguments
(tests/test_host_cpu.py pins that function to the reference through tests/golden/utils.json).  Records are the harness's: the words
a kernel loads and stores, little-endian, so a message's record is its bytes.  Output buffers start as 0xa5 bytes, so a record a
kernel must leave alone is expected to read back as 0xa5 bytes."""
import functools
import hashlib
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import native_harness

ROOT = native_harness.ROOT
HARNESS = os.path.join(ROOT, "tests", "native", "blake2s_ops.hip")
GENERATOR = os.path.join(native_harness.CSRC, "gen_blake2s_asm.py")

CHAIN_MAX, VB_MAX, SAMPLE_WORDS = 255, 32 * 27, 256
# op: (input record bytes, output record bytes, per quad)
OPS = {"pair": (64, 64, False), "short": (128, 64, False), "chain": (64 + 64 * CHAIN_MAX, 64, False),
       "vbtwo": (32 + 2 * VB_MAX, 32, False), "quad": (80, 32, True), "sample": (48, 4 * SAMPLE_WORDS, True)}
SENTINEL = b"\xa5"
N_RANDOM_PAIR = 100000

# The builds: the library's defaults, the header's two A/B switches alone and together, and the generator's other forms of the
# single-lane asm rounds (each a generated include selected with -DB2_ASM_INC).  name: (defines, generator flags or None)
BUILDS = {
    "default": ((), None),
    "no_asm": (("B2_NO_ASM",), None),
    "no_quad_asm": (("B2Q_NO_ASM",), None),
    "no_asm_no_quad_asm": (("B2_NO_ASM", "B2Q_NO_ASM"), None),
    "gen_two_adds": ((), ("--two-adds",)),
    "gen_no_branch": ((), ("--no-branch",)),
    "gen_e64": ((), ("--e64",)),
    "gen_align": ((), ("--align",)),
    "gen_sdwa16": ((), ("--sdwa16",)),
}
MAX_HIPCC = 4


def blake(m):
    return hashlib.blake2s(m).digest()


def _w(*words):
    return b"".join(w.to_bytes(4, "little") for w in words)


# ---- messages --------------------------------------------------------------------------------------------------------------------
def special_blocks():
    """64-byte messages where an add or a rotate goes wrong first: all-zero, all-0xff, words of 0xffffffff / 0x80000000 (every add
    carries out of bit 31), one set bit and one clear bit at each of the 512 positions"""
    out = [bytes(64), b"\xff" * 64, _w(*[0x80000000] * 16), _w(*[0xffffffff, 0x80000000] * 8), _w(*[0x80000000, 0xffffffff] * 8),
           _w(*[0x7fffffff] * 16), _w(*[0xffffffff] * 8 + [0] * 8), _w(*[0] * 8 + [0x80000000] * 8)]
    for bit in range(512):
        v = 1 << bit
        out.append(v.to_bytes(64, "little"))
        out.append(((1 << 512) - 1 - v).to_bytes(64, "little"))
    return out


def _fill(rng, kind, n):
    """n message bytes of a kind: 0 zero, 1 all 0xff, 2 carry words, 3 one set bit, else random"""
    if kind == 0:
        return bytes(n)
    if kind == 1:
        return b"\xff" * n
    if kind == 2:
        return (_w(*[0xffffffff, 0x80000000] * ((n + 7) // 8)))[:n]
    if kind == 3 and n:
        return (1 << rng.randrange(8 * n)).to_bytes(n, "little")
    return rng.randbytes(n)


# ---- cases: (input bytes per record, expected bytes per record) --------------------------------------------------------------------
def _pair(part):
    rng = random.Random(0xb2)
    msgs = special_blocks() + [rng.randbytes(64) for _ in range(N_RANDOM_PAIR)]
    return [(m, blake(m) * 2) for m in msgs]


def _short(part):
    """every len 0..64, one wave of messages per len, zero past len as the call sites pad"""
    rng = random.Random(0x5407)
    recs = []
    for ln in range(65):
        for lane in range(64):
            m = _fill(rng, lane, ln)
            recs.append((_w(ln) + bytes(60) + m + bytes(64 - ln), blake(m) * 2))
    return recs


CHAIN_KS = tuple(range(1, 65)) + (96, 128, 255)


def _chain_rec(k, m):
    return _w(k) + bytes(60) + m + bytes(64 * (CHAIN_MAX - k)), blake(m) * 2


def _chain(part):
    """"uniform": one wave of 64 messages per block count k; "mixed": every lane its own k, and a partial last wave"""
    rng = random.Random(0xc4a1 + (part == "mixed"))
    if part == "uniform":
        return [_chain_rec(k, _fill(rng, lane, 64 * k)) for k in CHAIN_KS for lane in range(64)]
    ks = [CHAIN_KS[(7 * i + i // 64) % len(CHAIN_KS)] for i in range(300)]
    return [_chain_rec(k, _fill(rng, i % 5, 64 * k)) for i, k in enumerate(ks)]


VB_LENS = tuple(range(32, VB_MAX + 1, 32))


def _vb_rec(ln, a, b):
    return _w(ln) + bytes(28) + a + bytes(VB_MAX - ln) + b + bytes(VB_MAX - ln), blake(a + b)


def _vbtwo(part):
    """blake2s(a || b), a and b len bytes each: "uniform" one wave per len, "mixed" every lane its own len (a partial last wave)"""
    rng = random.Random(0x7b2 + (part == "mixed"))
    if part == "uniform":
        return [_vb_rec(ln, _fill(rng, lane, ln), _fill(rng, lane, ln)) for ln in VB_LENS for lane in range(64)]
    return [_vb_rec(VB_LENS[(5 * i) % len(VB_LENS)], _fill(rng, i % 5, VB_LENS[(5 * i) % len(VB_LENS)]),
                    _fill(rng, i % 7, VB_LENS[(5 * i) % len(VB_LENS)])) for i in range(150)]


QUAD_BLOCKS = (64, 256, 512)   # threads: the sampler's blocks, and merkle_top_kernel's QUADS = 64 and 128


def _quad_rec(m, tcount, live=True):
    """one quad's message: the first tcount bytes of m, zero padded (b2q_compress hashes one final block from the IV)"""
    m = m[:tcount] + bytes(64 - tcount)
    return m + _w(tcount, int(live), 0, 0), (blake(m[:tcount]) if live else SENTINEL * 32)


def _quad(part):
    """"main": every quad live -- the special blocks with tcount 64 and 32, every tcount 0..64, random messages; "prefix<B>": blocks
    of B threads where quads 0..active-1 are live (active = 1, 2, 4, ... B / 4, as merkle_top_kernel halves it), then a partial block"""
    rng = random.Random(0x4ad + len(part))
    if part == "main":
        recs = [_quad_rec(m, t) for m in special_blocks() for t in (64, 32)]
        recs += [_quad_rec(_fill(rng, i, 64), t) for t in range(65) for i in range(8)]
        recs += [_quad_rec(rng.randbytes(64), 64 if i & 1 else 32) for i in range(20000 - len(recs) - 37)]
        return recs
    quads = int(part[len("prefix"):]) // 4
    recs, active = [], 1
    while active <= quads:
        recs += [_quad_rec(_fill(rng, i, 64), (64, 32)[i & 1], i < active) for i in range(quads)]
        active *= 2
    return recs + [_quad_rec(rng.randbytes(64), 64) for _ in range(quads // 2 + 3)]


SAMPLE_COUNTS = (0, 1, 3, 4, 7, 8, 9, 40, 41, 80, 81, 255)
SAMPLE_EXCLUDES = (0, 2, 3, 8, 16, 255, 1 << 20)


def sample_moduli():
    rng = random.Random(0x5a)
    return (1, 2, 3, 4) + tuple(1 << k for k in (3, 5, 8, 10, 13, 16, 20, 23)) + ((1 << 24) - 1,) + tuple(
        rng.randrange(5, 1 << 24) for _ in range(2))


def real_modulus(modulus, exclude):
    return modulus * (exclude - 1) // exclude if exclude else modulus


def sample_args():
    """(modulus, count, exclude) combinations the library takes: modulus < 2^24 and a real modulus of at least 1"""
    return [(m, c, e) for m in sample_moduli() for c in SAMPLE_COUNTS for e in SAMPLE_EXCLUDES if real_modulus(m, e) >= 1]


def _sample_rec(entropy, modulus, count, exclude):
    from starks_amd.utils import get_pseudorandom_indices
    ys = get_pseudorandom_indices(entropy, modulus, count, exclude)
    return entropy + _w(modulus, count, exclude, 0), _w(*ys) + SENTINEL * (4 * (SAMPLE_WORDS - count))


def _sample(part):
    """"main": one 64-thread block (16 quads) per argument combination, the last block cut to 9 live quads; "one": a single live quad
    with count 255 (15 dead quads); "three": three live quads"""
    rng = random.Random(0x5e + len(part))
    if part == "main":
        recs = []
        for modulus, count, exclude in sample_args():
            recs += [_sample_rec(_fill(rng, i, 32), modulus, count, exclude) for i in range(16)]
        return recs[:-7]
    if part == "one":
        return [_sample_rec(rng.randbytes(32), (1 << 24) - 1, 255, 0)]
    return [_sample_rec(_fill(rng, i, 32), 1000, 81, 8) for i in range(3)]


CASES = {"pair": _pair, "short": _short, "chain": _chain, "vbtwo": _vbtwo, "quad": _quad, "sample": _sample}
PARTS = {"pair": ("main",), "short": ("main",), "chain": ("uniform", "mixed"), "vbtwo": ("uniform", "mixed"),
         "quad": ("main",) + tuple("prefix%d" % b for b in QUAD_BLOCKS), "sample": ("main", "one", "three")}
HOST_OPS = ("pair", "short", "chain", "vbtwo")


@functools.lru_cache(maxsize=None)
def case_set(op, part):
    """-> (record count, input bytes, expected bytes)"""
    recs = CASES[op](part)
    ib, ob, _ = OPS[op]
    assert all(len(i) == ib and len(o) == ob for i, o in recs), op
    return len(recs), b"".join(i for i, _ in recs), b"".join(o for _, o in recs)


def mismatches(op, part, got, block=64, limit=5):
    """the first few records that differ from the expected bytes, as readable text (lane: within a wave of `block`-thread blocks;
    for pair, short and chain, which half differs: the <true> form's digest or the <false> one's)"""
    n, inp, want = case_set(op, part)
    ib, ob, per_quad = OPS[op]
    if len(got) != len(want):
        return "%s/%s: %d result bytes, want %d" % (op, part, len(got), len(want))
    bad = []
    for i in range(n):
        g, e = got[i * ob:(i + 1) * ob], want[i * ob:(i + 1) * ob]
        if g != e:
            where = [h for h, s in (("<true>", slice(0, 32)), ("<false>", slice(32, 64))) if g[s] != e[s]] if ob == 64 else []
            lane = (4 * i if per_quad else i) % block % 64
            bad.append("record %d (lane %d) %s, input %s...: got %s want %s" % (i, lane, "/".join(where), inp[i * ib:i * ib + 16].hex(),
                                                                               g[:40].hex(), e[:40].hex()))
            if len(bad) == limit:
                break
    return "%s/%s: %d bad records: %s" % (op, part, sum(got[i * ob:(i + 1) * ob] != want[i * ob:(i + 1) * ob] for i in range(n)),
                                          "; ".join(bad))


# ---- the harness -----------------------------------------------------------------------------------------------------------------
def build_harness(exe, name, workdir):
    """build `name` of BUILDS at path `exe`; a generator form's include is generated into `workdir` (nothing under csrc is written)"""
    defines, gen = BUILDS[name]
    defines = list(defines)
    if gen is not None:
        inc = os.path.join(str(workdir), "blake2s_asm_%s.inc" % name)
        subprocess.check_call([sys.executable, GENERATOR, inc] + list(gen), timeout=120)
        defines.append('B2_ASM_INC="%s"' % inc)
    return native_harness.build(HARNESS, exe, defines)


def build_all(workdir, names=tuple(BUILDS)):
    """{name: exe}, at most MAX_HIPCC compilers at once"""
    with ThreadPoolExecutor(MAX_HIPCC) as ex:
        futs = {n: ex.submit(build_harness, os.path.join(str(workdir), "blake2s_ops_" + n), n, workdir) for n in names}
        return {n: f.result() for n, f in futs.items()}


def run_jobs(exe, mode, jobs, workdir, timeout=600):
    """jobs: (op, part, grid, block, tag) -> {tag: result bytes}.  One process runs every job."""
    return native_harness.run_jobs(exe, mode, jobs, workdir, lambda op, part: case_set(op, part)[:2], timeout)


def grid(op, part, block, extra=0):
    n = case_set(op, part)[0]
    threads = 4 * n if OPS[op][2] else n
    return (threads + block - 1) // block + extra


def device_jobs():
    """(op, part, grid, block, tag) for every op and layout of the device run"""
    jobs = [("pair", "main", grid("pair", "main", 256), 256, "pair.main.256"),
            ("pair", "main", grid("pair", "main", 96, 1), 96, "pair.main.96")]   # 96: a partial wave per block, one whole block past the end
    for block in (64, 256):
        jobs.append(("short", "main", grid("short", "main", block), block, "short.main.%d" % block))
    for op in ("chain", "vbtwo"):
        for part in ("uniform", "mixed"):
            for block in (64, 256):
                jobs.append((op, part, grid(op, part, block), block, "%s.%s.%d" % (op, part, block)))
    for block in QUAD_BLOCKS:
        jobs.append(("quad", "main", grid("quad", "main", block), block, "quad.main.%d" % block))
        jobs.append(("quad", "prefix%d" % block, grid("quad", "prefix%d" % block, block), block, "quad.prefix%d.%d" % (block, block)))
    for part in PARTS["sample"]:
        jobs.append(("sample", part, grid("sample", part, 64), 64, "sample.%s.64" % part))
    return jobs
