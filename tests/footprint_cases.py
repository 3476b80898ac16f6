"""The write-footprint audit of the device-resident C ABI (test_footprint_host.py, test_gpu_footprint.py): a guarded arena, a pure
checker over byte strings and one table row per sh_dev_* entry of include/starkhip.h.

ARENA.  Every buffer of a call lies in ONE sh_dev_alloc block as guard | payload | guard, GUARD = 256 KiB on each side (twice the
largest tile image a kernel holds: 4096 x 32 B in ntt_kernels.cuh, 2^13 x 8 B in ntt64.hip, 2^10 x 32 B in modntt.hip), payloads on
256-byte offsets.  Host outputs lie the same way in one host block (pageable, or one sh_host_alloc block for the asynchronous copy).
Guards and outputs are prefilled with pattern(seed): pseudorandom and position dependent, and the patterns of seeds 1 and 2 differ in
EVERY byte, so an output byte nobody wrote differs between the two runs.

RUNS.  A row's shape runs twice on the same inputs: run A on a fresh context with seed 1, run B on the same context with seed 2 after a
polluter call (a larger entry of another family) has left other contents in the shared workspaces.  check() wants every guard and
every read-only payload intact, compare_runs() wants the outputs of A and B byte-identical, and for the row's anchor shape the output
equals the exact model of the entry's *_cases module (modntt_cases.transform, modpoly_cases, oracle/pyoracle.py).  One limit: an
in/out payload holds the same input in both runs, so a byte of it that the call leaves unwritten shows only at the anchor shape.
Inputs that the library itself makes (the verifier rows' honest proofs, from the host-buffer prover) are made on a context of their
own that is destroyed before run A, so run A's context is fresh for those rows too.

TABLE.  ROWS holds one Row per (entry, aliasing form, knob).  roles maps every pointer argument of the C prototype to
    "const"          a small host constant (modulus, root, terms): passed as immutable bytes, not part of the arena
    "in"             read-only device payload            "hin"             read-only host payload
    "out:<expr>"     device output of <expr> bytes       "hout:<expr>"     host output of <expr> bytes
    "inout:<expr>"   device input that the call overwrites (an in-place form, sh_dev_lde's d_trace)
    "=<arg>"         the same pointer as <arg> (the aliasing the header permits)
<expr> is a Python expression over the shape's variables: the exact byte length include/starkhip.h gives for that output.
`cite` names the line of code that sets the boundary the shapes straddle."""
import ctypes
import hashlib
import os
import random
import re

import numpy as np

import modntt_cases as mc
import modpoly_cases as pc
import modstark_cases as sc
from oracle import pyoracle

GUARD = 256 * 1024
ALIGN = 256
OK = 0
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "starkhip.h")
EXEMPT = {
    "sh_dev_alloc": "returns a block, writes no caller buffer (every arena of the audit comes from it)",
    "sh_dev_free": "releases a block, writes no caller buffer (every arena of the audit goes through it)",
}


# ---- pattern, layout, checker: pure functions over byte strings ----------------------------------------------------------------------
def _stream(key, nbytes):
    return np.random.Generator(np.random.Philox(key=key)).integers(0, 256, size=nbytes, dtype=np.uint8)


def pattern(seed, nbytes):
    """nbytes pseudorandom bytes, a function of (seed, position).  An even seed is the odd seed below it plus a nonzero byte at every
    position: pattern(1) and pattern(2) differ everywhere."""
    if seed % 2:
        return _stream(seed, nbytes).tobytes()
    step = (_stream(seed, nbytes) % 255 + 1).astype(np.uint8)
    return (_stream(seed - 1, nbytes) + step).astype(np.uint8).tobytes()


class Region(object):
    def __init__(self, name, role, off, nbytes):
        self.name, self.role, self.off, self.nbytes = name, role, off, nbytes

    @property
    def end(self):
        return self.off + self.nbytes


class Layout(object):
    """regions in address order, each between two guards; everything outside the payloads is guard"""

    def __init__(self, bufs, guard=GUARD):
        self.regions, off = [], guard
        for name, role, nbytes in bufs:
            self.regions.append(Region(name, role, off, nbytes))
            off = (off + nbytes + ALIGN - 1) // ALIGN * ALIGN + guard
        self.total = off if self.regions else 0

    def __getitem__(self, name):
        return next(r for r in self.regions if r.name == name)

    def guards(self):
        pos = 0
        for r in self.regions:
            yield pos, r.off
            pos = r.end
        if self.regions:
            yield pos, self.total

    def image(self, seed, data):
        """the arena before a call: pattern(seed) with the inputs laid over their payloads"""
        img = bytearray(pattern(seed, self.total))
        for r in self.regions:
            if r.role in ("in", "inout"):
                assert len(data[r.name]) == r.nbytes, (r.name, len(data[r.name]), r.nbytes)
                img[r.off:r.end] = data[r.name]
        return bytes(img)

    def outputs(self, img):
        return {r.name: img[r.off:r.end] for r in self.regions if r.role in ("out", "inout")}


def _first_diff(a, b, lo, hi):
    if a[lo:hi] == b[lo:hi]:
        return None
    x = np.frombuffer(a, dtype=np.uint8, count=hi - lo, offset=lo) != np.frombuffer(b, dtype=np.uint8, count=hi - lo, offset=lo)
    return lo + int(np.argmax(x))


def check(layout, before, after):
    """-> [(kind, region name, offset of the first offending byte)]: a guard byte that changed ("guard", named by the payload
    nearest to it), a byte of a read-only payload that changed ("input")"""
    assert len(before) == len(after) == layout.total
    found = []
    for k, (lo, hi) in enumerate(layout.guards()):
        at = _first_diff(before, after, lo, hi)
        if at is not None:
            regs = layout.regions
            near = regs[k - 1] if k == len(regs) or (k > 0 and at - regs[k - 1].end < regs[k].off - at) else regs[k]
            found.append(("guard", near.name, at))
    for r in layout.regions:
        if r.role == "in":
            at = _first_diff(before, after, r.off, r.end)
            if at is not None:
                found.append(("input", r.name, at))
    return found


def compare_runs(layout, after_a, after_b):
    """-> [("differs", region name, offset)]: the first output byte that is not the same after both runs -- never written (the
    prefills differ everywhere), or computed from bytes the call was not given"""
    found = []
    for r in layout.regions:
        if r.role in ("out", "inout"):
            at = _first_diff(after_a, after_b, r.off, r.end)
            if at is not None:
                found.append(("differs", r.name, at))
    return found


# ---- the header --------------------------------------------------------------------------------------------------------------------
def header_prototypes():
    """{entry: [pointer argument names]} of every sh_dev_* function the header declares (ctx excluded)"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(sh_dev_\w+)\s*\(([^)]*)\)\s*;", text):
        ptrs = []
        for a in args.split(","):
            a = a.strip()
            if ("*" in a or "[" in a) and not a.startswith("sh_ctx"):
                ptrs.append(re.findall(r"[A-Za-z_]\w*", a.split("[")[0])[-1])
        out[name] = ptrs
    return out


# ---- fields ------------------------------------------------------------------------------------------------------------------------
class Fam(object):
    """one of the three kernel families: the modulus, the element size and how its entries are named and called"""

    def __init__(self, key, name, esize):
        self.key, self.name, self.esize, self.p = key, name, esize, mc.MODULI[name]
        self.prefix = {"mimc": "sh_dev_", "mod": "sh_dev_mod_", "mod64": "sh_dev_mod64_"}[key]

    def enc(self, vals):
        return b"".join(int(v).to_bytes(self.esize, "little") for v in vals)

    def dec(self, raw):
        return [int.from_bytes(raw[i:i + self.esize], "little") for i in range(0, len(raw), self.esize)]

    def head(self):
        return {"mimc": (), "mod": (self.p.to_bytes(32, "big"),), "mod64": (self.p,)}[self.key]

    def root(self, n):
        return mc.root_of(self.name, n)

    def rootarg(self, n):
        w = self.root(n)
        return w if self.key == "mod64" else w.to_bytes(32, "big")

    def polyhead(self):
        """the modulus, a root of order 2^20 and its log: what the polynomial entries of the run-time fields take"""
        if self.key == "mimc":
            return ()
        return self.head() + (self.rootarg(1 << 20), 20)

    def rand(self, seed, n):
        """n seeded values; every fifth one is at or above p where the element leaves room (inputs may be unreduced)"""
        rnd, top = random.Random(seed), 1 << (8 * self.esize)
        out = [rnd.randrange(self.p) for _ in range(n)]
        for i in range(2, n, 5):
            if out[i] + self.p < top:
                out[i] += self.p
        return out

    def raw(self, seed, n):
        """n seeded elements as bytes, every bit random (any value of the element's width is an input and stands for its residue);
        numpy, so that the 2^20- and 2^22-element shapes take no Python loop"""
        return _stream(1000 + seed, n * self.esize).tobytes()

    def leaf(self, v):
        """the 32 bytes sh_dev_merkelize (MiMC: canonical) / _plain / mod64_merkelize (as stored) hash for a stored value"""
        return (v % self.p if self.key == "mimc" else v).to_bytes(32, "big")


MIMC, MOD, MOD64 = Fam("mimc", "mimc", 32), Fam("mod", "bn254", 32), Fam("mod64", "goldilocks", 8)
FAMS = (MIMC, MOD, MOD64)


def terms_of(sp, p):
    """(coefs wire, exps, counts) of a list of step polynomials: sorted monomial order, starks_amd.stark.pack_step_polys' layout"""
    counts, coefs, exps = [], [], bytearray()
    for poly in sp:
        items = sorted(poly.items())
        counts.append(len(items))
        for k, c in items:
            coefs.append(c % p)
            exps += bytes(k)
    return mc.wire(coefs), bytes(exps), (ctypes.c_uint32 * len(sp))(*counts)


LINEAR_3 = [{(1, 0, 0): 1, (0, 0, 0): 1}, {(1, 1, 0): 1}, {(1, 0, 0): 2, (0, 0, 1): 1}]  # X1' = X1 + 1, X2' = X1 X2, X3' = X3 + 2 X1
SYSTEMS = {1: sc.CUBIC_1, 2: sc.MIMC_2, 3: LINEAR_3, 9: sc.QUINTIC_9}


# ---- rows --------------------------------------------------------------------------------------------------------------------------
class Call(object):
    """one call of an entry at one shape: `data` = the bytes of every in / inout / hin payload (a callable(L, ctx) where they come
    from the library itself, e.g. honest proofs), invoke(L, ctx, ptr) -> status, model() -> {output name: ("bytes", b) or
    ("ints", fam, [..])} for the anchor, after(L, ctx) -> status of a follow-up call (sh_stark_status, sh_io_sync)"""

    def __init__(self, data, invoke, model=None, after=None):
        self.data, self.invoke, self.model, self.after = data, invoke, model, after


class Row(object):
    def __init__(self, entry, roles, shapes, build, polluter, cite, variant="", env=None, anchor=0, pinned=False):
        self.entry, self.roles, self.shapes, self.build, self.polluter, self.cite = entry, roles, shapes, build, polluter, cite
        self.variant, self.env, self.anchor, self.pinned = variant, env or {}, anchor, pinned
        self.id = entry + ("-" + variant if variant else "")

    def bufs(self, shape, space):
        """[(name, role, nbytes)] of the device ("dev") or host ("host") arena at a shape; lengths of in / hin come from the data"""
        out = []
        for arg, role in self.roles.items():
            kind, _, expr = role.partition(":")
            if space == "dev" and kind in ("in", "out", "inout") or space == "host" and kind in ("hin", "hout"):
                out.append((arg, {"hin": "in", "hout": "out"}.get(kind, kind), out_len(expr, shape) if expr else None))
        return out


def out_len(expr, shape):
    return int(eval(expr, {"__builtins__": {}, "max": max, "min": min}, dict(shape)))  # noqa: S307 -- the table's own expressions


ROWS = []


_PROTOS = header_prototypes()


def row(entry, roles, shapes, build, polluter, cite, **k):
    """adds a row; a "const" role of the shared role sets is kept only where the entry's prototype has that pointer (the packed-word
    entries take the modulus and the root by value), and an anchor given as a shape is looked up"""
    roles = {a: r for a, r in roles.items() if r != "const" or a in _PROTOS.get(entry, ())}
    if isinstance(k.get("anchor"), dict):
        k["anchor"] = shapes.index(k["anchor"])
    ROWS.append(Row(entry, roles, shapes, build, polluter, cite, **k))


def _fn(L, name):
    return getattr(L, name)


# transforms ---------------------------------------------------------------------------------------------------------------------------
def _ntt_shapes(n_ins):
    out = []
    for lg in range(14):
        n = 1 << lg
        for batch in (1, 3):
            for inverse in (0, 1):
                for n_in in sorted(set(f(n) for f in n_ins)):
                    out.append(dict(n=n, batch=batch, inverse=inverse, n_in=n_in))
    return out


def _ntt_build(F, inplace):
    def build(s):
        n, batch, inv, n_in = s["n"], s["batch"], s["inverse"], s["n_in"]
        vals = F.rand(n * 7 + batch + inv, batch * n_in)

        def invoke(L, ctx, p):
            dst = p["d_in"] if inplace else p["d_out"]
            if F.key == "mod64":
                return L.sh_dev_mod64_ntt(ctx, F.p, p["d_in"], n_in, dst, n, batch, F.root(n), inv)
            return _fn(L, F.prefix + "ntt")(ctx, *F.head(), p["d_in"], dst, n, batch, F.rootarg(n), inv)

        def model():
            out = []
            for b in range(batch):
                out += mc.transform(vals[b * n_in:(b + 1) * n_in], n, F.p, F.root(n), bool(inv))
            return {"d_in" if inplace else "d_out": ("ints", F, out)}

        return Call({"d_in": F.enc(vals)}, invoke, model)
    return build


_NTT_CITE = {
    "mimc": "ntt_kernels.cuh: the tuned tile is 4096 x 32 B, n <= 2^8 runs in one workgroup without a work buffer (starkhip.h)",
    "mod": "modntt_items.cuh: passes over LDS tiles of 2^t elements, t = STARKHIP_MODNTT_TILE_LOG (default 10)",
    "mod64": "ntt64_items.cuh: the plan rule, tiles of 2^t words, t = STARKHIP_MOD64_TILE_LOG (default 12), radix log t - min(4, t / 2)",
}
_NTT_ANCHOR = dict(n=1024, batch=1, inverse=0, n_in=1024)
for F in FAMS:
    full = [lambda n: n]
    short = [lambda n: 1, lambda n: n // 2 + 1, lambda n: n] if F.key == "mod64" else full
    knob = {"mod": {"STARKHIP_MODNTT_TILE_LOG": "3"}, "mod64": {"STARKHIP_MOD64_TILE_LOG": "3"}}.get(F.key)
    expr = "%d * batch * n" % F.esize
    for env, tag in ((None, ""), (knob, "tile3")):
        if tag and not knob:
            continue
        row(F.prefix + "ntt", {"d_in": "in", "d_out": "out:" + expr, "modulus": "const", "root": "const"}, _ntt_shapes(short),
            _ntt_build(F, False), "mimc_stark" if F.key != "mimc" else "mod_stark", _NTT_CITE[F.key], variant=tag, env=env,
            anchor=_NTT_ANCHOR)
        row(F.prefix + "ntt", {"d_in": "inout:" + expr, "d_out": "=d_in", "modulus": "const", "root": "const"}, _ntt_shapes(full),
            _ntt_build(F, True), "mimc_stark" if F.key != "mimc" else "mod_stark", _NTT_CITE[F.key], variant=("inplace-" + tag).strip("-"),
            env=env, anchor=_NTT_ANCHOR)


def _lde_build(s):
    steps, ext, cols = s["steps"], s["ext"], s["cols"]
    vals = MIMC.rand(steps * 3 + ext + cols, cols * steps)
    g2 = MIMC.root(steps * ext)

    def invoke(L, ctx, p):
        return L.sh_dev_lde(ctx, p["d_trace"], p["d_out"], steps, ext, cols, g2.to_bytes(32, "big"))

    def model():
        out, coef = [], []
        for c in range(cols):
            col = [v % MIMC.p for v in vals[c * steps:(c + 1) * steps]]
            out += pyoracle.low_degree_extension(col, g2, ext, MIMC.p)
            coef += mc.transform(col, steps, MIMC.p, pow(g2, ext, MIMC.p), True)
        return {"d_out": ("ints", MIMC, out), "d_trace": ("ints", MIMC, coef)}

    return Call({"d_trace": MIMC.enc(vals)}, invoke, model)


# n = steps * ext = 2^1 .. 2^13, each size with a short source (n_in = steps < n), steps from 1 (run_ntt's pad_copy branch at n = 2)
LDE_PAIRS = ((1, 2), (1, 4), (2, 2), (2, 4), (4, 4), (4, 8), (16, 4), (16, 8), (32, 8), (128, 2), (64, 8), (128, 8), (512, 2), (256, 8), (2048, 2),
             (512, 8), (4096, 2), (512, 16), (1024, 8))
row("sh_dev_lde", {"d_trace": "inout:32 * cols * steps", "d_out": "out:32 * cols * steps * ext", "g2": "const"},
    [dict(steps=s, ext=e, cols=c) for s, e in LDE_PAIRS for c in (1, 3)],
    _lde_build, "mod_stark", "api_ntt.hip: sh_dev_lde = run_ntt in place on d_trace, then run_ntt with n_in = steps: pad_copy for log_n <= 1, else the short-source first pass",
    anchor=dict(steps=16, ext=4, cols=3))


# conversions, fills and copies ------------------------------------------------------------------------------------------------------
COUNTS = [dict(n=n) for n in (1, 255, 256, 257)]
_WG = "kernels.hip: TPB = 256, one element per lane, `if (i >= n) return` tail of flat_grid_for"


def _from_wire_build(s):
    vals = MIMC.rand(s["n"], s["n"])
    return Call({"host_wire": mc.wire(vals)}, lambda L, ctx, p: L.sh_dev_from_wire(ctx, ctypes.cast(p["host_wire"], ctypes.c_char_p), p["d_limbs"], s["n"]),
                lambda: {"d_limbs": ("ints", MIMC, vals)})


def _to_wire_build(s):
    vals = MIMC.rand(s["n"] + 1, s["n"])
    return Call({"d_limbs": MIMC.enc(vals)}, lambda L, ctx, p: L.sh_dev_to_wire(ctx, p["d_limbs"], p["host_wire"], s["n"]),
                lambda: {"host_wire": ("bytes", mc.wire([v % MIMC.p for v in vals]))})


def _from_limbs_build(s):
    vals = MOD.rand(s["n"] + 2, s["n"])
    return Call({"d_limbs": MOD.enc(vals)}, lambda L, ctx, p: L.sh_dev_mod64_from_limbs(ctx, MOD64.p, p["d_limbs"], p["d_words"], s["n"]),
                lambda: {"d_words": ("bytes", MOD64.enc([v % MOD64.p for v in vals]))})


def _to_limbs_build(s):
    vals = [random.Random(s["n"]).getrandbits(64) for _ in range(s["n"])]
    return Call({"d_words": MOD64.enc(vals)}, lambda L, ctx, p: L.sh_dev_mod64_to_limbs(ctx, p["d_words"], p["d_limbs"], s["n"]),
                lambda: {"d_limbs": ("bytes", MOD.enc(vals))})


def _fill_seeded_build(s):
    seed = 0x1234 + s["n"]

    def model():
        return {"d_limbs": ("ints", MIMC, [pc.seeded(seed, i) for i in range(s["n"])])}
    return Call({}, lambda L, ctx, p: L.sh_dev_fill_seeded(ctx, p["d_limbs"], s["n"], seed), model)


def _fill_mimc_build(s):
    steps, batch, first, const = s["steps"], s["batch"], 5, 42

    def model():
        wit, inp = [], []
        for u in range(first, first + batch):
            tr = pyoracle.get_computational_trace([const, 3 + u], steps, sc.MIMC_2, MIMC.p)
            wit += tr[0] + tr[1]
            inp += [const, 3 + u]
        return {"d_witness": ("ints", MIMC, wit), "d_inputs": ("ints", MIMC, inp)}
    return Call({}, lambda L, ctx, p: L.sh_dev_fill_mimc_units(ctx, p["d_witness"], p["d_inputs"], steps, first, batch, const), model)


def _copy_build(s):
    raw = pattern(77, s["n"])
    return Call({"d_src": raw}, lambda L, ctx, p: L.sh_dev_copy(ctx, p["d_src"], p["d_dst"], s["n"]), lambda: {"d_dst": ("bytes", raw)})


def _dl2d_build(s):
    pitch, width, rows = s["pitch"], s["width"], s["rows"]
    raw = pattern(79, pitch * rows)
    return Call({"d_src": raw}, lambda L, ctx, p: L.sh_dev_download_2d(ctx, p["d_src"], pitch, p["host_dst"], width, rows),
                lambda: {"host_dst": ("bytes", b"".join(raw[r * pitch:r * pitch + width] for r in range(rows)))})


row("sh_dev_from_wire", {"host_wire": "hin", "d_limbs": "out:32 * n"}, COUNTS, _from_wire_build, "mod_stark", _WG)
row("sh_dev_to_wire", {"d_limbs": "in", "host_wire": "hout:32 * n"}, COUNTS, _to_wire_build, "mod_stark", _WG)
row("sh_dev_mod64_from_limbs", {"d_limbs": "in", "d_words": "out:8 * n"}, COUNTS, _from_limbs_build, "mimc_stark", "ntt64.hip: n64_from_limbs_kernel, N64_WG = 256 (ntt64_items.cuh), one value per lane, `if (i >= count) return`")
row("sh_dev_mod64_to_limbs", {"d_words": "in", "d_limbs": "out:32 * n"}, COUNTS, _to_limbs_build, "mimc_stark", "ntt64.hip: n64_to_limbs_kernel, N64_WG = 256 (ntt64_items.cuh), one word per lane, `if (i >= count) return`")
row("sh_dev_fill_seeded", {"d_limbs": "out:32 * n"}, COUNTS, _fill_seeded_build, "mod_stark", _WG)
row("sh_dev_fill_mimc_units", {"d_witness": "out:64 * batch * steps", "d_inputs": "out:64 * batch"},
    [dict(steps=st, batch=b) for st in (1, 2, 300) for b in (1, 3, 63, 64, 65)], _fill_mimc_build, "mod_stark",
    "kernels.hip: fill_mimc_units_kernel, one unit per lane of a 64-lane workgroup (grid (batch + 63) / 64), `if (b >= batch) return`; steps is a "
    "serial loop inside the lane", anchor=dict(steps=300, batch=65))
row("sh_dev_copy", {"d_src": "in", "d_dst": "out:n"}, COUNTS, _copy_build, "mod_stark", "ctx.hip: sh_dev_copy is one hipMemcpyAsync of `bytes`")
row("sh_dev_download_2d", {"d_src": "in", "host_dst": "hout:width * rows"},
    [dict(pitch=pt, width=w, rows=r) for pt, w in ((96, 64), (1000, 33)) for r in (1, 3)], _dl2d_build, "mod_stark",
    "ctx.hip: sh_dev_download_2d is one hipMemcpy2DAsync, destination pitch = width")

# 1, the direct-copy threshold of 64 KiB on both sides, and the PIN_CHUNK = 8 MiB boundaries of the double-buffered staging loop
COPY_BYTES = (1, 65535, 65536, 8 << 20, (8 << 20) + 1, (16 << 20) + 5)
_COPY_CITE = "ctx.hip: h2d / d2h copy pageable memory directly below (size_t)64 << 10 bytes and through the two pinned slots of PIN_CHUNK = 8 << 20 above"


def _upload_build(s):
    raw = pattern(81, s["n"])
    return Call({"host_src": raw}, lambda L, ctx, p: L.sh_dev_upload(ctx, ctypes.cast(p["host_src"], ctypes.c_char_p), p["d_dst"], s["n"]),
                lambda: {"d_dst": ("bytes", raw)})


def _download_build(name):
    def build(s):
        raw = pattern(83, s["n"])
        return Call({"d_src": raw}, lambda L, ctx, p: _fn(L, name)(ctx, p["d_src"], p["host_dst"], s["n"]), lambda: {"host_dst": ("bytes", raw)},
                    after=(lambda L, ctx: L.sh_io_sync(ctx)) if name.endswith("async") else None)
    return build


row("sh_dev_upload", {"host_src": "hin", "d_dst": "out:n"}, [dict(n=n) for n in COPY_BYTES], _upload_build, "mod_stark", _COPY_CITE, anchor=4)
row("sh_dev_download", {"d_src": "in", "host_dst": "hout:n"}, [dict(n=n) for n in COPY_BYTES], _download_build("sh_dev_download"), "mod_stark",
    _COPY_CITE, anchor=4)
row("sh_dev_download_async", {"d_src": "in", "host_dst": "hout:n"}, [dict(n=n) for n in COPY_BYTES[:5]], _download_build("sh_dev_download_async"),
    "mod_stark", "ctx.hip: sh_dev_download_async is one copy on the copy stream into page-locked memory, finished by sh_io_sync", anchor=4,
    pinned=True)


# trees and the fold -----------------------------------------------------------------------------------------------------------------
def _tree(F, vals):
    nodes = pyoracle.merkelize([F.leaf(v) for v in vals])
    return b"\0" * 32 + b"".join(nodes[1:])


def _merkle_build(F, name):
    def build(s):
        n, batch = s["n"], s["batch"]
        raw = F.raw(n + batch, n * batch)
        vals = F.dec(raw) if n <= 16 else None  # the model runs at the anchor shape only
        return Call({"d_values" if F.key != "mod64" else "d_words": raw},
                    lambda L, ctx, p: _fn(L, name)(ctx, p["d_values" if F.key != "mod64" else "d_words"], n, batch, p["d_nodes"]),
                    lambda: {"d_nodes": ("bytes", b"".join(_tree(F, vals[b * n:(b + 1) * n]) for b in range(batch)))})
    return build


TREE_SHAPES = [dict(n=n, batch=b) for n in (4, 16, 1024, 1 << 13, 1 << 16) for b in (1, 3)]
_TREE_CITE = "kernels.hip: MERKLE_SERIAL_MAX_LEAVES = 1 << 15: trees of up to that many leaves in all (n batch) start in serial form"
row("sh_dev_merkelize", {"d_values": "in", "d_nodes": "out:64 * batch * n"}, TREE_SHAPES, _merkle_build(MIMC, "sh_dev_merkelize"), "mod_stark",
    _TREE_CITE, anchor=3)
row("sh_dev_merkelize_plain", {"d_values": "in", "d_nodes": "out:64 * batch * n"}, TREE_SHAPES, _merkle_build(MOD, "sh_dev_merkelize_plain"),
    "mimc_stark", _TREE_CITE, anchor=3)
row("sh_dev_mod64_merkelize", {"d_words": "in", "d_nodes": "out:64 * batch * n"}, TREE_SHAPES, _merkle_build(MOD64, "sh_dev_mod64_merkelize"),
    "mimc_stark", _TREE_CITE, anchor=3)


def _fold_build(s):
    n, batch = s["n"], s["batch"]
    vals = MIMC.rand(n * 5 + batch, n * batch)
    trees = [_tree(MIMC, vals[b * n:(b + 1) * n]) for b in range(batch)]
    w = MIMC.root(n)

    def model():
        xs, out = pyoracle.get_power_cycle(w, MIMC.p), []
        for b in range(batch):
            out += pyoracle.fri_fold([v % MIMC.p for v in vals[b * n:(b + 1) * n]], xs, int.from_bytes(trees[b][32:64], "big"), MIMC.p)
        return {"d_column": ("ints", MIMC, out)}
    return Call({"d_values": MIMC.enc(vals), "d_nodes": b"".join(trees)},
                lambda L, ctx, p: L.sh_dev_fri_fold(ctx, p["d_values"], p["d_nodes"], n, batch, w.to_bytes(32, "big"), p["d_column"]), model)


row("sh_dev_fri_fold", {"d_values": "in", "d_nodes": "in", "root": "const", "d_column": "out:8 * batch * n"},
    [dict(n=n, batch=b) for n in (4, 16, 4096) for b in (1, 3)], _fold_build, "mod_stark", "kernels.hip: one row of four per lane, " + _WG, anchor=3)


# FRI provers ------------------------------------------------------------------------------------------------------------------------
FRI_SHAPES = [dict(n=n, md=md, batch=b, samples=40) for n, md in ((16, 8), (64, 32), (4096, 1024)) for b in (1, 3)]
_FRI_CITE = "api_fri.hip / modfri.hip: rounds while maxdeg_plus_1 > 16, proof stride = sh_fri_proof_len(n, maxdeg_plus_1, samples)"


def _fri_build(F, name, short):
    def build(s):
        n, md, batch, samples = s["n"], s["md"], s["batch"], s["samples"]
        nc = md - 3 if short else n  # the polynomial's own length where the entry takes n_coeffs, else zero-padded to n
        vals = []
        for b in range(batch):
            co = F.rand(n + md + b, md - 3)
            vals += co + [0] * (nc - len(co))

        def invoke(L, ctx, p):
            a = (p["d_coeffs"],) + ((nc,) if short else ()) + (n, F.rootarg(n), md, 0, samples, batch, p["d_proof"])
            return _fn(L, name)(ctx, *F.head(), *a)

        def model():
            flat = b"".join(pyoracle.proof_flat(pyoracle.prove_low_degree(vals[b * nc:(b + 1) * nc], F.root(n), md, p=F.p,
                                                                           fri_spot_check_security_factor=samples)) for b in range(batch))
            return {"d_proof": ("bytes", flat)}
        return Call({"d_coeffs": F.enc(vals)}, invoke, model)
    return build


for F, name, short in ((MIMC, "sh_dev_fri_prove", False), (MIMC, "sh_dev_fri_prove_coeffs", True), (MOD, "sh_dev_mod_fri_prove", True),
                       (MOD64, "sh_dev_mod64_fri_prove", True)):
    row(name, {"d_coeffs": "in", "modulus": "const", "root": "const", "d_proof": "out:batch * proof_len"}, FRI_SHAPES,
        _fri_build(F, name, short), "mod_stark" if F.key == "mimc" else "mimc_stark", _FRI_CITE, anchor=3)


# STARK provers, witness generators ------------------------------------------------------------------------------------------------------
STARK_SHAPES = [dict(steps=st, ext=e, width=w, batch=b, samples=8) for st, e, w in ((8, 8, 2), (32, 4, 3), (8, 8, 9)) for b in (1, 3)]
_STARK_CITE = "api_stark.hip / modstark.hip / mod64stark.hip: proof stride = sh_stark_proof_len(steps, ext, width, degree, samples); width <= 9"


def _stark_inputs(F, width, batch, seed):
    rnd = random.Random(seed)
    return [[rnd.randrange(F.p) for _ in range(width)] for _ in range(batch)]


def _stark_build(F, name):
    def build(s):
        steps, ext, width, batch, samples = s["steps"], s["ext"], s["width"], s["batch"], s["samples"]
        sp = SYSTEMS[width]
        inputs = _stark_inputs(F, width, batch, steps + width)
        wits = [pyoracle.get_computational_trace(i, steps, sp, F.p) for i in inputs]
        coefs, exps, counts = terms_of(sp, F.p)

        def invoke(L, ctx, p):
            return _fn(L, name)(ctx, *F.head(), p["d_witness"], p["d_inputs"], steps, ext, width, coefs, exps, counts, samples, batch, p["d_proof"])

        def model():
            return {"d_proof": ("bytes", b"".join(pyoracle.stark_flat(pyoracle.mk_stark_proof(w, i, sp, steps, ext, p=F.p, samples=samples))
                                                  for w, i in zip(wits, inputs)))}
        return Call({"d_witness": F.enc([v for w in wits for col in w for v in col]), "d_inputs": F.enc([v for i in inputs for v in i])},
                    invoke, model, after=lambda L, ctx: L.sh_stark_status(ctx))
    return build


def _witness_build(F, name):
    def build(s):
        steps, width, batch = s["steps"], s["width"], s["batch"]
        sp = SYSTEMS[width]
        inputs = _stark_inputs(F, width, batch, steps * 11 + width)
        coefs, exps, counts = terms_of(sp, F.p)

        def model():
            return {"d_witness": ("bytes", F.enc([v for i in inputs for col in pyoracle.get_computational_trace(i, steps, sp, F.p) for v in col]))}
        return Call({"d_inputs": F.enc([v for i in inputs for v in i])},
                    lambda L, ctx, p: _fn(L, name)(ctx, *F.head(), p["d_inputs"], steps, width, coefs, exps, counts, batch, p["d_witness"]), model)
    return build


_TERMS = {"term_coefs": "const", "term_exps": "const", "term_counts": "const", "modulus": "const"}
WITNESS_SHAPES = [dict(steps=st, width=w, batch=b) for st in (1, 2, 65, 300) for w in (1, 2, 9) for b in (1, 65)]
for F in FAMS:
    plen = "batch * proof_len"
    # d_witness is `void*` in the prototype and documented read-only: declared "in", so any change to it is reported
    row(F.prefix + "stark_prove", dict(_TERMS, d_witness="in", d_inputs="in", d_proof="out:" + plen), STARK_SHAPES,
        _stark_build(F, F.prefix + "stark_prove"), "mod_stark" if F.key == "mimc" else "mimc_stark", _STARK_CITE)
    row(F.prefix + "stark_witness", dict(_TERMS, d_inputs="in", d_witness="out:%d * batch * width * steps" % F.esize), WITNESS_SHAPES,
        _witness_build(F, F.prefix + "stark_witness"), "mod_stark" if F.key == "mimc" else "mimc_stark",
        "witness.hip / modwitness.hip / mod64witness.hip: one (unit, dimension group) per lane; at the default slice (WI_ / MWI_ / M6W_SLICE_PRODUCTS "
        "over the plan's cost per step, at least 455 steps for these systems) every shape is ONE dispatch", anchor=14)
    # the resumed dispatches (k0 > 0 re-reads row k0 - 1 from d_witness itself): 65 is one step past a slice of 64, 300 crosses four
    row(F.prefix + "stark_witness", dict(_TERMS, d_inputs="in", d_witness="out:%d * batch * width * steps" % F.esize), WITNESS_SHAPES,
        _witness_build(F, F.prefix + "stark_witness"), "mod_stark" if F.key == "mimc" else "mimc_stark",
        "api_stark.hip / api_modstark.hip / api_mod64stark.hip: `for (k0 = 0; k0 < steps; k0 = k1)` with k1 - k0 = plan.slice = STARKHIP_WITNESS_SLICE "
        "= 64: steps 65 and 300 run 2 and 5 dispatches, each resuming from the last row the previous one stored", variant="slice64",
        env={"STARKHIP_WITNESS_SLICE": "64"}, anchor=dict(steps=300, width=2, batch=1))


# batch verifiers --------------------------------------------------------------------------------------------------------------------
VERIFY_SHAPES = [dict(batch=b) for b in (1, 3, 65)]
_VERIFY_CITE = "verify_dev.hip / modverify_dev.hip: one proof per workgroup, d_status = batch int32"


def _stark_verify_build(F, name):
    steps, ext, width, samples, sp = 8, 8, 2, 8, sc.MIMC_2

    def build(s):
        batch = s["batch"]
        inputs = _stark_inputs(F, width, batch, 99)
        wits = [pyoracle.get_computational_trace(i, steps, sp, F.p) for i in inputs]
        coefs, exps, counts = terms_of(sp, F.p)
        head = F.head()

        def proofs(L, ctx):
            plen = L.sh_stark_proof_len(steps, ext, width, 3, samples)
            out = ctypes.create_string_buffer(plen * batch)
            host = _fn(L, name.replace("_dev", "").replace("verify", "prove"))
            rc = host(ctx, *head, mc.wire([v for w in wits for col in w for v in col]), mc.wire([v for i in inputs for v in i]), steps, ext, width,
                      coefs, exps, counts, samples, batch, out, len(out))
            assert rc == OK, (rc, L.sh_last_error(ctx))
            return out.raw

        def invoke(L, ctx, p):
            return _fn(L, name)(ctx, *head, p["d_proof"], p["d_inputs"], p["d_outputs"], 1, steps, ext, width, coefs, exps, counts, samples, batch,
                                p["d_status"])
        return Call({"d_proof": proofs, "d_inputs": MIMC.enc([v for i in inputs for v in i]), "d_outputs": MIMC.enc([col[-1] for w in wits for col in w])},
                    invoke, lambda: {"d_status": ("bytes", b"\0" * (4 * batch))})
    return build


def _fri_verify_build(F, name):
    n, md, samples = 64, 32, 40

    def build(s):
        batch = s["batch"]
        coeffs = [F.rand(500 + b, md - 3) for b in range(batch)]
        head = F.head()

        def proofs(L, ctx):
            plen = L.sh_fri_proof_len(n, md, samples)
            out = ctypes.create_string_buffer(plen * batch)
            host = _fn(L, name.replace("_dev", "").replace("verify", "prove"))
            rc = host(ctx, *head, mc.wire([v for c in coeffs for v in c]), md - 3, n, F.rootarg(n), md, 0, samples, batch, out, len(out))
            assert rc == OK, (rc, L.sh_last_error(ctx))
            return out.raw
        roots = b"".join(pyoracle.merkelize(mc.transform(c, n, F.p, F.root(n)))[1] for c in coeffs)

        def invoke(L, ctx, p):
            return _fn(L, name)(ctx, *head, p["d_proof"], p["d_merkle_roots"], n, F.rootarg(n), md, 0, samples, batch, p["d_status"])
        return Call({"d_proof": proofs, "d_merkle_roots": roots}, invoke, lambda: {"d_status": ("bytes", b"\0" * (4 * batch))})
    return build


for F in (MIMC, MOD):
    row(F.prefix + "stark_verify", dict(_TERMS, d_proof="in", d_inputs="in", d_outputs="in", d_status="out:4 * batch"), VERIFY_SHAPES,
        _stark_verify_build(F, F.prefix + "stark_verify"), "mod_stark" if F.key == "mimc" else "mimc_stark", _VERIFY_CITE, anchor="all")
    row(F.prefix + "fri_verify", {"modulus": "const", "root": "const", "d_proof": "in", "d_merkle_roots": "in", "d_status": "out:4 * batch"},
        VERIFY_SHAPES, _fri_verify_build(F, F.prefix + "fri_verify"), "mod_stark" if F.key == "mimc" else "mimc_stark", _VERIFY_CITE, anchor="all")


# batch inversion --------------------------------------------------------------------------------------------------------------------
INV_TILE = {"mimc": (1024, 256), "mod": (512, 256), "mod64": (2048, 1024)}  # values / rows per tile: inv_items.cuh, modpoly_items.cuh, mod64poly_items.cuh
_INV_CITE = {
    "mimc": "inv_items.cuh: IV_LANES x IV_CHUNK = 1024 values, IV_LANES x IV_ROW_CHUNK = 256 rows per tile, one product-tree level per power of it",
    "mod": "modpoly_items.cuh: MP_IV_LANES x MP_IV_CHUNK = 512 values, MP_IV_LANES x MP_IV_ROW_CHUNK = 256 rows per tile",
    "mod64": "mod64poly_items.cuh: M6P_IV_LANES x M6P_IV_CHUNK = 2048 values, M6P_IV_LANES x M6P_IV_ROW_CHUNK = 1024 rows per tile",
}


def _level_counts(T):
    return [dict(n=n) for n in (1, T - 1, T, T + 1, T * T + 1)]


def _inv_build(F, inplace):
    def build(s):
        n = s["n"]
        e, raw = F.esize, bytearray(F.raw(n, n))
        raw[n // 2 * e:(n // 2 + 1) * e] = bytes(e)  # a zero: its inverse is 0
        if n > 1:
            raw[:e] = F.enc([F.p])  # and the modulus itself, zero as a residue (64-bit family: p; 256-bit: p as stored)
        raw = bytes(raw)
        return Call({"d_in": raw},
                    lambda L, ctx, p: _fn(L, F.prefix + "multi_inv")(ctx, *F.head(), p["d_in"], p["d_in"] if inplace else p["d_out"], n),
                    lambda: {"d_in" if inplace else "d_out": ("bytes", F.enc(pc.multi_inv(F.p, F.dec(raw))))})
    return build


def _interp_build(F, alias):
    def build(s):
        rows = s["n"]
        e, xs, ys = F.esize, bytearray(F.raw(rows * 3, 4 * rows)), F.raw(rows * 3 + 1, 4 * rows)
        xs[e:2 * e] = xs[:e]  # a repeated x: its zero denominators count as 1
        xs, out = bytes(xs), alias or "d_coeffs"
        return Call({"d_xs": xs, "d_ys": ys},
                    lambda L, ctx, p: _fn(L, F.prefix + "multi_interp_4")(ctx, *F.head(), p["d_xs"], p["d_ys"], rows, p[out]),
                    lambda: {out: ("bytes", F.enc(pc.multi_interp_4(F.p, F.dec(xs), F.dec(ys))))})
    return build


for F in FAMS:
    T, TR = INV_TILE[F.key]
    pol, e = "mod_stark" if F.key == "mimc" else "mimc_stark", F.esize
    row(F.prefix + "multi_inv", {"modulus": "const", "d_in": "in", "d_out": "out:%d * n" % e}, _level_counts(T), _inv_build(F, False), pol, _INV_CITE[F.key], anchor=3)
    row(F.prefix + "multi_inv", {"modulus": "const", "d_in": "inout:%d * n" % e, "d_out": "=d_in"}, _level_counts(T), _inv_build(F, True), pol, _INV_CITE[F.key],
        variant="inplace", anchor=3)
    for alias in (None, "d_xs", "d_ys"):
        roles = {"modulus": "const", "d_xs": "in", "d_ys": "in", "d_coeffs": "out:%d * n" % (4 * e)}
        if alias:
            roles.update({alias: "inout:%d * n" % (4 * e), "d_coeffs": "=" + alias})
        row(F.prefix + "multi_interp_4", roles, _level_counts(TR), _interp_build(F, alias), pol, _INV_CITE[F.key], variant="over-" + alias if alias else "", anchor=1)


# polynomial arithmetic and evaluation -------------------------------------------------------------------------------------------------
_POLY_CITE = ("poly_items.cuh: the drivers shared by the three families; every transform is the next power of two, pointwise kernels are "
              "one element per lane with `if (g < total)` tails, pairs of 8-byte words go out as 16-byte stores where aligned16 holds")
_PH = {"modulus": "const", "root": "const"}


def _mul_build(F):
    def build(s):
        a, b = F.rand(s["n_a"], s["n_a"]), F.rand(s["n_b"] + 1000, s["n_b"])
        return Call({"d_a": F.enc(a), "d_b": F.enc(b)},
                    lambda L, ctx, p: _fn(L, F.prefix + "poly_mul")(ctx, *F.polyhead(), p["d_a"], len(a), p["d_b"], len(b), p["d_out"]),
                    lambda: {"d_out": ("bytes", F.enc(pc.mul(F.p, a, b)))})
    return build


def _divmod_build(F):
    def build(s):
        a, b = F.rand(s["n_a"], s["n_a"]), F.rand(s["n_b"] + 1000, s["n_b"])
        b[-1] = b[-1] % F.p or 1

        def model():
            q, r = pc.divmod_(F.p, a, b)
            return {"d_q": ("bytes", F.enc(q)), "d_r": ("bytes", F.enc(r))}
        return Call({"d_a": F.enc(a), "d_b": F.enc(b)},
                    lambda L, ctx, p: _fn(L, F.prefix + "poly_divmod")(ctx, *F.polyhead(), p["d_a"], len(a), p["d_b"], len(b), p["d_q"], p["d_r"]), model)
    return build


def _zpoly_build(F):
    def build(s):
        xs = F.rand(s["n"] + 3, s["n"])
        return Call({"d_xs": F.enc(xs)}, lambda L, ctx, p: _fn(L, F.prefix + "zpoly")(ctx, *F.polyhead(), p["d_xs"], len(xs), p["d_out"]),
                    lambda: {"d_out": ("bytes", F.enc(pc.zpoly(F.p, xs)))})
    return build


def _lagrange_build(F):
    def build(s):
        xs, ys = F.rand(s["n"] + 5, s["n"]), F.rand(s["n"] + 6, s["n"])
        return Call({"d_xs": F.enc(xs), "d_ys": F.enc(ys)},
                    lambda L, ctx, p: _fn(L, F.prefix + "lagrange_interp")(ctx, *F.polyhead(), p["d_xs"], p["d_ys"], len(xs), p["d_out"]),
                    lambda: {"d_out": ("bytes", F.enc(pc.lagrange(F.p, xs, ys)))})
    return build


def _eval_build(F):
    def build(s):
        n, m, batch = s["n"], s["m"], s["batch"]
        co, xs = F.rand(n + m, batch * n), F.rand(n + m + 1, m)
        xs[0] = 0
        return Call({"d_coefs": F.enc(co), "d_xs": F.enc(xs)},
                    lambda L, ctx, p: _fn(L, F.prefix + "poly_eval")(ctx, *F.polyhead(), p["d_coefs"], n, batch, p["d_xs"], m, p["d_out"]),
                    lambda: {"d_out": ("bytes", F.enc([pc.horner(F.p, co[b * n:(b + 1) * n], x) for b in range(batch) for x in xs]))})
    return build


EVAL_DIRECT = [dict(n=n, m=m, batch=b) for n in (1, 255, 256, 257, 1025) for m in (1, 3, 4, 5) for b in (1, 3)]
EVAL_TREE = [dict(n=1025, m=9, batch=1), dict(n=300, m=300, batch=1), dict(n=300, m=300, batch=3)]
for F in FAMS:
    pol, e = "mod_stark" if F.key == "mimc" else "mimc_stark", F.esize
    row(F.prefix + "poly_mul", dict(_PH, d_a="in", d_b="in", d_out="out:%d * (n_a + n_b - 1)" % e),
        [dict(n_a=a, n_b=b) for a, b in ((1, 1), (1, 5), (33, 32), (257, 300), (1025, 1))], _mul_build(F), pol, _POLY_CITE, anchor=2)
    row(F.prefix + "poly_divmod", dict(_PH, d_a="in", d_b="in", d_q="out:%d * max(n_a - n_b + 1, 0)" % e, d_r="out:%d * min(n_a, n_b - 1)" % e),
        [dict(n_a=a, n_b=b) for a, b in ((5, 9), (9, 1), (513, 257), (700, 300))], _divmod_build(F), pol, _POLY_CITE, anchor=3)
    row(F.prefix + "zpoly", dict(_PH, d_xs="in", d_out="out:%d * (n + 1)" % e), [dict(n=n) for n in (0, 1, 2, 255, 256, 257, 700)], _zpoly_build(F), pol,
        _POLY_CITE, anchor=5)
    row(F.prefix + "lagrange_interp", dict(_PH, d_xs="in", d_ys="in", d_out="out:%d * n" % e), [dict(n=n) for n in (1, 2, 65, 257, 700)],
        _lagrange_build(F), pol, _POLY_CITE, anchor=3)
    row(F.prefix + "poly_eval", dict(_PH, d_coefs="in", d_xs="in", d_out="out:%d * batch * m" % e), EVAL_DIRECT, _eval_build(F), pol,
        "poly_items.cuh PE_GROUP / modeval_items.cuh ME_GROUP / mod64eval_items.cuh M6E_GROUP = 4 points per lane, TPB = 256 lanes over the coefficients", anchor=29)
    row(F.prefix + "poly_eval", dict(_PH, d_coefs="in", d_xs="in", d_out="out:%d * batch * m" % e), EVAL_TREE, _eval_build(F), pol,
        "poly_items.cuh: the chunked scaled remainder tree, N = 2^ceil(log2 m), ceil(n / N) chunks per polynomial", variant="tree",
        env={"STARKHIP_EVAL_PATH": "tree"}, anchor=0)


def by_id():
    return {r.id: r for r in ROWS}


# ---- running a row on the GPU ------------------------------------------------------------------------------------------------------
class _Arena(object):
    """the device block and the host block of one call, their layouts and images"""

    def __init__(self, L, ctx, r, shape, data, seed):
        self.L, self.ctx = L, ctx
        dev = [(n, role, len(data[n]) if ln is None else ln) for n, role, ln in r.bufs(shape, "dev")]
        host = [(n, role, len(data[n]) if ln is None else ln) for n, role, ln in r.bufs(shape, "host")]
        self.dev, self.host = Layout(dev), Layout(host)
        self.dev_before, self.host_before = self.dev.image(seed, data), self.host.image(seed + 2, data)
        self.d, self.h, self.hbuf = ctypes.c_void_p(), ctypes.c_void_p(), None
        _ok(L, ctx, L.sh_dev_alloc(ctx, max(self.dev.total, 1), ctypes.byref(self.d)), "sh_dev_alloc")
        if self.dev.total:
            _ok(L, ctx, L.sh_dev_upload(ctx, self.dev_before, self.d, self.dev.total), "sh_dev_upload")
        if self.host.total:
            if r.pinned:
                _ok(L, ctx, L.sh_host_alloc(ctx, self.host.total, ctypes.byref(self.h)), "sh_host_alloc")
            else:
                self.hbuf = ctypes.create_string_buffer(self.host.total)
                self.h = ctypes.c_void_p(ctypes.addressof(self.hbuf))
            ctypes.memmove(self.h, self.host_before, self.host.total)
        self.ptr = {g.name: ctypes.c_void_p(self.d.value + g.off) for g in self.dev.regions}
        self.ptr.update({g.name: ctypes.c_void_p(self.h.value + g.off) for g in self.host.regions})
        self.pinned = r.pinned

    def after(self):
        out = ctypes.create_string_buffer(max(self.dev.total, 1))
        if self.dev.total:
            _ok(self.L, self.ctx, self.L.sh_dev_download(self.ctx, self.d, out, self.dev.total), "sh_dev_download")
        return out.raw[:self.dev.total], ctypes.string_at(self.h, self.host.total) if self.host.total else b""

    def free(self):
        self.L.sh_dev_free(self.ctx, self.d)
        if self.pinned and self.h:
            self.L.sh_host_free(self.ctx, self.h)


class Failure(Exception):
    pass


def _ok(L, ctx, rc, what):
    if rc != OK:
        raise Failure("%s returned %d: %s" % (what, rc, L.sh_last_error(ctx).decode(errors="replace")))


def _one_run(L, ctx, r, shape, call, data, seed):
    if "proof_len" in " ".join(r.roles.values()):
        s = shape
        shape = dict(shape, proof_len=(L.sh_fri_proof_len(s["n"], s["md"], s["samples"]) if "md" in s else
                                       L.sh_stark_proof_len(s["steps"], s["ext"], s["width"], sc.degree_of(SYSTEMS[s["width"]]), s["samples"])))
    a = _Arena(L, ctx, r, shape, data, seed)
    try:
        _ok(L, ctx, call.invoke(L, ctx, a.ptr), r.entry)
        _ok(L, ctx, L.sh_sync(ctx), "sh_sync")
        if call.after:
            _ok(L, ctx, call.after(L, ctx), "the call after " + r.entry)
        dev_after, host_after = a.after()
    finally:
        a.free()
    found = [("dev",) + f for f in check(a.dev, a.dev_before, dev_after)] + [("host",) + f for f in check(a.host, a.host_before, host_after)]
    return a, dev_after, host_after, found


def _new_ctx(L):
    ctx = ctypes.c_void_p()
    rc = L.sh_ctx_create(int(os.environ.get("STARKHIP_DEVICE", "0") or 0), ctypes.byref(ctx))
    if rc != OK:
        raise Failure("sh_ctx_create returned %d" % rc)
    return ctx


def run_shape(L, r, k):
    """runs A and B of shape k of row r on a context of its own -> a list of findings, empty when the contract holds"""
    shape, found = r.shapes[k], []
    call = r.build(shape)
    data = dict(call.data)
    if any(callable(v) for v in data.values()):  # inputs the library makes (honest proofs) come from a context of their own, gone before run A
        ctx = _new_ctx(L)
        try:
            data = {n: (v(L, ctx) if callable(v) else v) for n, v in data.items()}
        finally:
            L.sh_ctx_destroy(ctx)
    ctx = _new_ctx(L)
    try:
        a, dev_a, host_a, f = _one_run(L, ctx, r, shape, call, data, 1)
        found += [("A",) + x for x in f]
        POLLUTERS[r.polluter](L, ctx)
        b, dev_b, host_b, f = _one_run(L, ctx, r, shape, call, data, 2)
        found += [("B",) + x for x in f]
        found += [("A/B", "dev") + x for x in compare_runs(a.dev, dev_a, dev_b)] + [("A/B", "host") + x for x in compare_runs(a.host, host_a, host_b)]
        if r.anchor == "all" or k == r.anchor:
            got = dict(a.dev.outputs(dev_a), **a.host.outputs(host_a))
            want = call.model()
            assert want, "the anchor shape has a model"
            for name, w in want.items():
                if w[0] == "ints":  # lazily reduced limbs: equal as residues
                    same = [v % w[1].p for v in w[1].dec(got[name])] == [v % w[1].p for v in w[2]]
                else:
                    same = got[name] == w[1]
                if not same:
                    found.append(("model", name, hashlib.sha256(got[name]).hexdigest()[:16]))
    finally:
        L.sh_sync(ctx)
        L.sh_ctx_destroy(ctx)
    return [(r.id, tuple(sorted(shape.items()))) + x for x in found]


def run_row(L, r):
    """every shape of the row in sequence; stops at the first call that does not return SH_OK (Failure), retries nothing"""
    found = []
    for k in range(len(r.shapes)):
        try:
            found += run_shape(L, r, k)
        except Failure as e:
            return found + [(r.id, tuple(sorted(r.shapes[k].items())), "status", str(e))]
    return found


# ---- polluters: a larger call of another family that leaves its own contents in the context's workspaces ---------------------------------
def _pollute(F, prove, witness):
    steps, ext, batch, sp = 256, 8, 4, sc.MIMC_2

    def run(L, ctx):
        coefs, exps, counts = terms_of(sp, F.p)
        plen = L.sh_stark_proof_len(steps, ext, 2, 3, 80)
        sizes = (64 * batch, 64 * batch * steps, plen * batch, 32 * 1500, 32 * 1500, 32 * 1500)
        ptrs = [ctypes.c_void_p() for _ in sizes]
        try:
            for ptr, nb in zip(ptrs, sizes):
                _ok(L, ctx, L.sh_dev_alloc(ctx, nb, ctypes.byref(ptr)), "sh_dev_alloc")
            di, dw, dp, dx, dy, do = ptrs
            _ok(L, ctx, L.sh_dev_upload(ctx, MIMC.enc([v for b in range(batch) for v in (42, 3 + b)]), di, 64 * batch), "sh_dev_upload")
            _ok(L, ctx, _fn(L, witness)(ctx, *F.head(), di, steps, 2, coefs, exps, counts, batch, dw), witness)
            _ok(L, ctx, _fn(L, prove)(ctx, *F.head(), dw, di, steps, ext, 2, coefs, exps, counts, 80, batch, dp), prove)
            _ok(L, ctx, L.sh_dev_fill_seeded(ctx, dx, 1500, 1), "sh_dev_fill_seeded")
            _ok(L, ctx, L.sh_dev_fill_seeded(ctx, dy, 1500, 2), "sh_dev_fill_seeded")
            _ok(L, ctx, _fn(L, F.prefix + "lagrange_interp")(ctx, *F.polyhead(), dx, dy, 1500, do), "lagrange_interp")
            _ok(L, ctx, L.sh_stark_status(ctx), "sh_stark_status")
        finally:
            L.sh_sync(ctx)
            for ptr in ptrs:
                if ptr:
                    L.sh_dev_free(ctx, ptr)
    return run


POLLUTERS = {
    "mimc_stark": _pollute(MIMC, "sh_dev_stark_prove", "sh_dev_stark_witness"),
    "mod_stark": _pollute(MOD, "sh_dev_mod_stark_prove", "sh_dev_mod_stark_witness"),
}
