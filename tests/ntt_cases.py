"""Cases, inputs and the exact reference for every NTT pass kernel of starks_amd/csrc/ntt.hip, as run one instantiation at a time by
tests/native/ntt_ops.hip.  Shared by tests/test_ntt_passes_host.py (CPU: the harness builds and refuses bad jobs, the grid reaches
every instantiation in the cross-compiled code object, the chooser agrees with choose_cell() below, the reference passes compose to
the C oracle's transform) and tests/test_gpu_ntt_passes.py (GPU: the whole grid, element for element).

THE REFERENCE is the definition of a pass over Python integers (ntt_kernels.cuh; R = 2^log_R, tables are whatever the job holds):
  column pass: column c < total, j2 = c mod S, blk = c div S, x_i = src[blk R S + i S + j2] (with src_n: src[blk src_n + i S + j2]
      where i S + j2 < src_n, else 0);  dst[blk R S + k S + j2] = tw(k, j2) * sum_i x_i wR^(i k),
      tw = tw2[k S + j2], or lo[e] (direct), or lo[e & mask] * hi[e >> lb], e = j2 k.
  row pass: row c < total, b = c div P, r = c mod P, x_i = src[b n + r R + i] (with src_n, P = 1: src[b src_n + i], i < src_n, else 0);
      dst[b n + drev(r) + k P] = scale * sum_i x_i wR^(i k); drev takes the digits of r from the most significant end, widths
      dig[0 .. ndig), and places each at the bit offset given by the sum of the widths before it.
The R-point sums are the C oracle's fft (oracle/oracle.c), the products Python ints.  test_ntt_passes_host.py checks that these
passes, composed over a plan, are the oracle's whole transform.  Device values are any representative in [0, 2^256): they are
compared with the reference as residues mod p, exactly."""
import functools
import os
import random
import re
import subprocess

import native_harness

ROOT = native_harness.ROOT
CSRC = native_harness.CSRC
HARNESS = os.path.join(ROOT, "tests", "native", "ntt_ops.hip")
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"

P = 2**256 - 2**32 * 351 + 1
M = 2**256
EDGES = (0, 1, P - 1, P, P + 1, M - 1)
STALE = b"\xa5" * 32
TWO128 = 1 << 128
NARROW_HALF_TILES = 128
DEFAULT_KNOBS = {"tile_log": 10, "tile_forced": False, "tile_log_big": 11, "tile_logs": (0, 0, 0, 0, 0, 0, 0, 0), "xcd": 1, "narrow": 256}
REF_BUDGET_LOG = 14  # distinct source elements per job, about (the rest of a batch repeats them)


def root_of(n):
    return pow(7, (P - 1) // n, P)


# ---- which kernel a pass runs in: an independent statement of knobs.hpp's rules ------------------------------------------------------
def cell_exists(form, tile_log, log_R):
    """2048-element tiles for every radix 2^2 .. 2^11; 1024 to radix 2^10; 512 to 2^8; 4096 from 2^4; narrow: 1024 to 2^10, 512 to 2^8"""
    if not 2 <= log_R <= 11:
        return False
    if form == "narrow":
        return {10: log_R <= 10, 9: log_R <= 8}.get(tile_log, False)
    return {12: log_R >= 4, 11: True, 10: log_R <= 10, 9: log_R <= 8}.get(tile_log, False) if form == "tile" else False


def choose_cell(kn, log_R, last, total, log_n, log_S, pass_index):
    """-> (form, tile_log, xcd), the rules documented in knobs.hpp / DESIGN.md section 5"""
    forced = kn["tile_logs"][pass_index] if pass_index < 8 else 0

    def tiles(tl):
        return -(-total // (1 << (tl - log_R)))

    if log_R <= 10 and not forced and kn["narrow"] > 0 and 0 < tiles(10) <= kn["narrow"]:
        return ("narrow", 9 if log_R <= 8 and tiles(10) <= NARROW_HALF_TILES else 10, False)
    if log_R <= 8:
        if forced and cell_exists("tile", forced, log_R):
            tl = forced
        elif not last and log_R == 8 and log_S + 8 == log_n and log_S >= 16 and not kn["tile_forced"]:
            tl = 11
        else:
            tl = kn["tile_log"]
    else:
        ok = [t for t in (10, 11, 12) if cell_exists("tile", t, log_R)]
        tl = forced if forced in ok else kn["tile_log_big"] if kn["tile_log_big"] in ok else 11
    xcd = tiles(tl) >= 64 and (kn["xcd"] == 2 or (kn["xcd"] == 1 and tl - log_R < 2))
    return ("tile", tl, xcd)


# ---- the instantiations, read from a cross-compiled code object ----------------------------------------------------------------------
def instantiations(binary, workdir):
    """{("tile" | "narrow", log_R, log_T, last)} and whether ntt_tiny_kernel is there, from the symbol table of the gfx950 code object
    inside `binary` (an object file or a linked program)"""
    d = os.path.join(str(workdir), "code_objects")
    os.makedirs(d, exist_ok=True)
    local = os.path.join(d, "bin")
    with open(binary, "rb") as src, open(local, "wb") as dst:
        dst.write(src.read())
    subprocess.check_call([OBJDUMP, "--offloading", "bin"], cwd=d, stdout=subprocess.DEVNULL)
    found, tiny = set(), False
    for f in os.listdir(d):
        if "gfx950" not in f:
            continue
        syms = subprocess.run([OBJDUMP, "-t", "-C", f], cwd=d, capture_output=True, text=True, check=True).stdout
        for kind, r, t, last in re.findall(r"ntt_(narrow_pass|pass)_kernel<(\d+), (\d+), (true|false)>", syms):
            found.add(("narrow" if kind == "narrow_pass" else "tile", int(r), int(t), last == "true"))
        tiny |= "ntt_tiny_kernel" in syms
    return found, tiny


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
def _split_digits(log_P):
    """log_P as up to three unequal digit widths (most significant digit first)"""
    if log_P == 0:
        return ()
    if log_P <= 2:
        return (log_P,)
    if log_P <= 5:
        return (log_P - 1, 1)
    a = log_P // 2
    return (a, log_P - a - 1, 1) if a != log_P - a - 1 else (a + 1, log_P - a - 2, 1)


def _pass(name, log_R, last, form, tile_log, xcd, batch, log_S=0, log_pre=0, digs=(), tw=None, lb=0, rand_tw=False, wpow=1, scale=False,
          src_n=0, inplace=False, pass_index=0, src="dense", default=False):
    log_P = sum(digs)
    log_n = log_R + (log_P if last else log_S + log_pre)
    return {"name": name, "op": "pass", "log_R": log_R, "last": last, "form": form, "tile_log": tile_log, "xcd": xcd, "batch": batch,
            "log_S": log_S, "log_pre": log_pre, "digs": tuple(digs), "log_P": log_P, "log_n": log_n, "tw": tw, "lb": lb, "rand_tw": rand_tw,
            "wpow": wpow, "scale": scale, "src_n": src_n, "inplace": inplace, "pass_index": pass_index, "src": src, "default": default,
            "total": batch << (log_n - log_R)}


TW_KINDS = ("tw2", "direct", "split_below", "split_at")


def _tw_args(kind, log_R, log_S):
    """(tw, lb) of a table kind for a column pass of order R * S"""
    if kind == "split_below":
        return "split", max(1, (log_R + log_S) // 2)
    if kind == "split_at":
        return "split", log_R + log_S
    return kind, 0


@functools.lru_cache(None)
def cases():
    out = []
    count = [0]

    def col_kw(log_R, log_S):
        """the table kind, the root and whether the tables are random, taking turns over the column jobs"""
        i = count[0]
        count[0] += 1
        tw, lb = _tw_args(TW_KINDS[i % 4], log_R, log_S)
        return {"tw": tw, "lb": lb, "rand_tw": i % 3 == 0, "wpow": (1, 3, (1 << log_R) - 1)[i % 3]}

    tile_cells = [(tl, r) for tl in (9, 10, 11, 12) for r in range(2, 12) if cell_exists("tile", tl, r)]
    narrow_cells = [(tl, r) for tl in (9, 10) for r in range(2, 12) if cell_exists("narrow", tl, r)]
    # A. every tile instantiation: plain, and XCD-mapped over 67 .. 268 tiles (not a multiple of 8: the padded workgroups return)
    for tl, r in tile_cells:
        t = tl - r
        for xcd in (False, True):
            batch = 67 if xcd else 3
            log_S = max(2, t) + (count[0] % 2 if 2 <= t <= 8 else 0)  # 67 S / T tiles: 67, 134 or 268
            out.append(_pass("tile%d_r%d_col_%s" % (tl, r, "xcd" if xcd else "plain"), r, False, "tile", tl, xcd, batch, log_S=log_S,
                             **col_kw(r, log_S)))
            digs = _split_digits(max(t, 1) + (1 if xcd and t <= 1 else (tl + r) % 2))
            out.append(_pass("tile%d_r%d_row_%s" % (tl, r, "xcd" if xcd else "plain"), r, True, "tile", tl, xcd, batch, digs=digs,
                             scale=bool((tl + r + xcd) % 2), wpow=(1, 3, (1 << r) - 1)[(tl + r) % 3]))
    # B. every narrow instantiation: whole tiles, and 1.5 tiles (batch 3, half a tile per vector: the inactive-thread path)
    for tl, r in narrow_cells:
        t = tl - r
        out.append(_pass("narrow%d_r%d_col_full" % (tl, r), r, False, "narrow", tl, False, 4, log_S=t + 1, **col_kw(r, t + 1)))
        out.append(_pass("narrow%d_r%d_row_full" % (tl, r), r, True, "narrow", tl, False, 4, digs=_split_digits(t + 1), scale=bool(r % 2)))
        if t >= 1:
            out.append(_pass("narrow%d_r%d_col_partial" % (tl, r), r, False, "narrow", tl, False, 3, log_S=t - 1, **col_kw(r, t - 1)))
            out.append(_pass("narrow%d_r%d_row_partial" % (tl, r), r, True, "narrow", tl, False, 3, digs=_split_digits(t - 1),
                             scale=not r % 2, wpow=3))
    # C. every tile shape over 512 workgroups: both workgroup slots of every CU taken, waves free to drift apart
    for tl, r in tile_cells:
        t = tl - r
        if (tl + r) % 2:
            log_S = max(2, t)
            out.append(_pass("tile%d_r%d_col_wg512" % (tl, r), r, False, "tile", tl, False, 512 >> (log_S - t), log_S=log_S, **col_kw(r, log_S)))
        else:
            out.append(_pass("tile%d_r%d_row_wg512" % (tl, r), r, True, "tile", tl, False, 512, digs=_split_digits(t), wpow=3))
    # D. per radix, the argument forms; each in the cell the default knobs choose and in the tile cell they choose without the narrow form
    for r in range(2, 12):
        R = 1 << r
        variants = []
        for i, kind in enumerate(TW_KINDS):
            log_S = 2 + i
            tw, lb = _tw_args(kind, r, log_S)
            variants.append(("col_" + kind, dict(last=False, batch=2, log_S=log_S, tw=tw, lb=lb, rand_tw=i % 2 == 1, wpow=(1, 3, R - 1)[i % 3])))
        S, n = 8, R * 8
        for tag, src_n in (("1", 1), ("S-1", S - 1), ("S+1", S + 1), ("n/8+1", n // 8 + 1), ("n-1", n - 1)):
            variants.append(("col_srcn_" + tag, dict(last=False, batch=3, log_S=3, tw=("tw2", "direct")[src_n % 2], src_n=src_n,
                                                     rand_tw=tag == "S+1", wpow=R - 1)))
        variants.append(("col_inplace", dict(last=False, batch=3, log_S=2, tw="tw2", inplace=True, wpow=3)))
        variants.append(("col_blk", dict(last=False, batch=2, log_S=3, log_pre=2, tw="split", lb=r, pass_index=1, rand_tw=True)))
        variants.append(("col_probe", dict(last=False, batch=r + 3, log_S=2, tw="tw2", src="probe")))
        variants.append(("row_srcn_scale", dict(last=True, batch=5, src_n=R - 1, scale=True, wpow=R - 1)))
        variants.append(("row_srcn_1", dict(last=True, batch=3, src_n=1)))
        variants.append(("row_inplace", dict(last=True, batch=5, inplace=True, wpow=3)))
        variants.append(("row_ndig1", dict(last=True, batch=2, digs=(3,), scale=True)))
        variants.append(("row_ndig2", dict(last=True, batch=2, digs=(4, 2), wpow=3)))
        variants.append(("row_ndig3", dict(last=True, batch=1, digs=(5, 3, 2) if r <= 6 else (3, 1, 2), scale=True, wpow=R - 1)))
        variants.append(("row_probe", dict(last=True, batch=r + 3, src="probe")))
        for tag, kw in variants:
            kw = dict(kw)
            last, batch = kw.pop("last"), kw.pop("batch")
            shape = _pass("", r, last, "tile", 11, False, batch, **kw)
            seen = set()
            for knobs in (DEFAULT_KNOBS, dict(DEFAULT_KNOBS, narrow=0)):
                form, tl, xcd = choose_cell(knobs, r, last, shape["total"], shape["log_n"], shape["log_S"], shape["pass_index"])
                if (form, tl) in seen:
                    continue
                seen.add((form, tl))
                out.append(_pass("r%d_%s_%s%d" % (r, tag, form, tl), r, last, form, tl, xcd, batch, default=knobs is DEFAULT_KNOBS, **kw))
    # E. the one- and two-point transforms
    for n in (1, 2):
        for scale in (False, True):
            for batch in (1, 63, 64, 65, 4097):
                out.append({"name": "tiny%d_x%d%s" % (n, batch, "_scale" if scale else ""), "op": "tiny", "n": n, "batch": batch, "scale": scale})
    # F. the table kernels against exact powers: lo alone, lo * hi with lb below the order and at it
    for r, s, lb, hi in ((2, 2, 0, False), (5, 3, 0, False), (5, 3, 4, True), (8, 4, 12, True), (3, 9, 6, True), (11, 2, 13, True), (7, 0, 0, False)):
        out.append({"name": "tw2_r%d_s%d_%s" % (r, s, "lb%d" % lb if hi else "nohi"), "op": "tw2", "log_R": r, "log_S": s, "lb": lb, "hi": hi})
    for n, lb, hi in ((1, 0, False), (1000, 10, False), (1000, 4, True), (4096, 12, True), (4097, 6, True), (70000, 17, False), (70000, 8, True)):
        out.append({"name": "powers_%d_%s" % (n, "lb%d" % lb if hi else "nohi"), "op": "powers", "n": n, "lb": lb, "hi": hi})
    # G. zero padding
    for n_in in (0, 1, 15, 16):
        out.append({"name": "pad16_in%d" % n_in, "op": "pad", "n": 16, "n_in": n_in, "batch": 5})
    out.append({"name": "pad1000_in999_x67", "op": "pad", "n": 1000, "n_in": 999, "batch": 67})
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return [c for c in cases() if c["name"] == name][0]


def tiles_of(c):
    return -(-c["total"] // (1 << (c["tile_log"] - c["log_R"])))


def cells_of(c):
    """what a case covers"""
    op = c["op"]
    if op == "tiny":
        return {("tiny", c["n"], c["scale"], c["batch"])}
    if op in ("tw2", "powers"):
        return {(op, "hi" if c["hi"] else "nohi")}
    if op == "pad":
        return {("pad", {0: "0", 1: "1", c["n"] - 1: "n-1", c["n"]: "n"}[c["n_in"]])}
    r, tl, last, tiles = c["log_R"], c["tile_log"], c["last"], tiles_of(c)
    t = tl - r
    out = set()
    if c["form"] == "tile":
        if not c["xcd"]:
            out.add(("tile", r, t, last, "plain"))
            if tiles >= 512:
                out.add(("wg512", r, t))
        elif tiles >= 64 and tiles % 8:
            out.add(("tile", r, t, last, "xcd"))
    else:
        out.add(("narrow", r, t, last, "partial" if c["total"] % (1 << t) else "full"))
    if last:
        out.add(("row", r, "ndig%d" % len(c["digs"])))
        out.add(("row", r, "scale" if c["scale"] else "noscale"))
        if c["src_n"]:
            out.add(("row", r, "srcn"))
        if c["inplace"]:
            out.add(("row", r, "inplace"))
    else:
        n, S = 1 << c["log_n"], 1 << c["log_S"]
        kind = c["tw"] if c["tw"] != "split" else "split_at" if c["lb"] == r + c["log_S"] else "split_below"
        out.add(("col", r, kind))
        out.add(("col", r, "log_S", c["log_S"]))
        if c["rand_tw"]:
            out.add(("col", r, "rand_tw"))
        if c["src_n"]:
            out |= {("col", r, "srcn", tag) for tag, v in (("1", 1), ("S-1", S - 1), ("S+1", S + 1), ("n/8+1", n // 8 + 1), ("n-1", n - 1))
                    if v == c["src_n"]}
        if c["inplace"]:
            out.add(("col", r, "inplace"))
        if c["log_pre"]:
            out.add(("col", r, "blk"))
    if c["src"] == "probe":
        out.add(("row" if last else "col", r, "probe"))
    return out


def required_cells(insts):
    """every instantiation `insts` (instantiations()) plain and XCD-mapped, every narrow one whole and with a partial tile, every tile
    shape over 512 workgroups, and per radix the argument forms of the column and row passes"""
    out = set()
    for form, r, t, last in insts:
        if form == "tile":
            out |= {("tile", r, t, last, "plain"), ("tile", r, t, last, "xcd"), ("wg512", r, t)}
        else:
            out.add(("narrow", r, t, last, "full"))
            if t >= 1:
                out.add(("narrow", r, t, last, "partial"))
    for r in sorted({i[1] for i in insts}):
        out |= {("col", r, k) for k in TW_KINDS + ("rand_tw", "inplace", "blk", "probe")}
        out |= {("col", r, "srcn", s) for s in ("1", "S-1", "S+1", "n/8+1", "n-1")}
        out |= {("col", r, "log_S", s) for s in (2, 3, 4, 5)}
        out |= {("row", r, k) for k in ("ndig0", "ndig1", "ndig2", "ndig3", "scale", "noscale", "srcn", "inplace", "probe")}
    out |= {("tiny", n, s, b) for n in (1, 2) for s in (False, True) for b in (1, 63, 64, 65, 4097)}
    out |= {(op, h) for op in ("tw2", "powers") for h in ("hi", "nohi")}
    out |= {("pad", k) for k in ("0", "1", "n-1", "n")}
    return out


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _rng(c, what):
    return random.Random("%s/%s" % (c["name"], what))


def _w32(v):
    return int(v).to_bytes(32, "big")


def _wire(vals):
    return b"".join(map(_w32, vals))


def vec_len(c):
    return c["src_n"] or (1 << c["log_n"])


def distinct(c):
    """the number of distinct source vectors of a pass or tiny job; vector b of the batch is vector b mod distinct.  Odd, so that
    neighbouring columns / rows / vectors never hold the same values"""
    if c["op"] == "tiny":
        return min(c["batch"], 129)
    if c["src"] == "probe":
        return c["batch"]
    return min(c["batch"], max(3, (1 << REF_BUDGET_LOG) >> c["log_n"]) | 1)


def _place_edges(v, turn):
    L = len(v)
    for i in range(min(6, L)):
        v[L - 1 - i] = EDGES[(i + 3 + turn) % 6]
    for i in range(min(6, L)):
        v[i] = EDGES[(i + turn) % 6]
    if L > 1:
        v[L - 1] = EDGES[(3 + turn) % 6]


@functools.lru_cache(8)
def _sources(name):
    c = case(name)
    V, L = distinct(c), (c["n"] if c["op"] == "tiny" else vec_len(c))
    rng = _rng(c, "src")
    if c["op"] == "pass" and c["src"] == "probe":
        # one non-zero element per position class: the first point, the last, one per level bit of the row index i; one all-equal
        r, step = c["log_R"], 1 if c["last"] else 1 << c["log_S"]
        spots = [0, L - 1] + [(1 << b) * step + (0 if c["last"] else 1) for b in range(r)]
        vecs = []
        for s in spots:
            v = [0] * L
            v[s] = rng.randrange(1, M)
            vecs.append(v)
        vecs.append([rng.randrange(1, M)] * L)
        assert len(vecs) == V
        return vecs
    vecs = []
    for b in range(V):
        buf = rng.randbytes(32 * L)
        v = [int.from_bytes(buf[32 * i:32 * i + 32], "big") for i in range(L)]
        for _ in range(min(4, L // 8)):
            v[rng.randrange(L)] = P + rng.randrange(M - P)
        if b in (0, V - 1, (c["batch"] - 1) % V):
            _place_edges(v, b)
        vecs.append(v)
    return vecs


def sources(c):
    """the distinct source vectors (ints in [0, 2^256)): dense random ones with a few unreduced values, the edge set 0, 1, p-1, p, p+1,
    2^256-1 at the first and last positions of the first and last vector"""
    return _sources(c["name"])


@functools.lru_cache(8)
def _tables(name):
    c = case(name)
    rng = _rng(c, "tables")
    if c["op"] == "tiny":
        return {"scale": rng.randrange(2, P) if c["scale"] else None}
    if c["op"] in ("tw2", "powers"):
        order_log = c["log_R"] + c["log_S"] if c["op"] == "tw2" else max(1, (c["n"] - 1).bit_length())
        g = pow(root_of(1 << order_log), 3, P)
        span = 1 << order_log if c["op"] == "tw2" else c["n"]
        if not c["hi"]:
            return {"g": g, "lo": _powers(g, span), "hi": None}
        return {"g": g, "lo": _powers(g, min(span, 1 << c["lb"])), "hi": _powers(pow(g, 1 << c["lb"], P), ((span - 1) >> c["lb"]) + 1)}
    R = 1 << c["log_R"]
    wR = pow(root_of(R), c["wpow"], P)
    t = {"wR": wR, "wr": _powers(wR, R // 2), "tw2": None, "lo": None, "hi": None, "scale": None}
    if c["scale"]:
        t["scale"] = rng.randrange(2, P)
    if c["last"]:
        return t
    S, RS = 1 << c["log_S"], R << c["log_S"]
    g = pow(root_of(RS), 5, P)
    emax = (S - 1) * (R - 1)

    def table(n, base):
        return [rng.randrange(P) for _ in range(n)] if c["rand_tw"] else _powers(base, n)

    if c["tw"] == "tw2":
        if c["rand_tw"]:
            t["tw2"] = table(RS, None)
        else:
            rows = [_powers(pow(g, k, P), S) for k in range(R)]  # row k: (g^k)^j2
            t["tw2"] = [x for row in rows for x in row]
    elif c["tw"] == "direct":
        t["lo"] = table(emax + 1, g)
    else:
        lb = c["lb"]
        t["lo"] = table(min(emax, (1 << lb) - 1) + 1, g)
        t["hi"] = table((emax >> lb) + 1, pow(g, 1 << lb, P))
    return t


def _powers(g, n):
    out, x = [], 1
    for _ in range(n):
        out.append(x)
        x = x * g % P
    return out


def tables(c):
    return _tables(c["name"])


def tw_of(c, t):
    """the inter-pass factor tw(k, j2) of a column job, from its tables"""
    S = 1 << c["log_S"]
    if c["tw"] == "tw2":
        return lambda k, j2: t["tw2"][k * S + j2]
    if c["tw"] == "direct":
        return lambda k, j2: t["lo"][j2 * k]
    lb = c["lb"]
    mask = (1 << lb) - 1
    return lambda k, j2: t["lo"][(j2 * k) & mask] * t["hi"][(j2 * k) >> lb] % P


def job_input(name):
    c = case(name)
    if c["op"] == "pad":
        return b"".join(_wire(v[:c["n_in"]]) for v in pad_sources(c))
    t = tables(c)
    if c["op"] in ("tw2", "powers"):
        return _wire(t["lo"]) + _wire(t["hi"] or [])
    src = b"".join(_wire(v) for v in sources(c))
    if c["op"] == "tiny":
        return (_w32(t["scale"]) if c["scale"] else b"") + src
    parts = [b"".join(_w32(v) + _w32(v * TWO128 % P) for v in t["wr"])]
    parts += [_wire(t[k] or []) for k in ("tw2", "lo", "hi")]
    parts.append(_w32(t["scale"]) if c["scale"] else b"")
    return b"".join(parts) + src


def pad_sources(c):
    rng = _rng(c, "src")
    return [[rng.randrange(M) for _ in range(c["n"])] for _ in range(c["batch"])]


def job_line(c, inp, out, **override):
    """the harness's job line of case c; `override` replaces keys (the refusal tests)"""
    op = c["op"]
    if op == "pass":
        t = tables(c)
        d = c["digs"] + (0, 0, 0)
        k = {"log_R": c["log_R"], "last": int(c["last"]), "form": int(c["form"] == "narrow"), "tile_log": c["tile_log"], "xcd": int(c["xcd"]),
             "total": c["total"], "log_n": c["log_n"], "log_S": c["log_S"], "log_P": c["log_P"],
             "tw": {None: 0, "tw2": 1, "direct": 2, "split": 3}[c["tw"]], "lb": c["lb"] if c["tw"] == "split" else 0, "ndig": len(c["digs"]),
             "d0": d[0], "d1": d[1], "d2": d[2], "scale": int(c["scale"]), "src_n": c["src_n"], "pass_index": c["pass_index"],
             "inplace": int(c["inplace"]), "n_wr": len(t["wr"]), "n_tw2": len(t["tw2"] or []), "n_lo": len(t["lo"] or []),
             "n_hi": len(t["hi"] or []), "n_src": distinct(c) * vec_len(c)}
    elif op == "tiny":
        k = {"n": c["n"], "batch": c["batch"], "scale": int(c["scale"]), "n_src": distinct(c) * c["n"]}
    elif op == "pad":
        k = {"n": c["n"], "n_in": c["n_in"], "batch": c["batch"]}
    else:
        t = tables(c)
        k = {"lb": c["lb"], "n_lo": len(t["lo"]), "n_hi": len(t["hi"] or [])}
        k.update({"log_R": c["log_R"], "log_S": c["log_S"]} if op == "tw2" else {"n": c["n"]})
    k.update(override)
    return "%s name=%s in=%s out=%s %s" % (op, c["name"], inp, out, " ".join("%s=%d" % kv for kv in k.items()))


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def _dft(xs, R, wR):
    """sum_i x_i wR^(i k), k < R: the C oracle's R-point transform of the reduced inputs"""
    from oracle import coracle
    if R == 1:
        return [xs[0] % P]
    buf = coracle.fft_bytes(b"".join(_w32(x % P) for x in xs), R, wR)
    return [int.from_bytes(buf[32 * i:32 * i + 32], "big") for i in range(R)]


def drev(r, digs):
    sh, wl, acc = sum(digs), 0, 0
    for d in digs:
        sh -= d
        acc |= ((r >> sh) & ((1 << d) - 1)) << wl
        wl += d
    return acc


def ref_column(vec, log_n, log_R, log_S, wR, tw, src_n=0):
    """one vector through a column pass -> n residues"""
    n, R, S = 1 << log_n, 1 << log_R, 1 << log_S
    RS = R * S
    out = [None] * n
    for blk in range(n // RS):
        for j2 in range(S):
            if src_n:
                xs = [vec[blk * src_n + i * S + j2] if i * S + j2 < src_n else 0 for i in range(R)]
            else:
                xs = vec[blk * RS + j2:(blk + 1) * RS:S]
            X = _dft(xs, R, wR)
            for k in range(R):
                out[blk * RS + k * S + j2] = tw(k, j2) * X[k] % P
    return out


def ref_row(vec, log_n, log_R, digs, wR, scale=None, src_n=0):
    """one vector through the row pass -> n residues"""
    n, R = 1 << log_n, 1 << log_R
    Pn = n // R
    assert sum(digs) == log_n - log_R
    out = [None] * n
    for r in range(Pn):
        xs = [vec[i] if i < src_n else 0 for i in range(R)] if src_n else vec[r * R:(r + 1) * R]
        X = _dft(xs, R, wR)
        base = drev(r, digs)
        for k in range(R):
            out[base + k * Pn] = X[k] * scale % P if scale is not None else X[k]
    return out


@functools.lru_cache(4)
def _expected(name):
    c = case(name)
    t = tables(c)
    if c["op"] == "tiny":
        outs = []
        for v in sources(c):
            if c["n"] == 1:
                outs.append([v[0] % P])  # the one-point transform; its n^-1 is 1: the kernel takes no scale there
            else:
                s = t["scale"] if c["scale"] else 1
                outs.append([(v[0] + v[1]) * s % P, (v[0] - v[1]) * s % P])
        return outs
    if c["last"]:
        return [ref_row(v, c["log_n"], c["log_R"], c["digs"], t["wR"], t["scale"], c["src_n"]) for v in sources(c)]
    return [ref_column(v, c["log_n"], c["log_R"], c["log_S"], t["wR"], tw_of(c, t), c["src_n"]) for v in sources(c)]


def expected(c):
    """the residues of each distinct vector's output"""
    return _expected(c["name"])


def compose(vals, radices, w, inverse=False, src_n=0):
    """the reference passes over a plan (log2 radices, first pass first; n = their product >= 4): pass d < m is a column pass with P =
    the product of the radices before it, S = n / (P R), tw(k, j2) = (w^P)^(j2 k) and wR = w^(n / R); the last is the row pass with the
    earlier radices as digits.  inverse: over w^-1, times n^-1 -- the row pass's scale in a one-pass plan, else folded into the first
    pass's twiddles (api_ntt.hip: get_plan).  src_n: vals holds the first src_n elements, the rest is zero."""
    log_n = sum(radices)
    n = 1 << log_n
    root = pow(w, n - 1, P) if inverse else w
    ninv = pow(n, P - 2, P) if inverse else None
    m, log_pre, vec = len(radices), 0, list(vals)
    for d, r in enumerate(radices[:-1]):
        log_S = log_n - log_pre - r
        g = pow(root, 1 << log_pre, P)
        f = ninv if (d == 0 and inverse) else 1
        gk = _powers(g, 1 << r)
        vec = ref_column(vec, log_n, r, log_S, pow(root, n >> r, P), lambda k, j2, gk=gk, f=f: f * pow(gk[k], j2, P) % P,
                         src_n if d == 0 else 0)
        log_pre += r
    r = radices[-1]
    return ref_row(vec, log_n, r, tuple(radices[:-1]), pow(root, n >> r, P), ninv if m == 1 else None, src_n if m == 1 else 0)


def where(c, o):
    """(column or row inside the vector, k) of output element o of a vector"""
    if c["last"]:
        Pn = 1 << c["log_P"]
        return next(r for r in range(Pn) if drev(r, c["digs"]) == o % Pn), o // Pn
    S, RS = 1 << c["log_S"], 1 << (c["log_R"] + c["log_S"])
    return (o // RS) * S + o % S, (o % RS) // S


def residues(raw):
    """the harness's limb records (little-endian) -> residues mod p"""
    return [int.from_bytes(raw[i:i + 32], "little") % P for i in range(0, len(raw), 32)]


def check(c, out, want=None):
    """None if the harness's output of case c is what it must be, else the first wrong element.  `want`: the expected residues per
    distinct vector (default: expected(c))"""
    op = c["op"]
    if op in ("tw2", "powers", "pad"):
        if op == "pad":
            exp = [x % P if i < c["n_in"] else 0 for v in pad_sources(c) for i, x in enumerate(v)]
        elif op == "tw2":
            g, S = tables(c)["g"], 1 << c["log_S"]
            exp = [pow(g, j2 * k, P) for k in range(1 << c["log_R"]) for j2 in range(S)]
        else:
            exp = _powers(tables(c)["g"], c["n"])
        if len(out) != 32 * len(exp):
            return "%d output bytes, want %d" % (len(out), 32 * len(exp))
        got = residues(out)
        bad = next((i for i in range(len(exp)) if got[i] != exp[i] or out[32 * i:32 * i + 32] == STALE), None)
        return None if bad is None else "first wrong element %d" % bad
    n = c["n"] if op == "tiny" else 1 << c["log_n"]
    V, batch = distinct(c), c["batch"]
    if len(out) != 32 * n * batch:
        return "%d output bytes, want %d" % (len(out), 32 * n * batch)
    want = want if want is not None else expected(c)
    for b in range(batch):
        raw = out[32 * n * b:32 * n * (b + 1)]
        # a vector whose bytes equal those of the checked vector V places before it (same source, same expectation) is right
        if b >= V and raw == out[32 * n * (b - V):32 * n * (b - V + 1)]:
            continue
        got, exp = residues(raw), want[b % V]
        for o in range(n):
            if got[o] != exp[o] or raw[32 * o:32 * o + 32] == STALE:
                stale = " (never written)" if raw[32 * o:32 * o + 32] == STALE else ""
                if op == "tiny":
                    return "first wrong element: vector %d, k %d%s" % (b, o, stale)
                cr, k = where(c, o)
                return "first wrong element: vector %d, %s %d, k %d%s" % (b, "row" if c["last"] else "column", cr, k, stale)
    return None


# ---- running -------------------------------------------------------------------------------------------------------------------------
BUILD_TIMEOUT = 900  # measured: the harness cross-compiles in 72 .. 103 s (ntt.hip alone: 107 s on its own); + 800 s for a loaded machine


def build(workdir, csrc=None):
    exe = os.path.join(str(workdir), "ntt_ops")
    csrc = csrc or CSRC
    return native_harness.build([HARNESS, os.path.join(csrc, "ntt.hip"), os.path.join(csrc, "kernels.hip")], exe, csrc=csrc, timeout=BUILD_TIMEOUT)


def run(exe, names, workdir, timeout=300, env=None):
    """one harness process for the cases `names` -> ({name: path of its output}, {name: the cell the library's chooser names for it,
    (form, tile_log, xcd), None for the other ops}).  A failed process is an assertion error: nothing is run again."""
    lines, outs, inps = [], {}, []
    for i, name in enumerate(names):
        # files are numbered: a case name ("r2_col_srcn_n/8+1_narrow9") need not be a file name
        inp = os.path.join(str(workdir), "job%04d.in" % i)
        inps.append(inp)
        with open(inp, "wb") as fh:
            fh.write(job_input(name))
        outs[name] = os.path.join(str(workdir), "job%04d.out" % i)
        lines.append(job_line(case(name), inp, outs[name]))
    jf = os.path.join(str(workdir), "ntt_jobs")
    with open(jf, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    try:
        p = subprocess.run([exe, jf], capture_output=True, text=True, timeout=timeout, env=env)
    finally:
        for inp in inps:
            os.remove(inp)
    assert p.returncode == 0, "ntt_ops exited %d: %s%s" % (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    chosen = {}
    for name, cell in re.findall(r"^(\S+) chosen=(\S+)$", p.stdout, re.M):
        if cell != "-":
            f, tl, x = map(int, cell.split("/"))
            chosen[name] = ({0: "tile", 1: "narrow"}[f], tl, bool(x))
    return outs, chosen


def read_output(path):
    """the bytes of one harness output, the file removed"""
    with open(path, "rb") as fh:
        data = fh.read()
    os.remove(path)
    return data
