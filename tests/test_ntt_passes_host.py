"""The NTT pass harness (tests/native/ntt_ops.hip), its case grid and its exact reference (tests/ntt_cases.py), on the CPU: the harness
cross-compiles with ntt.hip and kernels.hip alone and refuses every malformed job before it touches the GPU; the grid launches every
pass kernel in the cross-compiled code object; the set of cells shk_launch_ntt_cell accepts is that code object's instantiation list;
knobs.hpp's chooser agrees with an independent statement of its rules over its whole domain; the reference passes, composed over a
plan, are the C oracle's transform; and check() rejects every kind of wrong output.  CPU only."""
import itertools
import os
import random
import subprocess

import pytest

import ntt_cases as nc

NATIVE = os.path.join(nc.ROOT, "tests", "native")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return nc.build(tmp_path_factory.mktemp("ntt_ops"))


@pytest.fixture(scope="module")
def insts(exe, tmp_path_factory):
    return nc.instantiations(exe, tmp_path_factory.mktemp("ntt_syms"))


@pytest.fixture(scope="module")
def chooser(tmp_path_factory):
    """tests/native/ntt_choose_host.cpp: knobs.hpp alone under plain g++ (as knobs_tsan.cpp)"""
    out = str(tmp_path_factory.mktemp("ntt_choose") / "ntt_choose_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-pthread", "-I", nc.CSRC, os.path.join(NATIVE, "ntt_choose_host.cpp"),
                           "-o", out], timeout=300)
    return out


def test_harness_cross_compiles(exe):
    """hipcc --offload-arch=gfx950 of ntt_ops.hip + ntt.hip + kernels.hip: measured 72 .. 103 s on the development machine (ntt.hip alone
    107 s before its four dead kernels went); the time limit is ntt_cases.BUILD_TIMEOUT = 900 s, the measured time + 800 s of margin"""
    assert os.path.getsize(exe) > 0


def test_code_object_holds_the_known_instantiations(insts):
    """68 tile kernels (72 before <2,10,*> and <3,9,*>, which nothing could launch, went), 32 narrow ones and ntt_tiny_kernel"""
    found, tiny = insts
    assert tiny
    assert len([i for i in found if i[0] == "tile"]) == 68 and len([i for i in found if i[0] == "narrow"]) == 32
    assert not {i for i in found if i[:3] in (("tile", 2, 10), ("tile", 3, 9))}


def test_grid_covers_every_cell(insts):
    """every instantiation in the code object is launched by a case (a new one without a case fails here), plain and through the padded
    XCD grid, every narrow one with a partial tile, every tile shape over 512 workgroups, and every argument form per radix"""
    found, _ = insts
    by_cell = {}
    for c in nc.cases():
        for cell in nc.cells_of(c):
            by_cell.setdefault(cell, []).append(c["name"])
    need = nc.required_cells(found)
    for cell in sorted(need, key=str):
        print("covered" if cell in by_cell else "MISSING", cell, by_cell.get(cell, [])[:3])
    assert need <= set(by_cell)
    assert len(need) >= 520
    # what a case names, the harness can launch; the padded XCD grids really are padded
    for c in nc.cases():
        if c["op"] == "pass":
            assert (c["form"], c["log_R"], c["tile_log"] - c["log_R"], c["last"]) in found, c["name"]
            if c["name"].endswith("_xcd"):
                assert nc.tiles_of(c) >= 64 and nc.tiles_of(c) % 8, c["name"]


def test_cell_switch_matches_code_object(insts, chooser):
    """the cells shk_launch_ntt_cell accepts (shk_ntt_cell_exists: the `if constexpr` guards of its switch) are the code object's
    instantiations, no more and no fewer, and the Python statement of the same table agrees"""
    found, _ = insts
    lines = subprocess.run([chooser, "exists"], capture_output=True, text=True, check=True, timeout=60).stdout.split("\n")
    exists = {tuple(map(int, l.split())) for l in lines if l}
    assert {(("tile", "narrow")[f], r, tl - r, last) for f, tl, r in exists for last in (False, True)} == found
    assert exists == {(f, tl, r) for f in (0, 1) for tl in range(17) for r in range(17) if nc.cell_exists(("tile", "narrow")[f], tl, r)}


def _totals(log_R):
    """column / row counts around every threshold: 64 tiles of each tile size (the XCD rule), 128 and 256 tiles of 1024 elements (the
    narrow rules), and the ends"""
    out = {1, 2, 3, 1 << 20}
    for tl in (9, 10, 11, 12):
        if tl >= log_R:
            for m in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000):
                out |= {max(1, (m << (tl - log_R)) + d) for d in (-1, 0, 1)}
    return sorted(out)


def test_chooser_against_the_documented_rules(chooser):
    """shk_ntt_choose_cell over its whole domain -- radices 2^2 .. 2^11, column and row passes, pass index 0 .. 3, every legal value of
    STARKHIP_TILE_LOG (given or not), TILE_LOG_BIG, a TILE_LOGS entry, XCD_SWZ, NARROW_TILES, tile counts around every threshold,
    first passes on both sides of the 2^16 rule -- equals ntt_cases.choose_cell; every chosen cell exists, every cell is chosen"""
    queries, want = [], []
    tile_knobs = [(10, False), (9, True), (10, True), (11, True)]
    for (tile_log, forced), big, swz, narrow in itertools.product(tile_knobs, (10, 11, 12), (0, 1, 2), (0, 1, 256, 10**8)):
        for pi, f in [(p, f) for p in (0, 3) for f in (0, 9, 10, 11, 12)] + [(1, 0), (1, 12), (2, 9), (2, 0)]:
            logs = [11, 9, 12, 10, 0, 0, 0, 0]
            logs[pi] = f
            kn = {"tile_log": tile_log, "tile_forced": forced, "tile_log_big": big, "tile_logs": tuple(logs), "xcd": swz, "narrow": narrow}
            head = "K %d %d %d %d %d %d %d %d %d" % (tile_log, forced, big, logs[0], logs[1], logs[2], logs[3], swz, narrow)
            for log_R, last in itertools.product(range(2, 12), (False, True)):
                shapes = [(log_R + 16, 16), (log_R + 15, 15), (log_R + 17, 16), (log_R + 18, 18)] if (log_R == 8 and not last) else [(log_R + 16, 16)]
                totals = _totals(log_R)
                if len(shapes) == 1 and (swz, narrow) not in ((1, 256), (2, 0)):
                    totals = totals[::5]  # the full threshold sweep under the default and the all-XCD knobs, a fifth of it elsewhere
                for (log_n, log_S), total in itertools.product(shapes, totals):
                    queries.append("%s %d %d %d %d %d %d" % (head, log_R, last, total, log_n, log_S, pi))
                    want.append(nc.choose_cell(kn, log_R, last, total, log_n, log_S, pi))
    p = subprocess.run([chooser, "choose"], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=600)
    assert p.returncode == 0
    got = [tuple(map(int, l.split())) for l in p.stdout.split("\n") if l]
    assert len(got) == len(want) > 100000
    chosen = set()
    for q, g, w in zip(queries, got, want):
        assert (("tile", "narrow")[g[0]], g[1], bool(g[2])) == w, q
        chosen.add((w[0], w[1], int(q.split()[10])))
    assert all(nc.cell_exists(*c) for c in chosen)
    assert chosen == {(f, tl, r) for f in ("tile", "narrow") for tl in range(17) for r in range(2, 12) if nc.cell_exists(f, tl, r)}
    # a radix that has no kernel
    p = subprocess.run([chooser, "choose"], input="K 10 0 11 0 0 0 0 1 256 12 0 64 20 8 0\nK 10 0 11 0 0 0 0 1 256 1 1 64 20 8 0\n",
                       capture_output=True, text=True, timeout=60)
    assert p.stdout.split("\n")[:2] == ["-1 0 0", "-1 0 0"]


def test_default_choices_are_the_documented_ones(chooser):
    """DESIGN.md section 5 under the default knobs, through the environment parse: 1024-element tiles up to radix 2^8, 2048 for radix
    2^9 .. 2^11 and for the radix-2^8 first pass of transforms from 2^24 points; narrow launches up to 256 1024-element tiles, 512-element
    ones up to 128 (radix <= 2^8); adjacent tiles on one XCD when a tile has fewer than 4 columns and the launch 64 tiles.  Then two
    environments of the plan-parity test"""
    def ask(env, *qs):
        e = {k: v for k, v in os.environ.items() if not k.startswith("STARKHIP_")}
        p = subprocess.run([chooser, "choose"], input="".join("E %d %d %d %d %d %d\n" % q for q in qs), capture_output=True, text=True,
                           timeout=60, env=dict(e, **env))
        assert p.returncode == 0
        return [tuple(map(int, l.split())) for l in p.stdout.split("\n") if l]

    big = 1 << 20
    assert ask({}, (8, 0, big, 24, 16, 0), (8, 0, big, 24, 8, 1), (8, 1, big, 24, 0, 2), (7, 0, big, 25, 18, 0), (8, 0, big, 23, 15, 0)) == \
        [(0, 11, 0), (0, 10, 0), (0, 10, 0), (0, 10, 0), (0, 10, 0)]
    assert ask({}, (9, 0, big, 17, 8, 0), (10, 1, big, 20, 0, 1), (11, 0, big, 20, 9, 0), (9, 0, 63 * 4 + 1024, 17, 8, 0)) == \
        [(0, 11, 0), (0, 11, 1), (0, 11, 1), (0, 11, 0)]
    assert ask({}, (7, 0, 128 * 8, 14, 7, 0), (7, 0, 128 * 8 + 1, 14, 7, 0), (7, 0, 256 * 8, 14, 7, 0), (7, 0, 256 * 8 + 1, 14, 7, 0),
               (9, 0, 2 * 128, 17, 8, 0), (10, 1, 256, 20, 0, 1), (10, 1, 257, 20, 0, 1)) == \
        [(1, 9, 0), (1, 10, 0), (1, 10, 0), (0, 10, 0), (1, 10, 0), (1, 10, 0), (0, 11, 1)]
    assert ask({"STARKHIP_TILE_LOGS": "12,12,12", "STARKHIP_NTT_NARROW_TILES": "0"}, (6, 0, big, 16, 10, 0), (5, 0, big, 16, 5, 1),
               (5, 1, big, 16, 0, 2), (3, 1, big, 16, 0, 2)) == [(0, 12, 0), (0, 12, 0), (0, 12, 0), (0, 10, 0)]
    assert ask({"STARKHIP_TILE_LOG": "9", "STARKHIP_TILE_LOG_BIG": "10", "STARKHIP_NTT_NARROW_TILES": "0", "STARKHIP_XCD_SWZ": "2"},
               (8, 0, big, 24, 16, 0), (9, 0, big, 18, 9, 0), (11, 0, big, 20, 9, 0)) == [(0, 9, 1), (0, 10, 1), (0, 11, 1)]


def test_reference_passes_compose_to_the_oracle_transform(chooser):
    """the definitions of ntt_cases (ref_column, ref_row, drev, the twiddle of pass d) composed over a plan are coracle.fft, forward and
    inverse: every plan shk_choose_radices gives for 2^2 .. 2^16 points, and 30 seeded random plans (digits 2 .. 11, one to four
    passes) with and without a short source.  This, not the kernel, decides what a pass is"""
    from oracle import coracle
    env = {k: v for k, v in os.environ.items() if not k.startswith("STARKHIP_")}
    lines = subprocess.run([chooser, "radices"], capture_output=True, text=True, check=True, timeout=60, env=env).stdout.split("\n")
    plans = [tuple(map(int, l.split()[1:])) for l in lines if l and 2 <= int(l.split()[0]) <= 16]
    assert len(plans) == 15 and plans[6] == (8,) and plans[7] == (5, 4) and plans[14] == (8, 8)
    rng = random.Random(2024)
    rand = []
    while len(rand) < 30:
        plan = tuple(rng.randrange(2, 12) for _ in range(rng.randrange(1, 5)))
        if sum(plan) <= 13:
            rand.append(plan)
    assert {len(p) for p in rand} == {1, 2, 3, 4}
    for i, plan in enumerate(plans + rand):
        n = 1 << sum(plan)
        w = pow(nc.root_of(n), (1, 3, n - 1)[i % 3], nc.P)
        vals = [rng.randrange(nc.M) for _ in range(n)]
        short = (0, 0, 1, n // 8 + 1, n - 1, rng.randrange(1, n))[i % 6] if i >= len(plans) else 0
        for inverse in (False, True):
            if n > 1 << 14 and inverse != bool(i % 2):
                continue  # 2^15 and 2^16 points: one direction each
            src = vals[:short] if short else vals
            assert nc.compose(src, plan, w, inverse, short) == coracle.fft([v % nc.P for v in src], n, w, inverse), (plan, inverse, short)


def _perfect(c):
    """the output bytes check() accepts for case c: the expected residues as limbs, one vector after the other"""
    want = nc.expected(c)
    V = nc.distinct(c)
    return bytearray(b"".join(x.to_bytes(32, "little") for b in range(c["batch"]) for x in want[b % V]))


def _small(pred):
    return min((c for c in nc.cases() if c["op"] == "pass" and pred(c)), key=lambda c: c["total"] << c["log_R"])


@pytest.mark.parametrize("kind", ["col", "row", "col_repeats", "tiny"])
def test_check_rejects_wrong_outputs(kind):
    """check() accepts the expected output in any representative and rejects: one element off by 1, two outputs swapped, an element
    never written (0xa5 bytes), an element plus p wrapped past 2^256 -- in a vector checked in full and in one that repeats another"""
    if kind == "tiny":
        c = nc.case("tiny2_x65_scale")
    else:
        c = _small(lambda c: c["last"] == (kind == "row") and c["log_R"] >= 4 and
                   (c["batch"] > nc.distinct(c)) == (kind == "col_repeats") and (kind != "row" or c["digs"]))
    n = c["n"] if kind == "tiny" else 1 << c["log_n"]
    good = _perfect(c)
    assert nc.check(c, bytes(good)) is None
    want = nc.expected(c)
    b = c["batch"] - 1  # the last vector: a repeat where the batch has repeats
    exp = want[b % nc.distinct(c)]
    at = lambda o: 32 * (n * b + o)  # noqa: E731
    o = next(o for o in range(n) if exp[o] + nc.P < nc.M) if any(x + nc.P < nc.M for x in exp) else None
    if o is not None:  # the other representative of a small residue is as good
        alt = bytearray(good)
        alt[at(o):at(o) + 32] = (exp[o] + nc.P).to_bytes(32, "little")
        assert nc.check(c, bytes(alt)) is None
    o = n // 2
    for what, val in (("off by one", (exp[o] + 1) % nc.P), ("stale", int.from_bytes(nc.STALE, "little")),
                      ("plus p, wrapped", (next(x for x in exp if x + nc.P >= nc.M) + nc.P) % nc.M)):
        bad = bytearray(good)
        if what == "plus p, wrapped":
            o = next(i for i in range(n) if exp[i] + nc.P >= nc.M)
        bad[at(o):at(o) + 32] = val.to_bytes(32, "little")
        why = nc.check(c, bytes(bad))
        assert why is not None and "vector %d" % b in why, (what, why)
        if kind in ("col", "col_repeats"):
            assert why.startswith("first wrong element: vector %d, column %d, k %d" % ((b,) + nc.where(c, o))), why
    bad = bytearray(good)
    i, j = next((i, j) for i in range(n) for j in range(i + 1, n) if exp[i] != exp[j])
    bad[at(i):at(i) + 32], bad[at(j):at(j) + 32] = good[at(j):at(j) + 32], good[at(i):at(i) + 32]
    assert "vector %d" % b in nc.check(c, bytes(bad))
    assert nc.check(c, bytes(good[:-32])) is not None
    # a stale element whose expected residue happens to be the residue of the 0xa5 pattern is still stale
    fake = [list(v) for v in want]
    fake[b % nc.distinct(c)][3 % n] = int.from_bytes(nc.STALE, "little") % nc.P
    bad = bytearray(good)
    first = 32 * (n * (b % nc.distinct(c)) + 3 % n)  # in the first vector of that source
    bad[first:first + 32] = nc.STALE
    assert "never written" in nc.check(c, bytes(bad), want=fake)


def test_table_kernels_expectations():
    """check() of the tw2 / powers / pad jobs against exact powers, sensitive to one wrong entry"""
    for name in ("tw2_r5_s3_lb4", "powers_1000_lb4", "pad16_in15"):
        c = nc.case(name)
        if c["op"] == "pad":
            good = b"".join((x % nc.P if i < c["n_in"] else 0).to_bytes(32, "little") for v in nc.pad_sources(c) for i, x in enumerate(v))
        elif c["op"] == "tw2":
            g = nc.tables(c)["g"]
            assert pow(g, 1 << (c["log_R"] + c["log_S"] - 1), nc.P) == nc.P - 1
            t = nc.tables(c)
            good = b"".join((t["lo"][(j * k) & 15] * t["hi"][(j * k) >> 4] % nc.P).to_bytes(32, "little") for k in range(32) for j in range(8))
        else:
            t = nc.tables(c)
            good = b"".join((t["lo"][i & 15] * t["hi"][i >> 4] % nc.P).to_bytes(32, "little") for i in range(c["n"]))
        assert nc.check(c, good) is None
        bad = bytearray(good)
        bad[32 * 7] ^= 1
        assert nc.check(c, bytes(bad)) == "first wrong element 7"


def _run_line(exe, tmp_path, lines, data):
    (tmp_path / "in").write_bytes(data)
    out = tmp_path / "out"
    if out.exists():
        out.unlink()
    (tmp_path / "jobs").write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(tmp_path / "jobs")], capture_output=True, text=True, timeout=120)
    return p.returncode, out.exists(), p.stdout + p.stderr


def test_harness_refuses_bad_jobs(exe, tmp_path):
    """a table shorter than the largest index the pass can read (tw2: R S entries; lo / hi: e <= (S - 1)(R - 1); wR: R / 2 pairs), a
    source that does not cover src_n per vector, inconsistent sizes, a cell that does not exist, too many elements, an aliased short
    source, an unknown op or key, a missing key: status 2 and no output, even when a valid job comes first.  The untouched job lines
    pass the checks: without a GPU they end at the first HIP call (status 3), with one they run (status 0)"""
    inp, out = str(tmp_path / "in"), str(tmp_path / "out")
    col = _small(lambda c: not c["last"] and c["tw"] == "tw2" and c["log_R"] == 4 and not c["src_n"] and not c["inplace"] and c["log_S"] >= 2)
    direct = _small(lambda c: not c["last"] and c["tw"] == "direct" and c["log_R"] == 5 and not c["src_n"] and c["log_S"] >= 2)
    split = _small(lambda c: not c["last"] and c["tw"] == "split" and c["lb"] < c["log_R"] + c["log_S"] and c["log_S"] >= 2 and not c["src_n"])
    short = _small(lambda c: not c["last"] and c["src_n"] > 8)
    row = _small(lambda c: c["last"] and len(c["digs"]) == 2 and c["log_R"] == 3)
    row1 = _small(lambda c: c["last"] and c["src_n"] > 1)
    tw2j, powj, padj, tiny = nc.case("tw2_r5_s3_lb4"), nc.case("powers_1000_lb4"), nc.case("pad16_in15"), nc.case("tiny2_x65_scale")
    R, S = 1 << col["log_R"], 1 << col["log_S"]
    emax_d = ((1 << direct["log_S"]) - 1) * ((1 << direct["log_R"]) - 1)
    t_split = nc.tables(split)
    bad = [
        (col, dict(n_tw2=R * S - 1), "tw2 needs"), (direct, dict(n_lo=emax_d), "lo does not cover"),
        (split, dict(n_lo=len(t_split["lo"]) - 1), "lo does not cover"), (split, dict(n_hi=len(t_split["hi"]) - 1), "hi does not cover"),
        (split, dict(lb=split["lb"] - 1), "hi does not cover"), (col, dict(n_wr=R // 2 - 1), "wR needs"),
        (short, dict(n_src=short["src_n"] - 1), "whole vectors"), (short, dict(n_src=nc.distinct(short) * short["src_n"] - 1), "whole vectors"),
        (row1, dict(n_src=row1["src_n"] - 1), "whole vectors"), (col, dict(n_src=(1 << col["log_n"]) - 1), "whole vectors"),
        (col, dict(total=col["total"] + 1), "whole number"), (col, dict(log_S=col["log_S"] + 1), "exceeds n"),
        (col, dict(log_n=col["log_n"] + 2), "whole number of vectors"), (row, dict(d0=row["digs"][0] + 1), "sum to log_P"),
        (row, dict(ndig=1), "digit widths"), (row, dict(log_P=row["log_P"] + 1), "P = n / R"), (row, dict(inplace=1), "single-pass"),
        (short, dict(inplace=1), "alias"), (short, dict(src_n=(1 << short["log_n"]) + 1), "exceeds n"),
        (short, dict(log_n=short["log_n"] + 1, total=short["total"] * 2), "first pass"),
        (col, dict(form=0, tile_log=12, log_R=3), "no such cell"), (col, dict(form=1, tile_log=11), "no such cell"),
        (col, dict(form=0, tile_log=9, log_R=9), "no such cell"), (col, dict(form=1, tile_log=9, xcd=1), "only tile launches"),
        (col, dict(total=1 << 23), "element cap"), (col, dict(total=S << 19, log_n=col["log_n"] + 19), "too many elements"),
        (col, dict(tw=0), "needs tw"), (col, dict(tw=2), "no tw2"), (row, dict(tw=1), "no inter-pass"), (col, dict(scale=1), "no digits"),
        (tw2j, dict(n_hi=1), "hi does not cover"), (tw2j, dict(log_S=20), "too large"), (powj, dict(n_lo=15), "lo does not cover"),
        (powj, dict(n=0), "out of range"), (padj, dict(n_in=17), "exceeds n"), (padj, dict(batch=1 << 20), "out of range"),
        (tiny, dict(n=3), "n must be"), (tiny, dict(n_src=1), "whole vectors"), (tiny, dict(batch=0), "out of range"),
    ]
    for c in (col, direct, split, short, row, row1, tw2j, powj, padj, tiny):
        rc, wrote, msg = _run_line(exe, tmp_path, [nc.job_line(c, inp, out)], nc.job_input(c["name"]))
        assert rc in (0, 3), (c["name"], rc, msg)
    for c, override, text in bad:
        rc, wrote, msg = _run_line(exe, tmp_path, [nc.job_line(c, inp, out, **override)], nc.job_input(c["name"]))
        assert rc == 2 and not wrote and text in msg, (c["name"], override, rc, msg)
    data = nc.job_input(col["name"])
    good = nc.job_line(col, inp, out)
    other = nc.job_line(col, inp, str(tmp_path / "out2"))
    for lines, d in (([good], data[:-32]), ([good], data + bytes(32)), ([good.replace("pass ", "ntt ", 1)], data), ([good + " bogus=1"], data),
                     ([good.replace(" lb=0", "")], data), ([good + " lb=0"], data), ([good.replace("total=", "total=-")], data),
                     ([good.replace(" in=" + inp, "")], data), ([good + " x"], data), ([], data),
                     ([other, nc.job_line(col, inp, out, n_wr=1)], data)):
        rc, wrote, msg = _run_line(exe, tmp_path, lines, d)
        assert rc == 2 and not wrote and not (tmp_path / "out2").exists(), (lines, rc, msg)
