"""The FRI commit over any odd modulus below 2^64 on packed 64-bit words (sh_mod64_fri_prove, sh_dev_mod64_fri_prove, sh_mod64_fri_fold,
sh_dev_mod64_merkelize: starks_amd/csrc/mod64fri_items.cuh, mod64fri.hip, api_mod64fri.hip) on the MI355X: the whole grid of
tests/mod64fri_cases.py against the exact oracle (oracle/pyoracle.py with p = the modulus), byte for byte; the device form; the generic
commit (sh_mod_fri_prove) as yardstick at the sizes the Python oracle cannot reach; the library's verifier; the fold and the tree
alone; two moduli on two contexts; the Python entries; the refusals.  Every refused call is refused on the host before any launch."""
import ctypes
import hashlib

import pytest

import mod64fri_cases as qc
import modfri_cases as fc
import modntt_cases as mc
import ntt64_cases as nc
from mod64fri_cases import MODULI, root_of
from oracle import pyoracle

pytestmark = pytest.mark.gpu

OK, INVALID, ROOT_ORDER, TOO_SMALL, UNSUPPORTED, REJECTED = 0, -1, -2, -5, -6, -9


def b32(x):
    return int(x).to_bytes(32, "big")


@pytest.fixture(scope="module")
def L():
    from starks_amd import _lib
    _lib.ctx()
    return _lib.lib()


def _ctx():
    from starks_amd import _lib
    return _lib.ctx()


def prove_raw(L, p, words, n_coeffs, n, w, md, exclude=0, samples=40, batch=1, ctx=None):
    plen = L.sh_fri_proof_len(n, md, samples)
    out = ctypes.create_string_buffer(max(plen * batch, 1))
    rc = L.sh_mod64_fri_prove(ctx or _ctx(), p, words, n_coeffs, n, w, md, exclude, samples, batch, out, plen * batch)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))
    return out.raw[:plen * batch]


def prove(L, c, ctx=None):
    """sh_mod64_fri_prove on a Case -> the batch's flat proofs"""
    return prove_raw(L, c.p, c.words(), c.n_coeffs, c.n, c.root, c.md, c.exclude, c.samples, c.batch, ctx)


def generic(L, p, vals, n_coeffs, n, w, md, exclude=0, samples=40, batch=1):
    """sh_mod_fri_prove on the same values as 32-byte wire"""
    plen = L.sh_fri_proof_len(n, md, samples)
    out = ctypes.create_string_buffer(max(plen * batch, 1))
    rc = L.sh_mod_fri_prove(_ctx(), b32(p), mc.wire(vals), n_coeffs, n, b32(w), md, exclude, samples, batch, out, plen * batch)
    assert rc == OK, (rc, L.sh_last_error(_ctx()))
    return out.raw[:plen * batch]


class Dev(object):
    """a device buffer of `nbytes` bytes on a context"""

    def __init__(self, L, nbytes, ctx=None):
        self.L, self.ctx, self.nbytes = L, ctx or _ctx(), nbytes
        self.ptr = ctypes.c_void_p()
        assert L.sh_dev_alloc(self.ctx, max(nbytes, 32), ctypes.byref(self.ptr)) == OK

    def put(self, raw):
        assert self.L.sh_dev_upload(self.ctx, raw, self.ptr, len(raw)) == OK
        return self

    def get(self):
        out = ctypes.create_string_buffer(max(self.nbytes, 1))
        assert self.L.sh_dev_download(self.ctx, self.ptr, out, self.nbytes) == OK
        return out.raw[:self.nbytes]

    def free(self):
        assert self.L.sh_sync(self.ctx) == OK
        assert self.L.sh_dev_free(self.ctx, self.ptr) == OK


def dev_prove(L, c, coeffs, n_coeffs, ctx=None):
    """sh_dev_mod64_fri_prove on [batch][n_coeffs] words -> (source, the proof buffer, to be read after a sync)"""
    ctx = ctx or _ctx()
    plen = L.sh_fri_proof_len(c.n, c.md, c.samples)
    src = Dev(L, 8 * len(coeffs), ctx).put(nc.words(coeffs))
    dst = Dev(L, plen * c.batch, ctx)
    rc = L.sh_dev_mod64_fri_prove(ctx, c.p, src.ptr, n_coeffs, c.n, c.root, c.md, c.exclude, c.samples, c.batch, dst.ptr)
    assert rc == OK, (rc, L.sh_last_error(ctx))
    return src, dst


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(L, name):
    """every case of the modulus through sh_mod64_fri_prove equals the oracle's flat proof byte for byte"""
    cases = [c for c in qc.GRID if c.name == name]
    assert cases
    for c in cases:
        assert prove(L, c) == qc.oracle_flat(c), c.id


def test_both_tree_forms(L):
    """n = 2^14, batch 3 over BIG18: the first trees are above MERKLE_SERIAL_MAX_LEAVES, the later rounds' below it"""
    c = qc.BOTH_TREE_FORMS
    assert prove(L, c) == qc.oracle_flat(c)


def test_top_bit_leaves(L):
    """the constant p - 1 over BIG18: every final value and sampled leaf is 24 zero bytes and p - 1, top bit set"""
    top = bytes(24) + (qc.BIG18 - 1).to_bytes(8, "big")
    for c in [c for c in qc.GRID if c.const is not None]:
        got = prove(L, c)
        assert got == qc.oracle_flat(c)
        k = c.n >> (2 * c.rounds())
        assert got[-32 * k:] == top * k
        if c.rounds():
            assert got[32:96] == top * 2  # the first sample's column branch opens with its leaf and the leaf's sibling


# ---- 2. the device form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["big18-n4096-md1024-c1000-x0-s40-b1", "big18-n64-md32-c30-x0-s40-b3", "goldilocks-n256-md128-c128-x0-s80-b1",
                                 "f65537-n16-md16-c3-x0-s40-b1"])
def test_device_form(L, cid):
    """sh_dev_mod64_fri_prove from [batch][n_coeffs] word buffers, n_coeffs < n and (zero-extended on the host) n_coeffs = n"""
    c = qc._BY_ID[cid]
    assert c.n_coeffs < c.n
    want = qc.oracle_flat(c)
    co = c.coeffs()
    src, dst = dev_prove(L, c, co, c.n_coeffs)
    assert dst.get() == want
    full = []
    for b in range(c.batch):
        full += co[b * c.n_coeffs:(b + 1) * c.n_coeffs] + [0] * (c.n - c.n_coeffs)
    src2, dst2 = dev_prove(L, c, full, c.n)
    assert dst2.get() == want
    for d in (src, dst, src2, dst2):
        d.free()


# ---- 3. the generic commit as yardstick ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,lg,batch", [("goldilocks", 12, 1), ("goldilocks", 16, 1), ("goldilocks", 18, 2), ("goldilocks", 20, 1),
                                           ("babybear", 16, 3)])
def test_equals_the_generic_commit(L, name, lg, batch):
    """the packed commit equals sh_mod_fri_prove byte for byte (itself pinned by the oracle and by mod_fri.json) on the same values as
    32-byte wire, at sizes that reach the wide Merkle kernels and multi-pass transforms: md = n / 8, exclude = 8, seeded words"""
    p, n = MODULI[name], 1 << lg
    md, w = n // 8, root_of(name, n)
    vals = nc.inputs(1000 + lg, md * batch, p)
    want = generic(L, p, vals, md, n, w, md, 8, 40, batch)
    got = prove_raw(L, p, nc.words(vals), md, n, w, md, 8, 40, batch)
    assert want[:32] != bytes(32) and len(got) == len(want)
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(want).hexdigest()


# ---- 4. the library's verifier -------------------------------------------------------------------------------------------------------
def test_verifier_accepts_and_rejects(L):
    """sh_mod_fri_verify takes a packed-word proof unchanged, and rejects it after one flipped leaf byte"""
    c = qc._BY_ID["big18-n256-md128-c128-x0-s40-b1"]
    proof = prove(L, c)
    root = qc.merkle_root(c)

    def verify(flat):
        return L.sh_mod_fri_verify(b32(c.p), flat, len(flat), root, c.n, b32(c.root), c.md, c.exclude, c.samples)

    assert verify(proof) == OK
    bad = bytearray(proof)
    bad[32 + 31] ^= 1  # the low byte of the first sample's column leaf
    assert verify(bytes(bad)) == REJECTED


# ---- 5. the fold and the tree alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f257", "goldilocks", "big18", "c2", "p64_59"])
def test_fold(L, name):
    """sh_mod64_fri_fold against pyoracle.fri_fold at the challenges 0, 1, p - 1, p, 2^256 - 1, a point of the domain and the negative of
    one; n = 4 (one row) and n = 64; words at or above p included"""
    p = MODULI[name]
    for n in (4, 64) if name != "p64_59" else (4,):
        w = root_of(name, n)
        xs = pyoracle.get_power_cycle(w, p)
        vals = nc.inputs(n + 3, n, p)
        canon = [v % p for v in vals]
        out = ctypes.create_string_buffer(2 * n)
        for k, sx in enumerate(fc.fold_challenges(p, xs, n // 4 + 1 if n > 4 else 1)):
            assert L.sh_mod64_fri_fold(_ctx(), p, nc.words(vals), n, w, b32(sx), out) == OK, L.sh_last_error(_ctx())
            assert nc.ints(out.raw) == pyoracle.fri_fold(canon, xs, sx % p, p), (name, n, k)
            if k == 5 and n == 64:
                assert nc.ints(out.raw)[1] == canon[n // 4 + 1]  # the row through the challenge returns its own value


@pytest.mark.parametrize("n,batch", [(4, 1), (4, 3), (16, 1), (16, 3), (1024, 1), (1024, 3), (1 << 16, 1), (1 << 16, 3)])
def test_merkelize(L, n, batch):
    """sh_dev_mod64_merkelize equals pyoracle.merkelize node for node, and sh_dev_merkelize_plain on sh_dev_mod64_to_limbs of the same
    words byte for byte; 0, p - 1 and 2^64 - 1 among the values: nothing is reduced"""
    p = qc.BIG18
    vals = nc.inputs(n + batch, n * batch, p)
    vals[0], vals[1], vals[n // 2], vals[-1] = 0, p - 1, 2**64 - 1, 2**64 - 1
    src = Dev(L, 8 * n * batch).put(nc.words(vals))
    dst = Dev(L, 64 * n * batch)
    assert L.sh_dev_mod64_merkelize(_ctx(), src.ptr, n, batch, dst.ptr) == OK, L.sh_last_error(_ctx())
    raw = dst.get()
    for b in range(batch):
        want = pyoracle.merkelize(vals[b * n:(b + 1) * n])
        assert raw[64 * n * b:64 * n * (b + 1)] == bytes(32) + b"".join(want[1:]), (n, b)
    limbs, dst2 = Dev(L, 32 * n * batch), Dev(L, 64 * n * batch)
    assert L.sh_dev_mod64_to_limbs(_ctx(), src.ptr, limbs.ptr, n * batch) == OK
    assert L.sh_dev_merkelize_plain(_ctx(), limbs.ptr, n, batch, dst2.ptr) == OK
    assert dst2.get() == raw
    for d in (src, dst, limbs, dst2):
        d.free()


# ---- 6. two moduli at once -----------------------------------------------------------------------------------------------------------
def test_two_moduli_on_two_contexts(L):
    """Goldilocks on one context and BIG18 on another at n = 4096, enqueued back to back with no synchronisation in between: each
    proof equals the bytes of its run alone (a modulus kept in a device global fails here)"""
    from starks_amd import _lib
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    cases = [qc._BY_ID["goldilocks-n4096-md1024-c1000-x0-s40-b1"], qc._BY_ID["big18-n4096-md1024-c1000-x0-s40-b1"]]
    want = [qc.oracle_flat(c) for c in cases]
    assert [prove(L, c, ctx) for c, ctx in zip(cases, ctxs)] == want
    held = []
    for r in range(4):
        for c, ctx in zip(cases, ctxs):
            held.append(dev_prove(L, c, c.coeffs(), c.n_coeffs, ctx))
    for ctx in ctxs:
        assert L.sh_sync(ctx) == OK
    for k, (src, dst) in enumerate(held):
        assert dst.get() == want[k % 2], k
        src.free()
        dst.free()


# ---- 7. Python -----------------------------------------------------------------------------------------------------------------------
def test_python_entries(L):
    import array
    from starks_amd import IntegersModP, fri
    c = qc._BY_ID["big18-n256-md128-c128-x0-s40-b1"]
    want = qc.oracle_flat(c)
    co = c.coeffs()
    for data in (co, c.words(), array.array("Q", co), bytearray(c.words())):
        assert fri.mod64_prove_flat(c.p, data, c.n, c.root, c.md) == want
    assert fri.mod64_prove_flat(c.p, co, c.n, c.root, c.md) == fri.mod_prove_flat(c.p, c.wire(), c.n, c.root, c.md)
    b3 = qc._BY_ID["big18-n64-md32-c30-x0-s40-b3"]
    assert fri.mod64_prove_flat(b3.p, b3.words(), b3.n, b3.root, b3.md, batch=3) == qc.oracle_flat(b3)
    x8 = qc._BY_ID["big18-n1024-md256-c256-x8-s40-b1"]
    assert fri.mod64_prove_flat(x8.p, x8.coeffs(), x8.n, x8.root, x8.md, exclude_multiples_of=8) == qc.oracle_flat(x8)
    # the nested proof, through the reference-shaped verifier and the library's
    S = fri.SmoothSubgroupFRI(IntegersModP(c.p))
    nested = fri.unpack_proof(want, c.n, c.md)
    assert nested == qc.oracle_proofs(c)[0]
    assert S.verify_proximity_proof(nested, qc.merkle_root(c), c.root, c.md)
    assert fri.mod_verify_flat(c.p, want, qc.merkle_root(c), c.n, c.root, c.md)
    # the fold
    p, n = c.p, 64
    w = root_of("big18", n)
    xs = pyoracle.get_power_cycle(w, p)
    vals = nc.inputs(77, n, p)
    for sx in (xs[5], 2**256 - 1):
        want_col = pyoracle.fri_fold([v % p for v in vals], xs, sx % p, p)
        assert list(fri.mod64_fold(p, vals, n, w, sx)) == want_col
        assert list(fri.mod64_fold(p, array.array("Q", vals), n, w, b32(sx))) == want_col
    with pytest.raises(ValueError):
        fri.mod64_prove_flat(c.p, co[:7], c.n, c.root, c.md, batch=2)
    with pytest.raises(ValueError):
        fri.mod64_fold(p, vals[:8], n, w, 1)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(L):
    c, p = _ctx(), mc.GOLDILOCKS
    case = qc._BY_ID["goldilocks-n64-md32-c32-x0-s40-b1"]
    w, co = case.root, case.words()
    cap = L.sh_fri_proof_len(64, 32, 40)
    out = ctypes.create_string_buffer(3 * cap)

    def call(mod=p, root=w, n_coeffs=32, n=64, md=32, exclude=0, samples=40, batch=1, proof_cap=3 * cap, coeffs=co):
        rc = L.sh_mod64_fri_prove(c, mod, coeffs, n_coeffs, n, root, md, exclude, samples, batch, out, proof_cap)
        msg = L.sh_last_error(c).decode()
        assert "sh_mod64_fri_prove" in msg
        if rc != TOO_SMALL:  # the device form refuses the same calls (nothing is launched: the pointers are never read)
            assert L.sh_dev_mod64_fri_prove(c, mod, out, n_coeffs, n, root, md, exclude, samples, batch, out) == rc
            assert "sh_dev_mod64_fri_prove" in L.sh_last_error(c).decode()
        return rc, msg

    for bad in (p - 1, 1 << 63):  # even
        rc, msg = call(mod=bad)
        assert rc == INVALID and "odd" in msg, (bad, msg)
    for bad in (0, 1, 2):  # below 3
        rc, msg = call(mod=bad)
        assert rc == INVALID and "at least 3" in msg, (bad, msg)
    rc, msg = call(root=p)
    assert rc == ROOT_ORDER and "below" in msg
    rc, msg = call(root=2**64 - 1)
    assert rc == ROOT_ORDER and "below" in msg
    for bad_root in (root_of("goldilocks", 32), root_of("goldilocks", 128), 2):
        rc, msg = call(root=bad_root)
        assert rc == ROOT_ORDER and "order" in msg
    rc, msg = call(n=48)
    assert rc == INVALID and "power of two" in msg
    rc, msg = call(n_coeffs=65, coeffs=co * 3)
    assert rc == INVALID and "coefficients" in msg
    rc, msg = call(batch=0)
    assert rc == INVALID and "batch" in msg
    rc, msg = call(exclude=1)
    assert rc == INVALID and "exclude" in msg
    rc, msg = call(samples=0)
    assert rc == INVALID and "samples" in msg
    rc, msg = call(n=8, root=root_of("goldilocks", 8), n_coeffs=8, md=32)
    assert rc == INVALID and "16 points" in msg
    rc, msg = call(n=64, md=1 << 10)  # the third round would have 4 points
    assert rc == INVALID and "16 points" in msg
    big = 1 << 26
    rc, msg = call(n=big, root=root_of("goldilocks", big), md=32)  # the column of 2^24 rows cannot be sampled
    assert rc == UNSUPPORTED and "2^24" in msg
    rc, msg = call(n=1 << 29, root=root_of("goldilocks", 1 << 29), md=16)
    assert rc == UNSUPPORTED and "2^28" in msg
    rc, msg = call(n=1 << 20, root=root_of("goldilocks", 1 << 20), md=16, batch=257)
    assert rc == UNSUPPORTED and "2^28" in msg
    rc, msg = call(batch=65536)  # 2^22 points in all: inside the transform's limit
    assert rc == UNSUPPORTED and "65535" in msg
    rc, msg = call(proof_cap=cap - 1)
    assert rc == TOO_SMALL and "proof_cap" in msg
    assert L.sh_mod64_fri_prove(c, p, None, 32, 64, w, 32, 0, 40, 1, out, cap) == INVALID and "null" in L.sh_last_error(c).decode()
    assert L.sh_mod64_fri_prove(c, p, co, 32, 64, w, 32, 0, 40, 1, None, cap) == INVALID and "null" in L.sh_last_error(c).decode()
    assert L.sh_dev_mod64_fri_prove(c, p, None, 32, 64, w, 32, 0, 40, 1, out) == INVALID
    assert L.sh_dev_mod64_fri_prove(c, p, out, 32, 64, w, 32, 0, 40, 1, None) == INVALID
    assert L.sh_mod64_fri_prove(None, p, co, 32, 64, w, 32, 0, 40, 1, out, cap) == INVALID
    # the fold and the tree
    col = ctypes.create_string_buffer(8 * 16)
    assert L.sh_mod64_fri_fold(c, p - 1, co + co, 64, w, b32(1), col) == INVALID and "odd" in L.sh_last_error(c).decode()
    assert L.sh_mod64_fri_fold(c, p, co + co, 64, root_of("goldilocks", 32), b32(1), col) == ROOT_ORDER
    assert L.sh_mod64_fri_fold(c, p, co, 2, p - 1, b32(1), col) == INVALID and "4 values" in L.sh_last_error(c).decode()
    assert L.sh_mod64_fri_fold(c, p, None, 64, w, b32(1), col) == INVALID
    assert L.sh_mod64_fri_fold(c, p, co + co, 64, w, None, col) == INVALID
    assert L.sh_mod64_fri_fold(c, p, co + co, 64, w, b32(1), None) == INVALID
    assert L.sh_dev_mod64_merkelize(c, out, 2, 1, out) == INVALID
    assert L.sh_dev_mod64_merkelize(c, out, 24, 1, out) == INVALID
    assert L.sh_dev_mod64_merkelize(c, out, 16, 0, out) == INVALID
    assert L.sh_dev_mod64_merkelize(c, None, 16, 1, out) == INVALID
    assert L.sh_dev_mod64_merkelize(c, out, 16, 1, None) == INVALID
    assert L.sh_sync(c) == OK
    # a valid call afterwards on the same context
    assert prove(L, case) == qc.oracle_flat(case)
