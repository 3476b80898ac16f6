"""The FRI commit over any odd modulus below 2^256 (sh_mod_fri_prove, sh_dev_mod_fri_prove, sh_mod_fri_fold, sh_dev_merkelize_plain:
starks_amd/csrc/modfri_items.cuh, modfri.hip, api_modfri.hip) on the MI355X: the whole grid of tests/modfri_cases.py against the exact
oracle (oracle/pyoracle.py with p = the modulus) and tests/golden/mod_fri.json (the live reference's primitives), byte for byte; the
device form; the tuned MiMC commit as yardstick at the sizes the Python oracle cannot reach; the fold and the plain tree alone; two
moduli on two contexts; the Python call sites; the errors.  Every refused call is refused on the host before any launch."""
import ctypes
import hashlib

import pytest

from conftest import load_golden
import modfri_cases as fc
import modntt_cases as mc
from modfri_cases import MODULI, root_of
from modntt_cases import ints, wire
from oracle import pyoracle

pytestmark = pytest.mark.gpu

OK, INVALID, ROOT_ORDER, TOO_SMALL, UNSUPPORTED = 0, -1, -2, -5, -6


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


def prove(L, c, ctx=None):
    """sh_mod_fri_prove on a Case -> the batch's flat proofs"""
    return prove_raw(L, c.p, c.wire(), c.n_coeffs, c.n, c.root, c.md, c.exclude, c.samples, c.batch, ctx)


def prove_raw(L, p, coeffs, n_coeffs, n, w, md, exclude=0, samples=40, batch=1, ctx=None):
    plen = L.sh_fri_proof_len(n, md, samples)
    out = ctypes.create_string_buffer(max(plen * batch, 1))
    rc = L.sh_mod_fri_prove(ctx or _ctx(), b32(p), coeffs, n_coeffs, n, b32(w), md, exclude, samples, batch, out, plen * batch)
    assert rc == OK, (rc, L.sh_last_error(ctx or _ctx()))
    return out.raw[:plen * batch]


class Dev(object):
    """a device buffer of `nbytes` bytes on a context"""

    def __init__(self, L, nbytes, ctx=None):
        self.L, self.ctx, self.nbytes = L, ctx or _ctx(), nbytes
        self.ptr = ctypes.c_void_p()
        assert L.sh_dev_alloc(self.ctx, max(nbytes, 32), ctypes.byref(self.ptr)) == OK

    def put_values(self, vals):  # plain values as 8 x u32 little-endian limbs = 32 little-endian bytes
        raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
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
    """sh_dev_mod_fri_prove on [batch][n_coeffs] plain values -> (the proof buffer, to be read after a sync)"""
    ctx = ctx or _ctx()
    plen = L.sh_fri_proof_len(c.n, c.md, c.samples)
    src = Dev(L, 32 * len(coeffs), ctx).put_values(coeffs)
    dst = Dev(L, plen * c.batch, ctx)
    rc = L.sh_dev_mod_fri_prove(ctx, b32(c.p), src.ptr, n_coeffs, c.n, b32(c.root), c.md, c.exclude, c.samples, c.batch, dst.ptr)
    assert rc == OK, (rc, L.sh_last_error(ctx))
    return src, dst


# ---- 1. the grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MODULI))
def test_grid(L, name):
    """every case of the modulus through sh_mod_fri_prove equals the oracle's flat proof byte for byte"""
    cases = [c for c in fc.GRID if c.name == name]
    assert cases
    for c in cases:
        assert prove(L, c) == fc.oracle_flat(c), c.id


def test_both_tree_forms(L):
    """n = 2^14, batch 3: the first trees are above MERKLE_SERIAL_MAX_LEAVES, the later rounds' below it"""
    c = fc.BOTH_TREE_FORMS
    assert prove(L, c) == fc.oracle_flat(c)


def test_fixture(L):
    """the live reference's primitives over BN254, 65537 and P43 (tests/golden/generate_mod_fri.py)"""
    G = load_golden("mod_fri.json")["cases"]
    for key, c in fc.FIXTURE.items():
        got = prove(L, c)
        assert len(got) == G[key]["len"] and hashlib.sha256(got).hexdigest() == G[key]["sha256"] and got[:64].hex() == G[key]["head"], key
        assert got[:32].hex() == G[key]["rounds"][0]["root_m2"]


def test_above_the_mimc_prime(L):
    """the constant p - 1 over P43: every final value and sampled leaf is p - 1 >= MIMC_P, which a MiMC canonicalisation would change"""
    top = wire([fc.P43 - 1])
    for c in [c for c in fc.GRID if c.const is not None]:
        got = prove(L, c)
        assert got == fc.oracle_flat(c)
        k = c.n >> (2 * c.rounds())
        assert got[-32 * k:] == top * k
        if c.rounds():
            assert got[32:96] == top * 2  # the first sample's column branch opens with its leaf and the leaf's sibling


# ---- 2. the device form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["bn254-n4096-md1024-c1000-x0-s40-b1", "bls12_381-n1024-md256-c256-x0-s40-b3", "p43-n64-md32-c1-x0-s40-b1-const",
                                 "f65537-n16-md16-c16-x0-s40-b1"])
def test_device_form(L, cid):
    """sh_dev_mod_fri_prove from [batch][n_coeffs] limb buffers, n_coeffs < n and (zero-extended on the host) n_coeffs = n"""
    c = fc._BY_ID[cid]
    want = prove(L, c)
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


# ---- 3. the tuned MiMC commit as yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg,batch", [(12, 1), (16, 1), (18, 2), (20, 1)])
def test_equals_the_mimc_commit(L, lg, batch):
    """over the MiMC prime the generic commit equals sh_fri_prove byte for byte (itself pinned by fri.json and fri_large.json), at
    sizes that reach the wide Merkle kernels: md = n / 8, exclude = 8, seeded coefficients of degree below md"""
    p, n = mc.MIMC_P, 1 << lg
    md, w = n // 8, mc.root_of("mimc", n)
    co = wire(mc.inputs(1000 + lg, md * batch, p))
    plen = L.sh_fri_proof_len(n, md, 40)
    want = ctypes.create_string_buffer(plen * batch)
    assert L.sh_fri_prove(_ctx(), co, md, n, b32(w), md, 8, 40, batch, want, plen * batch) == OK, L.sh_last_error(_ctx())
    got = prove_raw(L, p, co, md, n, w, md, 8, 40, batch)
    assert want.raw[:32] != bytes(32)
    assert hashlib.sha256(got).hexdigest() == hashlib.sha256(want.raw).hexdigest()


# ---- 4. the fold ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f257", "goldilocks", "bn254", "p43", "c2"])
def test_fold(L, name):
    """sh_mod_fri_fold against pyoracle.fri_fold at the challenges 0, 1, p - 1, p, 2^256 - 1, a point of the domain and the negative of
    one; n = 4 (one row) and n = 64; values at or above p included"""
    p = MODULI[name]
    for n in (4, 64):
        w = root_of(name, n)
        xs = pyoracle.get_power_cycle(w, p)
        vals = mc.inputs(n + 3, n, p)
        canon = [v % p for v in vals]
        out = ctypes.create_string_buffer(8 * n)
        for k, sx in enumerate(fc.fold_challenges(p, xs, n // 4 + 1 if n > 4 else 1)):
            assert L.sh_mod_fri_fold(_ctx(), b32(p), wire(vals), n, b32(w), b32(sx), out) == OK, L.sh_last_error(_ctx())
            assert ints(out.raw) == pyoracle.fri_fold(canon, xs, sx % p, p), (name, n, k)
            if k == 5 and n == 64:
                assert ints(out.raw)[1] == canon[n // 4 + 1]  # the row through the challenge returns its own value


# ---- 5. the tree, hashed as stored ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(4, 1), (4, 3), (16, 1), (16, 3), (1024, 1), (1024, 3), (1 << 16, 1), (1 << 16, 3)])
def test_merkelize_plain(L, n, batch):
    """sh_dev_merkelize_plain equals pyoracle.merkelize node for node; the values include p - 1 over P43 (above the MiMC prime) and
    2^256 - 1: nothing is reduced"""
    vals = mc.inputs(n + batch, n * batch, fc.P43)
    vals[0], vals[1], vals[n // 2], vals[-1] = fc.P43 - 1, 2**256 - 1, mc.MIMC_P, 2**256 - 1
    src = Dev(L, 32 * n * batch).put_values(vals)
    dst = Dev(L, 64 * n * batch)
    assert L.sh_dev_merkelize_plain(_ctx(), src.ptr, n, batch, dst.ptr) == OK, L.sh_last_error(_ctx())
    raw = dst.get()
    for b in range(batch):
        want = pyoracle.merkelize(vals[b * n:(b + 1) * n])
        assert raw[64 * n * b:64 * n * (b + 1)] == bytes(32) + b"".join(want[1:]), (n, b)
    src.free()
    dst.free()


# ---- 6. two moduli at once -----------------------------------------------------------------------------------------------------------
def test_two_moduli_on_two_contexts(L):
    """BN254 on one context and Goldilocks on another at n = 4096, enqueued back to back with no synchronisation in between: each
    proof equals the bytes of its run alone (a modulus kept in a device global fails here)"""
    from starks_amd import _lib
    ctxs = [_lib.ctx(), _lib.second_ctx()]
    cases = [fc._BY_ID["bn254-n4096-md1024-c1000-x0-s40-b1"], fc._BY_ID["goldilocks-n4096-md1024-c1000-x0-s40-b1"]]
    want = [fc.oracle_flat(c) for c in cases]
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
def test_python_call_sites(L):
    from starks_amd import IntegersModP, fft, fri, merkle_tree
    from starks_amd.wireseq import WireList
    c = fc._BY_ID["bn254-n256-md128-c128-x0-s40-b1"]
    F = IntegersModP(c.p)
    co = [v % c.p for v in c.coeffs()]
    S = fri.SmoothSubgroupFRI(F)
    proof = S.generate_proximity_proof([F(v) for v in co], F(c.root), c.md)
    assert proof == fc.oracle_proofs(c)[0]
    evals = fft.fft_1d(F, [F(v) for v in co], c.p, F(c.root))
    m_root = merkle_tree.merkelize(evals)[1]
    assert m_root == fc.merkle_root(c)
    assert S.verify_proximity_proof(proof, m_root, F(c.root), c.md)
    # the inverse transform's output (a WireList of n coefficients, the high ones zero) fed back in: the same proof
    back = fft.fft_1d(F, evals, c.p, F(c.root), inv=True)
    assert isinstance(back, WireList) and [int(v) for v in back] == co + [0] * (c.n - len(co))
    assert S.generate_proximity_proof(back, F(c.root), c.md) == proof
    assert fri.mod_prove_flat(c.p, c.wire(), c.n, c.root, c.md) == fc.oracle_flat(c)
    leaf = bytearray(proof[0][1][3][2][0])
    leaf[7] ^= 1
    proof[0][1][3][2][0] = bytes(leaf)
    with pytest.raises(AssertionError):
        S.verify_proximity_proof(proof, m_root, F(c.root), c.md)


def test_python_merkelize_above_the_mimc_prime(L):
    """a WireList over a field above the MiMC prime is committed as the bytes it is: the root equals pyoracle.merkelize"""
    from starks_amd import IntegersModP, merkle_tree
    from starks_amd.wireseq import WireList
    vals = [fc.P43 - 1, mc.MIMC_P, fc.P43 - 2, 5] * 4
    tree = merkle_tree.merkelize(WireList(wire(vals), IntegersModP(fc.P43)))
    want = pyoracle.merkelize(vals)
    assert tree[1] == want[1] and [tree[i] for i in range(1, 32)] == want[1:]


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors(L):
    c, p = _ctx(), mc.BN254
    case = fc._BY_ID["bn254-n64-md32-c32-x0-s40-b1"]
    w, co = case.root, case.wire()
    cap = L.sh_fri_proof_len(64, 32, 40)
    out = ctypes.create_string_buffer(3 * cap)

    def call(mod=p, root=w, n_coeffs=32, n=64, md=32, exclude=0, samples=40, batch=1, proof_cap=3 * cap, coeffs=co):
        rc = L.sh_mod_fri_prove(c, b32(mod), coeffs, n_coeffs, n, b32(root), md, exclude, samples, batch, out, proof_cap)
        msg = L.sh_last_error(c).decode()
        if rc != TOO_SMALL:  # the device form refuses the same calls
            assert L.sh_dev_mod_fri_prove(c, b32(mod), out, n_coeffs, n, b32(root), md, exclude, samples, batch, out) == rc
        return rc, msg

    for bad in (p - 1, 0, 1, 2, 1 << 255):
        rc, msg = call(mod=bad)
        assert rc == INVALID and "odd" in msg, (bad, msg)
    rc, msg = call(root=p + w)
    assert rc == ROOT_ORDER and "below" in msg
    for bad_root in (root_of("bn254", 32), root_of("bn254", 128), 2):
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
    rc, msg = call(n=8, root=root_of("bn254", 8), n_coeffs=8, md=32)
    assert rc == INVALID and "16 points" in msg
    rc, msg = call(n=64, md=1 << 10)  # the third round would have 4 points
    assert rc == INVALID and "16 points" in msg
    big = 1 << 26
    rc, msg = call(n=big, root=root_of("bn254", big), md=32)
    assert rc == UNSUPPORTED and "2^24" in msg
    rc, msg = call(n=big << 1, root=root_of("bn254", big << 1), md=16)
    assert rc == UNSUPPORTED and "2^26" in msg
    rc, msg = call(n=1 << 20, root=root_of("bn254", 1 << 20), md=16, batch=65)
    assert rc == UNSUPPORTED and "2^26" in msg
    rc, msg = call(proof_cap=cap - 1)
    assert rc == TOO_SMALL and "proof_cap" in msg
    assert L.sh_mod_fri_prove(c, None, co, 32, 64, b32(w), 32, 0, 40, 1, out, cap) == INVALID
    assert L.sh_mod_fri_prove(c, b32(p), co, 32, 64, None, 32, 0, 40, 1, out, cap) == INVALID
    # the fold and the plain tree
    col = ctypes.create_string_buffer(32 * 16)
    assert L.sh_mod_fri_fold(c, b32(p - 1), co, 64, b32(w), b32(1), col) == INVALID and "odd" in L.sh_last_error(c).decode()
    assert L.sh_mod_fri_fold(c, b32(p), co, 64, b32(root_of("bn254", 32)), b32(1), col) == ROOT_ORDER
    assert L.sh_mod_fri_fold(c, b32(p), co, 2, b32(p - 1), b32(1), col) == INVALID and "4 values" in L.sh_last_error(c).decode()
    assert L.sh_dev_merkelize_plain(c, out, 2, 1, out) == INVALID
    assert L.sh_dev_merkelize_plain(c, out, 24, 1, out) == INVALID
    assert L.sh_dev_merkelize_plain(c, out, 16, 0, out) == INVALID
    assert L.sh_sync(c) == OK
    # a valid call afterwards on the same context
    assert prove(L, case) == fc.oracle_flat(case)
