"""Every Merkle tree form and the FRI fold of starks_amd/csrc/kernels.hip on the MI355X, node for node.

The harness (tests/native/tree_ops.hip, built with kernels.hip alone) runs the whole grid of tests/tree_cases.py in one process: the
leaf kernel in each form (raw leaves, limb leaves with and without the leaf level) wide and narrow, the mid kernel with full and
partial workgroups and one parent per tree, the serial top kernel for every remaining level count, the trees built from the values,
the fold and the fold fused into its column's tree, and packed leaves.  Trees are batched so that the forms only a batch reaches
run on small buffers.  Each case reports its first wrong node as (tree, level, index), or its first wrong column row.

Then the same forms through the library's C ABI: sh_dev_merkelize over a batch grid with unreduced inputs, sh_dev_fri_fold with each
proof's challenge taken from node 1 of its own tree, sh_fri_fold where the twiddle table is stored as two halves, and
sh_merkelize_packed over (n, k)."""
import ctypes
import time

import pytest

import tree_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    d = tmp_path_factory.mktemp("tree_gpu")
    t0 = time.time()
    exe = tc.build(d)
    t1 = time.time()
    out = tc.run(exe, [c["name"] for c in tc.cases()], d, timeout=300)
    print("\ntree_ops: built in %.1f s, %d cases run in %.1f s" % (t1 - t0, len(out), time.time() - t1))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in tc.cases()])
def test_harness_case(results, name):
    c = tc.case(name)
    why = tc.check(c, tc.read_output(results[name]))
    assert why is None, "%s (%s): %s" % (name, sorted(tc.cells_of(c), key=str), why)


@pytest.fixture(scope="module")
def api():
    from starks_amd import _lib
    return _lib.lib(), _lib.ctx()


@pytest.fixture
def dev(api):
    """alloc(nbytes) -> a device buffer of the library's context; every buffer is freed when the test ends, passed or failed"""
    L, ctx = api
    bufs = []

    def alloc(nbytes):
        p = ctypes.c_void_p()
        assert L.sh_dev_alloc(ctx, nbytes, ctypes.byref(p)) == 0
        bufs.append(p)
        return p

    yield alloc
    for p in bufs:
        assert L.sh_dev_free(ctx, p) == 0


def _dev_trees(L, ctx, alloc, c):
    """values of case-like dict c through sh_dev_from_wire (unreduced ones stay unreduced), then sh_dev_merkelize -> (values, nodes)"""
    n, batch = c["n"], c["batch"]
    wire = b"".join(tc.values(c, b) for b in range(batch))
    dv, dt = alloc(32 * n * batch), alloc(64 * n * batch)
    assert L.sh_dev_from_wire(ctx, wire, dv, n * batch) == 0
    assert L.sh_dev_merkelize(ctx, dv, n, batch, dt) == 0
    return dv, dt


@pytest.mark.parametrize("n,batch", [(4, 7), (16, 4096), (64, 1 << 13), (1 << 10, 48), (1 << 12, 3), (1 << 16, 2)])
def test_dev_merkelize_batches(api, dev, n, batch):
    """every node of every tree of a batched sh_dev_merkelize equals the oracle's tree of the canonical values"""
    L, ctx = api
    c = {"name": "abi_tree_%d_%d" % (n, batch), "n": n, "batch": batch, "form": "limb"}
    dv, dt = _dev_trees(L, ctx, dev, c)
    got = ctypes.create_string_buffer(64 * n * batch)
    assert L.sh_dev_download(ctx, dt, got, 64 * n * batch) == 0
    got = got.raw
    for b in range(batch):
        want = tc.expected_tree(c, b)
        g = got[64 * n * b:64 * n * (b + 1)]
        assert g == want, "n %d batch %d: first bad node (tree, level, index) = %s" % (n, batch, (b,) + tc.first_bad_node(g, want, n)[1:])


@pytest.mark.parametrize("n,batch", [(4, 5), (64, 33), (1 << 10, 8), (1 << 14, 2)])
def test_dev_fri_fold_challenge_per_tree(api, dev, n, batch):
    """sh_dev_fri_fold on the trees of a batched sh_dev_merkelize: column b is the C oracle's fold of values b at node 1 of tree b"""
    from oracle import coracle
    L, ctx = api
    c = {"name": "abi_fold_%d_%d" % (n, batch), "n": n, "batch": batch, "form": "limb"}
    dv, dt = _dev_trees(L, ctx, dev, c)
    q = n // 4
    dc = dev(32 * q * batch)
    w = tc.root_of(n)
    assert L.sh_dev_fri_fold(ctx, dv, dt, n, batch, w.to_bytes(32, "big"), dc) == 0
    col = ctypes.create_string_buffer(32 * q * batch)
    assert L.sh_dev_to_wire(ctx, dc, col, q * batch) == 0
    nodes = ctypes.create_string_buffer(64 * n * batch)
    assert L.sh_dev_download(ctx, dt, nodes, 64 * n * batch) == 0
    col, nodes = col.raw, nodes.raw
    for b in range(batch):
        node1 = nodes[64 * n * b + 32:64 * n * b + 64]
        vals = [int.from_bytes(v, "big") for v in tc._split(tc.values(c, b))]
        got = [int.from_bytes(v, "big") for v in tc._split(col[32 * q * b:32 * q * (b + 1)])]
        want = coracle.fold(vals, w, node1)
        assert got == want, "batch %d: first bad row %d" % (b, next(i for i in range(q) if got[i] != want[i]))


@pytest.mark.parametrize("logn,sx", [(19, tc.M - 1), (20, tc.P + 1)])
def test_fri_fold_split_tables(api, logn, sx):
    """sh_fri_fold above 2^18 points, where the power table is stored as lo/hi halves, with an unreduced special_x"""
    from oracle import coracle
    L, ctx = api
    n = 1 << logn
    c = {"name": "abi_fold_big_%d" % logn, "n": n}
    wire = tc.values(c, 0)
    out = ctypes.create_string_buffer(8 * n)
    w = tc.root_of(n)
    assert L.sh_fri_fold(ctx, wire, n, w.to_bytes(32, "big"), sx.to_bytes(32, "big"), out) == 0
    got = [int.from_bytes(v, "big") for v in tc._split(out.raw)]
    want = coracle.fold([int.from_bytes(v, "big") for v in tc._split(wire)], w, sx.to_bytes(32, "big"))
    assert got == want, "first bad row %d" % next(i for i in range(n // 4) if got[i] != want[i])


@pytest.mark.parametrize("n,k", [(4, 1), (4, 5), (8, 16), (64, 2), (256, 7), (1 << 12, 8), (1 << 14, 3)])
def test_merkelize_packed_abi(api, n, k):
    """sh_merkelize_packed: nodes and permuted leaves equal merkelize_polynomial_evaluations"""
    L, ctx = api
    c = {"name": "abi_packed_%d_%d" % (n, k), "n": n, "k": k}
    evals = b"".join(tc.values(c, j, what="evals") for j in range(k))
    nodes, leaves = ctypes.create_string_buffer(32 * n), ctypes.create_string_buffer(32 * n * k)
    assert L.sh_merkelize_packed(ctx, evals, n, k, nodes, leaves) == 0
    want_nodes, want_leaves = tc.expected_packed(c)
    assert nodes.raw == want_nodes
    assert leaves.raw == want_leaves
