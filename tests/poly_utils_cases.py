"""The inputs of tests/golden/poly_utils.json's MiMC multi_inv cases, rebuilt from their recipes (tests/golden/generate_poly_utils.py):
each is checked against the fixture's `in_sha` before use."""
import hashlib
import struct

P = 2**256 - 2**32 * 351 + 1

ZERO_RUNS = {  # name: (seed, n, runs of zeros [a, b))
    "seeded_64_zero_runs": (21, 64, [(0, 1), (9, 12), (63, 64)]),
    "seeded_1000_zero_runs": (22, 1000, [(0, 3), (100, 164), (511, 520), (999, 1000)]),
    "seeded_5000_zero_tile": (23, 5000, [(1024, 2048), (4095, 4100)]),
}


def seeded(seed, i):
    return int.from_bytes(hashlib.blake2s(struct.pack("<QQ", seed, i)).digest(), "big") % P


def wire(vals):
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def mimc_inputs(c):
    name = c["name"]
    if name in ("xs_minus_1_4096", "z_evals_4096"):  # test_poly_utils.py:88-104
        g = pow(7, (P - 1) // 4096, P)
        xs = [pow(g, i, P) for i in range(4096)]
        vals = [(x - 1) % P for x in xs] if name == "xs_minus_1_4096" else [(xs[(i * 512) % 4096] - 1) % P for i in range(4096)]
    elif name in ZERO_RUNS:
        seed, n, runs = ZERO_RUNS[name]
        vals = [seeded(seed, i) for i in range(n)]
        for a, b in runs:
            for i in range(a, min(b, n)):
                vals[i] = 0
    elif name == "seeded_3_all_zero":
        vals = [0, 0, 0]
    else:
        raise KeyError(name)
    assert hashlib.sha256(wire(vals)).hexdigest() == c["in_sha"], name
    return vals


def interp_restated(xs, ys, p):
    """poly_utils.py:412-440 in Python ints, the reference's multi_inv on field elements included (a zero e_k "inverts" to 1)"""
    out = []
    for x, y in zip(xs, ys):
        c = [0, 0, 0, 0]
        for k in range(4):
            o = [x[j] for j in range(4) if j != k]
            eq = [-(o[0] * o[1] * o[2]), o[0] * o[1] + o[0] * o[2] + o[1] * o[2], -(o[0] + o[1] + o[2]), 1]
            e = (x[k] - o[0]) * (x[k] - o[1]) * (x[k] - o[2]) % p
            w = y[k] * (pow(e, p - 2, p) if e else 1) % p
            for i in range(4):
                c[i] = (c[i] + eq[i] * w) % p
        out.append(c)
    return out


def strip(c):
    c = list(c)
    while c and c[-1] == 0:
        c.pop()
    return c
