"""fastoracle -- TEST INFRASTRUCTURE ONLY (never imported by the product path).

STARK.mk_proof (starks/stark.py:27-279) in O(n log n), exact, in coefficient form like the reference.
oracle/pyoracle.py:mk_stark_proof restates the reference's construction literally (schoolbook products and long
division, O(n^2): 43 s at 2^12 steps, hours at 2^16).  This module builds the SAME polynomials -- coefficient for
coefficient -- from the C oracle's transforms (oracle/oracle.c, the reference's recursive FFT) and O(n) passes:

* P_j: inverse NTT of witness column j over G1 (stark.py:27-36).
* C_j = P_j(g1 X) - step_j(P): evaluated on the precision domain (size steps * ext > degree * (steps - 1), which the
  library demands of every shape), then inverse-NTT'd to its exact coefficients (stark.py:38-57).
* D_j = C_j (X - x_last) / (X^steps - 1): one multiplication by a linear factor and a synthetic division by the sparse
  divisor, whose remainder must vanish (stark.py:59-79 asserts `cp % z == 0`).  Never a pointwise division by Z, which
  is 0/0 on the trace points.
* B_j = (P_j - I_j) / ((X - 1)(X - x_last)): two synthetic divisions by monic linear factors, each remainder dropped.
  Floor division by monic polynomials composes, so this is p_divmod's quotient whatever the remainder (stark.py:81-104).
* The linear combination l, the packed Merkle tree, the spot checks and FRI follow pyoracle.mk_stark_proof, quirks
  included (the `(g2^steps)^(precision-1)` scalar, get_pseudorandom_ks, exclude_multiples_of = ext).

tests/test_stark_oracle.py pins it byte for byte to pyoracle.mk_stark_proof and to the reference's own proofs
(tests/golden/stark.json); tests/golden/generate_large.py --fast writes the at-size STARK fixtures with it.
"""
from oracle import coracle
from oracle.pyoracle import (MIMC_P, f_inv, get_index_in_permuted, get_pseudorandom_ks, mv_degree, stark_flat)

__all__ = ["mk_stark_proof_fast", "stark_flat"]


def _wire(vals):
    return b"".join((int(v) % MIMC_P).to_bytes(32, "big") for v in vals)


def _pad(buf, n):
    return buf + bytes(32 * n - len(buf))


def _terms(poly, width):
    """multivariate_polynomial.py:329-338 visits the terms in sorted order; the value does not depend on it."""
    items = sorted(poly.items())
    coefs = _wire(c for _, c in items)
    exps = b"".join(bytes(e) for e, _ in items)
    assert all(len(e) == width and max(e, default=0) <= 255 for e, _ in items)
    return coefs, exps, len(items)


def _unpack_fri(flat, n, maxdeg_plus_1, samples=40):
    """The flat FRI proof (oracle.c:fri_rec layout) -> prove_low_degree's list structure (fri.py:189-266)."""
    out, off = [], 0
    while maxdeg_plus_1 > 16:
        lg = n.bit_length() - 1
        root2 = flat[off:off + 32]
        off += 32
        branches = []
        for _ in range(samples):
            yb = []
            for size in [lg - 1] + [lg + 1] * 4:
                yb.append([flat[off + 32 * i:off + 32 * i + 32] for i in range(size)])
                off += 32 * size
            branches.append(yb)
        out.append([root2, branches])
        n //= 4
        maxdeg_plus_1 //= 4
        samples = 40  # fri.py:262-266: the recursion does not forward the sample count
    out.append([flat[off + 32 * i:off + 32 * i + 32] for i in range(n)])
    assert off + 32 * n == len(flat)
    return out


def _packed_branch(nodes, cols, k, n, index):
    """merkle_tree.py:59-68 over merkelize_polynomial_evaluations' tree: the leaf, its sibling leaf (both raw
    concatenations of the k column values), then the hashed siblings up to the root's child."""
    q = n // 4

    def leaf(pj):
        x = (pj & 3) * q + (pj >> 2)
        return b"".join(cols[32 * (e * n + x):32 * (e * n + x) + 32] for e in range(k))

    idx = get_index_in_permuted(index, n) + n
    o = [leaf(idx - n), leaf((idx ^ 1) - n)]
    idx //= 2
    while idx > 1:
        o.append(nodes[32 * (idx ^ 1):32 * (idx ^ 1) + 32])
        idx //= 2
    return o


def mk_stark_proof_fast(witness, inputs, step_polys, steps, ext, samples=80, p=MIMC_P):
    """STARK.mk_proof (stark.py:233-279) -> [m_root, l_root, branches, fri_proof], the same bytes as
    pyoracle.mk_stark_proof (feed it to pyoracle.stark_flat).  witness[dim][step], step_polys: {exponent tuple: coeff}."""
    assert p == MIMC_P, "the C oracle works over the MiMC prime only"
    L = coracle.lib()
    width = len(witness)
    precision = n = steps * ext
    degree = max(mv_degree(sp) for sp in step_polys)                                  # stark.py:230-231
    assert steps >= 2 and degree * (steps - 1) + 1 < n, "C (X - x_last) must fit the precision domain"
    g2 = pow(7, (p - 1) // precision, p)                                              # stark.py:205
    g1 = pow(g2, ext, p)                                                              # stark.py:208
    last = pow(g2, (steps - 1) * ext, p)                                              # stark.py:212
    last_w = last.to_bytes(32, "big")
    # P_j (stark.py:27-36) and its evaluations on the precision domain (stark.py:253-256)
    tps = [coracle.fft_bytes(_wire(col), steps, g1, inverse=True) for col in witness]
    p_evals = b"".join(coracle.fft_bytes(tp, n, g2) for tp in tps)
    # C_j on the domain -> exact coefficients -> D_j (stark.py:38-79)
    ds = []
    for j, sp in enumerate(step_polys):
        coefs, exps, nterms = _terms(sp, width)
        c_ev = bytes(32 * n)
        L.or_stark_c(p_evals, width, n, ext, j, coefs, exps, nterms, c_ev)
        c_coef = coracle.fft_bytes(c_ev, n, g2, inverse=True)
        d = bytes(32 * n)
        assert L.or_stark_d(c_coef, n, steps, last_w, d) == 0, "constraint polynomial is not a multiple of Z (stark.py:76)"
        ds.append(d)
    # B_j = (P_j - I_j) / ((X - 1)(X - x_last)), I_j through (1, input_j), (x_last, output_j) (stark.py:81-104,
    # poly_utils.py:397-410)
    bs = []
    one_w = (1).to_bytes(32, "big")
    for j in range(width):
        inp, out = inputs[j] % p, witness[j][-1] % p
        slope = (out - inp) * f_inv((last - 1) % p, p) % p
        a = [int.from_bytes(tps[j][0:32], "big"), int.from_bytes(tps[j][32:64], "big")]
        a = _wire([a[0] - (inp - slope), a[1] - slope]) + tps[j][64:]
        b1 = bytes(32 * (steps - 1))
        L.or_div_linear(a, steps, one_w, b1)
        b2 = bytes(32 * (steps - 2))
        if steps > 2:
            L.or_div_linear(b1, steps - 1, last_w, b2)
        bs.append(b2)
    # evaluations of P, D, B -> the packed tree (stark.py:253-257, merkle_tree.py:94-119)
    cols = p_evals + b"".join(coracle.fft_bytes(d, n, g2) for d in ds) + b"".join(coracle.fft_bytes(b, n, g2) for b in bs)
    k = 3 * width
    mnodes = bytes(32 * n)
    L.or_merkelize_columns(cols, k, n, mnodes)
    m_root = mnodes[32:64]
    # l = sum_j (1 + lk_j c) (D_j + (k1 + k2 c) P_j + (k3 + k4 c) B_j): the terms of stark.py:128-177, regrouped
    k1, k2, k3, k4 = [v % p for v in get_pseudorandom_ks(m_root, 4)]
    c = pow(pow(g2, steps, p), precision - 1, p)
    l_ks = get_pseudorandom_ks(m_root, width)
    scal = [0] * k
    for j in range(width):
        f = (1 + l_ks[j] % p * c) % p
        scal[j] = f * (k1 + k2 * c) % p
        scal[width + j] = f
        scal[2 * width + j] = f * (k3 + k4 * c) % p
    coef_cols = b"".join(_pad(tp, n) for tp in tps) + b"".join(ds) + b"".join(_pad(b, n) for b in bs)
    l_coef = bytes(32 * n)
    L.or_lincomb(coef_cols, k, n, _wire(scal), l_coef)
    l_evals = coracle.fft_bytes(l_coef, n, g2)                                        # stark.py:262
    lnodes = coracle.merkelize_bytes(l_evals)                                         # stark.py:263
    l_root = lnodes[32:64]
    positions = coracle.pseudorandom_indices(l_root, precision, samples, exclude=ext)
    branches = []
    for pos in positions:                                                             # stark.py:390-402
        branches.append(_packed_branch(mnodes, cols, k, n, pos))
        branches.append(_packed_branch(mnodes, cols, k, n, (pos + ext) % precision))
        branches.append(coracle.mk_branch_bytes(lnodes, pos))
    fri_flat = coracle.fri_prove_flat(l_coef, g2, steps * degree, ext, 40, n=n)      # stark.py:271-276
    return [m_root, l_root, branches, _unpack_fri(fri_flat, n, steps * degree)]
