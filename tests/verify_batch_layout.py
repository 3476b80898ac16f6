"""Byte regions of the flat STARK and FRI proofs (include/starkhip.h), for the batch-verifier tests: every region a verifier reads gets
bit flips of its own."""
import random


def _lg(n):
    return n.bit_length() - 1


def fri_regions(n, maxdeg_plus_1, samples, off=0, tag="fri"):
    """-> [(name, begin, end)] of the FRI proof at byte `off`, and its end."""
    out, first, md, r = [], True, maxdeg_plus_1, 0
    while md > 16 and n >= 16:
        s = samples if first else 40
        lg = _lg(n)
        l1, l2 = lg + 1, lg - 1
        per = 32 * (l2 + 4 * l1)
        out.append(("%s_r%d_root2" % (tag, r), off, off + 32))
        out.append(("%s_r%d_column" % (tag, r), off + 32, off + 32 + 32 * l2))  # sample 0's; the flips below pick a sample
        out.append(("%s_r%d_rows" % (tag, r), off + 32 + 32 * l2, off + 32 + per))
        out.append(("%s_r%d_samples" % (tag, r), off + 32, off + 32 + s * per))
        off += 32 + s * per
        n //= 4
        md //= 4
        first = False
        r += 1
    out.append(("%s_final" % tag, off, off + 32 * n))
    return out, off + 32 * n


def stark_regions(steps, ext, width, degree, samples):
    n = steps * ext
    lg = _lg(n)
    pb, lb = 32 * (6 * width + lg - 1), 32 * (lg + 1)
    per = 2 * pb + lb
    out = [("m_root", 0, 32), ("l_root", 32, 64), ("branch_p", 64, 64 + pb), ("branch_p_next", 64 + pb, 64 + 2 * pb),
           ("branch_l", 64 + 2 * pb, 64 + per), ("branches_last_sample", 64 + per * (samples - 1), 64 + per * samples)]
    fr, end = fri_regions(n, steps * degree, 40, 64 + per * samples)
    return out + fr, end


def flips(flat, regions, per_region, seed):
    """-> [(region name, flipped copy)]: per_region single-bit flips inside each region."""
    rng = random.Random(seed)
    out = []
    for name, a, b in regions:
        for _ in range(per_region):
            bad = bytearray(flat)
            bad[rng.randrange(a, b)] ^= 1 << rng.randrange(8)
            out.append((name, bytes(bad)))
    return out


def wrong_fold_fri(coeffs, n, w, maxdeg_plus_1, exclude=0, samples=40, nudge=1):
    """A flat FRI proof (oracle/coracle.py) of the polynomial `coeffs` over the n-point domain of w whose first column is the fold at
    special_x + nudge instead of at special_x = the committed root, with everything after it honest: every Merkle branch verifies and
    the later rounds and the final layer are a valid proof of that column, so only the first round's row checks can reject it
    (nudge = 0 gives the honest proof).  -> (flat, committed root)."""
    from oracle import coracle as co
    P = 2**256 - 2**32 * 351 + 1
    wire = lambda vals: b"".join((int(v) % P).to_bytes(32, "big") for v in vals)
    values = co.fft(list(coeffs) + [0] * (n - len(coeffs)), n, w)
    nodes = co.merkelize_bytes(wire(values))
    root = nodes[32:64]
    sx = ((int.from_bytes(root, "big") + nudge) % 2**256).to_bytes(32, "big")
    column = co.fold(values, w, sx)
    nodes2 = co.merkelize_bytes(wire(column))
    q = n // 4
    ys = co.pseudorandom_indices(nodes2[32:64], q, samples, exclude)
    out = [nodes2[32:64]]
    for y in ys:
        out += co.mk_branch_bytes(nodes2, y)
        for j in range(4):
            out += co.mk_branch_bytes(nodes, y + q * j)
    w4 = pow(w, 4, P)
    col_coeffs = co.fft(column, q, w4, inverse=True)
    out.append(co.fri_prove_flat(wire(col_coeffs), w4, maxdeg_plus_1 // 4, exclude, 40))
    return b"".join(out), root
