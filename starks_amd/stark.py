"""STARK.mk_proof / verify_proof (starks/stark.py:179-402) with the prover on the MI355X.

    stark = STARK(field, steps, extension_factor, width, step_polys)
    proof = stark.mk_proof(witness, boundary)          # [m_root, l_root, branches, fri_proof]
    assert stark.verify_proof(proof, witness, boundary)

`mk_proof` is one call into libstarkhip.so (sh_stark_prove, csrc/api_stark.hip:run_stark; over a field other than the MiMC prime's
sh_mod_stark_prove, csrc/api_modstark.hip, for any odd prime below 2^256 over which 7^((p - 1) // (steps * ext)) has full order): low-degree extension, the
constraint quotient D and boundary quotient B, the packed Merkle tree, the pseudorandom linear combination, the spot
checks and the FRI commit all run on the device and one copy brings the flat proof back.  The reference builds D and B
with O(n^2) coefficient arithmetic (stark.py:38-104); the device computes the same polynomials through the evaluation
domain (see csrc/stark.hip), so every root and proof byte is identical.  The verifier is host-side Python on ints.

starks/stark.py does not import at the reference snapshot (stark.py:13 wants a class fri.py keeps commented out), but
its code runs unchanged once that name exists; tests/golden/generate.py does exactly that to produce the fixtures this
module is tested against (tests/golden/stark.json).
"""
import ctypes

from . import _lib, fri
from ._lib import MIMC_P
from .merkle_tree import blake, mk_branch, verify_branch, unpack_merkle_leaf
from .utils import get_pseudorandom_indices

SPOT_CHECKS = 80  # compute_merkle_spot_checks' default, which mk_proof never overrides (stark.py:265, 390)


def get_pseudorandom_ks(m_root, num):
    """stark.py:106-126.  NB the suffixes are the ASCII strings "0x01".. (4 bytes each), not single bytes, and the
    two branches number from 1 and from 0 respectively -- both exactly as in the reference."""
    if 0 <= num <= 4:
        suffixes = [b"0x01", b"0x02", b"0x03", b"0x04"]
    elif num < 10:
        suffixes = [("0x0%s" % i).encode("UTF-8") for i in range(num)]
    else:
        return None  # the reference falls off the end and returns None
    return [int.from_bytes(blake(m_root + suffixes[i]), "big") for i in range(num)]


def compute_merkle_spot_checks(mtree, l_mtree, precision, extension_factor, samples=80):
    """STARK.compute_merkle_spot_checks (stark.py:390-402) on host-side trees: for each sampled position (multiples of
    the extension factor excluded) the branches of mtree at pos and pos + extension_factor and of l_mtree at pos."""
    branches = []
    positions = get_pseudorandom_indices(l_mtree[1], precision, samples, exclude_multiples_of=extension_factor)
    for pos in positions:
        branches.append(mk_branch(mtree, pos))
        branches.append(mk_branch(mtree, (pos + extension_factor) % precision))
        branches.append(mk_branch(l_mtree, pos))
    return branches


def pack_step_polys(step_polys, width, p=MIMC_P):
    """-> (term_coefs bytes, term_exps bytes, term_counts array, degree): the sparse-term form sh_stark_prove takes.
    Terms go in sorted monomial order, the order MultivariatePolynomial.__call__ visits them (:329-338)."""
    coefs, exps, counts, degree = bytearray(), bytearray(), [], 0
    for poly in step_polys:
        items = sorted(poly.coefficients.items())
        if not items:  # the zero polynomial: one zero term keeps the layout rectangular
            items = [((0,) * width, 0)]
        counts.append(len(items))
        for k, c in items:
            if len(k) != width or max(k) > 255:
                raise ValueError("bad power tuple %r" % (k,))
            coefs += (int(c) % p).to_bytes(32, "big")
            exps += bytes(k)
            degree = max(degree, sum(k) if int(c) % p else 0)
    return bytes(coefs), bytes(exps), (ctypes.c_uint32 * width)(*counts), degree


def proof_len(steps, ext, width, degree, samples=SPOT_CHECKS):
    return int(_lib.lib().sh_stark_proof_len(steps, ext, width, degree, samples))


def unpack_proof(flat, steps, ext, width, degree, samples=SPOT_CHECKS):
    """Flat device proof (layout in include/starkhip.h) -> [m_root, l_root, branches, fri_proof]."""
    n = steps * ext
    lg = n.bit_length() - 1
    k = 3 * width
    m_root, l_root = flat[0:32], flat[32:64]
    off = 64
    branches = []
    for _ in range(samples):
        for _ in range(2):
            br = [flat[off:off + 32 * k], flat[off + 32 * k:off + 64 * k]]
            off += 64 * k
            br.extend(flat[off + 32 * i:off + 32 * i + 32] for i in range(lg - 1))
            off += 32 * (lg - 1)
            branches.append(br)
        branches.append([flat[off + 32 * i:off + 32 * i + 32] for i in range(lg + 1)])
        off += 32 * (lg + 1)
    return [m_root, l_root, branches, fri.unpack_proof(flat[off:], n, steps * degree, 40)]


def pack_proof(proof):
    """[m_root, l_root, branches, fri_proof] -> the flat layout (the inverse of unpack_proof)."""
    m_root, l_root, branches, fri_proof = proof
    return m_root + l_root + b"".join(b"".join(br) for br in branches) + fri.pack_proof(fri_proof)


def prove_flat(witness_bytes, input_bytes, steps, ext, width, step_polys, batch=1, samples=SPOT_CHECKS):
    """witness_bytes: [batch][width][steps] wire form, input_bytes: [batch][width] -> batch flat proofs (concatenated)."""
    if len(witness_bytes) != 32 * batch * width * steps or len(input_bytes) != 32 * batch * width:
        raise ValueError("witness must hold batch*width*steps and inputs batch*width 32-byte elements "
                         "(got %d and %d bytes for batch=%d, width=%d, steps=%d)"
                         % (len(witness_bytes), len(input_bytes), batch, width, steps))
    coefs, exps, counts, degree = pack_step_polys(step_polys, width)
    plen = proof_len(steps, ext, width, degree, samples)
    if plen == 0:
        raise NotImplementedError("starks_amd.STARK: unsupported shape (steps=%d, ext=%d, width=%d, degree=%d)"
                                  % (steps, ext, width, degree))
    out = ctypes.create_string_buffer(plen * batch)
    rc = _lib.lib().sh_stark_prove(_lib.ctx(), witness_bytes, input_bytes, steps, ext, width, coefs, exps, counts, samples,
                                   batch, out, plen * batch)
    if rc == -8:  # SH_ERR_CONSTRAINT: the reference's `assert cp % z == 0` (stark.py:76)
        raise AssertionError("constraint polynomial is not a multiple of Z: the witness is not a valid trace")
    _lib.check(rc, "sh_stark_prove")
    return out.raw


def mod_prove_flat(modulus, witness_bytes, input_bytes, steps, ext, width, step_polys, batch=1, samples=SPOT_CHECKS):
    """prove_flat over any prime modulus below 2^256 (sh_mod_stark_prove): the same arguments and the same flat layout and length; any
    256-bit witness, input or coefficient value is taken modulo `modulus`.  G2 = 7^((p - 1) // (steps * ext)) must have order steps * ext."""
    if len(witness_bytes) != 32 * batch * width * steps or len(input_bytes) != 32 * batch * width:
        raise ValueError("witness must hold batch*width*steps and inputs batch*width 32-byte elements "
                         "(got %d and %d bytes for batch=%d, width=%d, steps=%d)"
                         % (len(witness_bytes), len(input_bytes), batch, width, steps))
    coefs, exps, counts, degree = pack_step_polys(step_polys, width, p=modulus)
    plen = proof_len(steps, ext, width, degree, samples)
    if plen == 0:
        raise NotImplementedError("starks_amd.STARK: unsupported shape (steps=%d, ext=%d, width=%d, degree=%d)"
                                  % (steps, ext, width, degree))
    out = ctypes.create_string_buffer(plen * batch)
    rc = _lib.lib().sh_mod_stark_prove(_lib.ctx(), int(modulus).to_bytes(32, "big"), bytes(witness_bytes), bytes(input_bytes), steps, ext,
                                       width, coefs, exps, counts, samples, batch, out, plen * batch)
    if rc == -8:  # SH_ERR_CONSTRAINT: the reference's `assert cp % z == 0` (stark.py:76)
        raise AssertionError("constraint polynomial is not a multiple of Z: the witness is not a valid trace")
    _lib.check(rc, "sh_mod_stark_prove")
    return out.raw


def unsupported_field_reason(modulus, precision):
    """None when STARK runs over Z/modulus on a domain of `precision` points (the MiMC prime, or an odd modulus below 2^256 over which
    the reference's G2 = 7^((p - 1) // precision) has order precision), else the reason it does not."""
    if modulus == MIMC_P:
        return None
    if modulus < 3 or modulus % 2 == 0:
        return "the modulus %d is even or below 3 (the generic prover takes odd prime moduli)" % modulus
    if modulus >> 256:
        return "the modulus is 2^256 or more"
    if precision < 2 or precision & (precision - 1) or pow(pow(7, (modulus - 1) // precision, modulus), precision // 2, modulus) != modulus - 1:
        return ("7 is not of full 2-power order: G2 = 7^((p - 1) // %d) does not have order %d modulo %d (7 is a quadratic residue, or "
                "p - 1 has too few factors of two)" % (precision, precision, modulus))
    return None


def verify_flat(flat, input_bytes, output_bytes, steps, ext, width, step_polys, samples=SPOT_CHECKS):
    """The library's own verifier (sh_stark_verify: host C++ behind the C ABI; the decisions of STARK.verify_proof below) on a FLAT
    proof as prove_flat returns it.  input_bytes / output_bytes: [width] wire-form boundary inputs and witness[dim][-1]."""
    coefs, exps, counts, _ = pack_step_polys(step_polys, width)
    rc = _lib.lib().sh_stark_verify(bytes(flat), len(flat), bytes(input_bytes), bytes(output_bytes), steps, ext, width, coefs, exps,
                                    counts, samples)
    if rc == -9:
        raise AssertionError("STARK proof rejected")
    _lib.check(rc, "sh_stark_verify")
    return True


def verify_flat_batch(flats, input_bytes, output_bytes, steps, ext, width, step_polys, batch, samples=SPOT_CHECKS):
    """`batch` flat proofs of one shape verified on the GPU in one call (sh_stark_verify_batch): flats = the proofs back to back,
    input_bytes / output_bytes = [batch][width] wire-form boundary inputs and witness[dim][-1].  -> [bool] per proof, each the
    decision verify_flat takes on that proof alone.  Shape errors raise as verify_flat raises them."""
    coefs, exps, counts, _ = pack_step_polys(step_polys, width)
    flats = bytes(flats)
    if batch < 1 or len(flats) % batch:
        raise ValueError("flats must hold batch proofs of equal length")
    status = (ctypes.c_int32 * batch)()
    rc = _lib.lib().sh_stark_verify_batch(_lib.ctx(), flats, len(flats) // batch, bytes(input_bytes), bytes(output_bytes), steps, ext,
                                          width, coefs, exps, counts, samples, batch, status)
    _lib.check(rc, "sh_stark_verify_batch")  # a shape error, or a proof length that is not the shape's
    return [s == 0 for s in status]


def mod_verify_flat(modulus, flat, input_bytes, output_bytes, steps, ext, width, step_polys, samples=SPOT_CHECKS):
    """verify_flat over any prime modulus below 2^256 (sh_mod_stark_verify: host C++, no context, no GPU; the decisions of
    STARK.verify_proof over IntegersModP(modulus)) on a FLAT proof as mod_prove_flat returns it.  Every value is taken modulo `modulus`."""
    coefs, exps, counts, _ = pack_step_polys(step_polys, width, p=modulus)
    rc = _lib.lib().sh_mod_stark_verify(int(modulus).to_bytes(32, "big"), bytes(flat), len(flat), bytes(input_bytes), bytes(output_bytes),
                                        steps, ext, width, coefs, exps, counts, samples)
    if rc == -9:
        raise AssertionError("STARK proof rejected")
    _lib.check(rc, "sh_mod_stark_verify")
    return True


def mod_verify_flat_batch(modulus, flats, input_bytes, output_bytes, steps, ext, width, step_polys, batch, samples=SPOT_CHECKS):
    """verify_flat_batch over any prime modulus below 2^256 (sh_mod_stark_verify_batch): `batch` flat proofs of one shape verified on the
    GPU in one call.  -> [bool] per proof, each the decision mod_verify_flat takes on that proof alone."""
    coefs, exps, counts, _ = pack_step_polys(step_polys, width, p=modulus)
    flats = bytes(flats)
    if batch < 1 or len(flats) % batch:
        raise ValueError("flats must hold batch proofs of equal length")
    status = (ctypes.c_int32 * batch)()
    rc = _lib.lib().sh_mod_stark_verify_batch(_lib.ctx(), int(modulus).to_bytes(32, "big"), flats, len(flats) // batch, bytes(input_bytes),
                                              bytes(output_bytes), steps, ext, width, coefs, exps, counts, samples, batch, status)
    _lib.check(rc, "sh_mod_stark_verify_batch")  # a shape error, or a proof length that is not the shape's
    return [s == 0 for s in status]


def witness_flat(input_bytes, steps, width, step_polys, batch=1):
    """AIR.generate_witness / get_computational_trace (air.py:32-52, 121-123) on the GPU (sh_stark_witness): input_bytes [batch][width]
    wire form (values may be >= p) -> the witness [batch][width][steps] in wire form, what prove_flat takes.  Any steps >= 1."""
    if len(input_bytes) != 32 * batch * width:
        raise ValueError("inputs must hold batch*width 32-byte elements (got %d bytes for batch=%d, width=%d)"
                         % (len(input_bytes), batch, width))
    coefs, exps, counts, _ = pack_step_polys(step_polys, width)
    nbytes = 32 * batch * width * steps
    out = ctypes.create_string_buffer(nbytes)
    _lib.check(_lib.lib().sh_stark_witness(_lib.ctx(), bytes(input_bytes), steps, width, coefs, exps, counts, batch, out, nbytes),
               "sh_stark_witness")
    return out.raw


def prove_inputs_flat(input_bytes, steps, ext, width, step_polys, batch=1, samples=SPOT_CHECKS):
    """Proofs straight from the inputs: upload them, then sh_dev_stark_witness -> sh_dev_stark_prove -> sh_stark_status on device
    buffers (the witness never leaves the device).  -> (batch flat proofs concatenated, outputs): outputs = witness[b][dim][-1] as
    [batch][width] wire form, the values sh_stark_verify / verify_flat_batch take beside the inputs."""
    if len(input_bytes) != 32 * batch * width:
        raise ValueError("inputs must hold batch*width 32-byte elements (got %d bytes for batch=%d, width=%d)"
                         % (len(input_bytes), batch, width))
    coefs, exps, counts, degree = pack_step_polys(step_polys, width)
    plen = proof_len(steps, ext, width, degree, samples)
    if plen == 0:
        raise NotImplementedError("starks_amd.STARK: unsupported shape (steps=%d, ext=%d, width=%d, degree=%d)"
                                  % (steps, ext, width, degree))
    L, ctx = _lib.lib(), _lib.ctx()
    di, dw, dp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    try:
        for ptr, nbytes in ((di, 32 * batch * width), (dw, 32 * batch * width * steps), (dp, plen * batch)):
            _lib.check(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)), "sh_dev_alloc")
        _lib.check(L.sh_dev_from_wire(ctx, bytes(input_bytes), di, batch * width), "sh_dev_from_wire")
        _lib.check(L.sh_dev_stark_witness(ctx, di, steps, width, coefs, exps, counts, batch, dw), "sh_dev_stark_witness")
        _lib.check(L.sh_dev_stark_prove(ctx, dw, di, steps, ext, width, coefs, exps, counts, samples, batch, dp), "sh_dev_stark_prove")
        rc = L.sh_stark_status(ctx)
        if rc == -8:  # a generated witness is a valid trace by construction: this would be a library fault
            raise AssertionError("constraint polynomial is not a multiple of Z: the generated witness is not a valid trace")
        _lib.check(rc, "sh_stark_status")
        proofs = ctypes.create_string_buffer(plen * batch)
        _lib.check(L.sh_dev_download(ctx, dp, proofs, plen * batch), "sh_dev_download")
        last = ctypes.create_string_buffer(32 * batch * width)  # witness[b][dim][steps - 1], canonical limb form
        _lib.check(L.sh_dev_download_2d(ctx, ctypes.c_void_p(dw.value + 32 * (steps - 1)), 32 * steps, last, 32, batch * width),
                   "sh_dev_download_2d")
    finally:
        for ptr in (di, dw, dp):
            if ptr.value:
                L.sh_dev_free(ctx, ptr)
    raw = last.raw
    outputs = b"".join(raw[i:i + 32][::-1] for i in range(0, len(raw), 32))  # limbs are little-endian: reversed = wire form
    return proofs.raw, outputs


def mod_witness_flat(modulus, input_bytes, steps, width, step_polys, batch=1):
    """witness_flat over any odd modulus 3 <= p < 2^256, composite ones included (sh_mod_stark_witness): input_bytes [batch][width]
    wire form (values may be >= p) -> the witness [batch][width][steps] in canonical wire form, what mod_prove_flat takes.  Any
    steps >= 1."""
    if len(input_bytes) != 32 * batch * width:
        raise ValueError("inputs must hold batch*width 32-byte elements (got %d bytes for batch=%d, width=%d)"
                         % (len(input_bytes), batch, width))
    coefs, exps, counts, _ = pack_step_polys(step_polys, width, p=modulus)
    nbytes = 32 * batch * width * steps
    out = ctypes.create_string_buffer(nbytes)
    _lib.check(_lib.lib().sh_mod_stark_witness(_lib.ctx(), int(modulus).to_bytes(32, "big"), bytes(input_bytes), steps, width, coefs, exps,
                                               counts, batch, out, nbytes), "sh_mod_stark_witness")
    return out.raw


def mod_prove_inputs_flat(modulus, input_bytes, steps, ext, width, step_polys, batch=1, samples=SPOT_CHECKS):
    """prove_inputs_flat over any prime modulus the generic prover takes: upload the inputs as little-endian limbs, then
    sh_dev_mod_stark_witness -> sh_dev_mod_stark_prove -> sh_stark_status on device buffers (the witness never leaves the device).
    -> (batch flat proofs concatenated, outputs): outputs = witness[b][dim][-1] as [batch][width] wire form."""
    if len(input_bytes) != 32 * batch * width:
        raise ValueError("inputs must hold batch*width 32-byte elements (got %d bytes for batch=%d, width=%d)"
                         % (len(input_bytes), batch, width))
    coefs, exps, counts, degree = pack_step_polys(step_polys, width, p=modulus)
    plen = proof_len(steps, ext, width, degree, samples)
    if plen == 0:
        raise NotImplementedError("starks_amd.STARK: unsupported shape (steps=%d, ext=%d, width=%d, degree=%d)"
                                  % (steps, ext, width, degree))
    L, ctx = _lib.lib(), _lib.ctx()
    pb = int(modulus).to_bytes(32, "big")
    raw_in = bytes(input_bytes)
    limbs = b"".join(raw_in[i:i + 32][::-1] for i in range(0, len(raw_in), 32))  # wire form reversed = little-endian limbs
    di, dw, dp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    try:
        for ptr, nbytes in ((di, 32 * batch * width), (dw, 32 * batch * width * steps), (dp, plen * batch)):
            _lib.check(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)), "sh_dev_alloc")
        _lib.check(L.sh_dev_upload(ctx, limbs, di, len(limbs)), "sh_dev_upload")
        _lib.check(L.sh_dev_mod_stark_witness(ctx, pb, di, steps, width, coefs, exps, counts, batch, dw), "sh_dev_mod_stark_witness")
        _lib.check(L.sh_dev_mod_stark_prove(ctx, pb, dw, di, steps, ext, width, coefs, exps, counts, samples, batch, dp),
                   "sh_dev_mod_stark_prove")
        rc = L.sh_stark_status(ctx)
        if rc == -8:  # a generated witness is a valid trace by construction: this would be a library fault
            raise AssertionError("constraint polynomial is not a multiple of Z: the generated witness is not a valid trace")
        _lib.check(rc, "sh_stark_status")
        proofs = ctypes.create_string_buffer(plen * batch)
        _lib.check(L.sh_dev_download(ctx, dp, proofs, plen * batch), "sh_dev_download")
        last = ctypes.create_string_buffer(32 * batch * width)  # witness[b][dim][steps - 1], plain canonical limbs
        _lib.check(L.sh_dev_download_2d(ctx, ctypes.c_void_p(dw.value + 32 * (steps - 1)), 32 * steps, last, 32, batch * width),
                   "sh_dev_download_2d")
    finally:
        for ptr in (di, dw, dp):
            if ptr.value:
                L.sh_dev_free(ctx, ptr)
    raw = last.raw
    outputs = b"".join(raw[i:i + 32][::-1] for i in range(0, len(raw), 32))
    return proofs.raw, outputs


def mod64_prove_flat(modulus, witness_words, input_words, steps, ext, width, step_polys, batch=1, samples=SPOT_CHECKS):
    """mod_prove_flat over any prime modulus below 2^64 on packed 64-bit words (sh_mod64_stark_prove): witness_words = batch * width *
    steps and input_words = batch * width native 8-byte words (the buffers fft.mod64_ntt takes: bytes, array('Q'), a numpy uint64
    array, or a sequence of ints; any 64-bit values, taken modulo `modulus`) -> batch flat proofs, byte for byte mod_prove_flat's over
    the same modulus on the same values.  STARK.mk_proof does not route here: it keeps the 32-byte path for every modulus."""
    from .fft import _words
    wsrc, _wkeep, wcount = _words(witness_words)
    isrc, _ikeep, icount = _words(input_words)
    if wcount != batch * width * steps or icount != batch * width:
        raise ValueError("witness must hold batch*width*steps and inputs batch*width 8-byte words "
                         "(got %d and %d words for batch=%d, width=%d, steps=%d)" % (wcount, icount, batch, width, steps))
    coefs, exps, counts, degree = pack_step_polys(step_polys, width, p=modulus)
    plen = proof_len(steps, ext, width, degree, samples)
    if plen == 0:
        raise NotImplementedError("starks_amd.STARK: unsupported shape (steps=%d, ext=%d, width=%d, degree=%d)"
                                  % (steps, ext, width, degree))
    out = ctypes.create_string_buffer(plen * batch)
    rc = _lib.lib().sh_mod64_stark_prove(_lib.ctx(), int(modulus), wsrc, isrc, steps, ext, width, coefs, exps, counts, samples, batch,
                                         out, plen * batch)
    if rc == -8:  # SH_ERR_CONSTRAINT: the reference's `assert cp % z == 0` (stark.py:76)
        raise AssertionError("constraint polynomial is not a multiple of Z: the witness is not a valid trace")
    _lib.check(rc, "sh_mod64_stark_prove")
    return out.raw


def mod64_prove_inputs_flat(modulus, input_bytes, steps, ext, width, step_polys, batch=1, samples=SPOT_CHECKS):
    """mod_prove_inputs_flat with the packed-word prover: upload the inputs as little-endian limbs, then sh_dev_mod_stark_witness ->
    sh_dev_mod64_from_limbs (witness and inputs) -> sh_dev_mod64_stark_prove -> sh_stark_status on device buffers (the witness never
    leaves the device).  -> (batch flat proofs concatenated, outputs): outputs = witness[b][dim][-1] as [batch][width] wire form."""
    if len(input_bytes) != 32 * batch * width:
        raise ValueError("inputs must hold batch*width 32-byte elements (got %d bytes for batch=%d, width=%d)"
                         % (len(input_bytes), batch, width))
    coefs, exps, counts, degree = pack_step_polys(step_polys, width, p=modulus)
    plen = proof_len(steps, ext, width, degree, samples)
    if plen == 0:
        raise NotImplementedError("starks_amd.STARK: unsupported shape (steps=%d, ext=%d, width=%d, degree=%d)"
                                  % (steps, ext, width, degree))
    L, ctx = _lib.lib(), _lib.ctx()
    pb = int(modulus).to_bytes(32, "big")
    raw_in = bytes(input_bytes)
    limbs = b"".join(raw_in[i:i + 32][::-1] for i in range(0, len(raw_in), 32))  # wire form reversed = little-endian limbs
    cols = batch * width
    di, dw, dwi, dww, dp = (ctypes.c_void_p() for _ in range(5))
    try:
        for ptr, nbytes in ((di, 32 * cols), (dw, 32 * cols * steps), (dwi, 8 * cols), (dww, 8 * cols * steps), (dp, plen * batch)):
            _lib.check(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)), "sh_dev_alloc")
        _lib.check(L.sh_dev_upload(ctx, limbs, di, len(limbs)), "sh_dev_upload")
        _lib.check(L.sh_dev_mod_stark_witness(ctx, pb, di, steps, width, coefs, exps, counts, batch, dw), "sh_dev_mod_stark_witness")
        _lib.check(L.sh_dev_mod64_from_limbs(ctx, int(modulus), dw, dww, cols * steps), "sh_dev_mod64_from_limbs")
        _lib.check(L.sh_dev_mod64_from_limbs(ctx, int(modulus), di, dwi, cols), "sh_dev_mod64_from_limbs")
        _lib.check(L.sh_dev_mod64_stark_prove(ctx, int(modulus), dww, dwi, steps, ext, width, coefs, exps, counts, samples, batch, dp),
                   "sh_dev_mod64_stark_prove")
        rc = L.sh_stark_status(ctx)
        if rc == -8:  # a generated witness is a valid trace by construction: this would be a library fault
            raise AssertionError("constraint polynomial is not a multiple of Z: the generated witness is not a valid trace")
        _lib.check(rc, "sh_stark_status")
        proofs = ctypes.create_string_buffer(plen * batch)
        _lib.check(L.sh_dev_download(ctx, dp, proofs, plen * batch), "sh_dev_download")
        last = ctypes.create_string_buffer(32 * cols)  # witness[b][dim][steps - 1], plain canonical limbs
        _lib.check(L.sh_dev_download_2d(ctx, ctypes.c_void_p(dw.value + 32 * (steps - 1)), 32 * steps, last, 32, cols),
                   "sh_dev_download_2d")
    finally:
        for ptr in (di, dw, dwi, dww, dp):
            if ptr.value:
                L.sh_dev_free(ctx, ptr)
    raw = last.raw
    outputs = b"".join(raw[i:i + 32][::-1] for i in range(0, len(raw), 32))
    return proofs.raw, outputs


def mod64_witness_flat(modulus, input_words, steps, width, step_polys, batch=1):
    """mod_witness_flat on packed 64-bit words over any odd modulus 3 <= p < 2^64, composite ones included (sh_mod64_stark_witness):
    input_words = batch * width native 8-byte words (the buffers fft.mod64_ntt takes; any 64-bit values, taken modulo `modulus`) -> the
    witness [batch][width][steps] as bytes of native words, plain and canonical: what mod64_prove_flat takes.  Any steps >= 1."""
    from .fft import _words
    isrc, _ikeep, icount = _words(input_words)
    if icount != batch * width:
        raise ValueError("inputs must hold batch*width 8-byte words (got %d words for batch=%d, width=%d)" % (icount, batch, width))
    coefs, exps, counts, _ = pack_step_polys(step_polys, width, p=modulus)
    count = batch * width * steps
    out = ctypes.create_string_buffer(8 * count)
    _lib.check(_lib.lib().sh_mod64_stark_witness(_lib.ctx(), int(modulus), isrc, steps, width, coefs, exps, counts, batch, out, count),
               "sh_mod64_stark_witness")
    return out.raw


def mod64_prove_input_words_flat(modulus, input_words, steps, ext, width, step_polys, batch=1, samples=SPOT_CHECKS):
    """mod64_prove_inputs_flat from words, on words throughout: upload the inputs, then sh_dev_mod64_stark_witness ->
    sh_dev_mod64_stark_prove -> sh_stark_status on device buffers (the witness never leaves the device, and no 32-byte copy of it
    exists).  -> (batch flat proofs concatenated, output_words): output_words = witness[b][dim][steps - 1] as [batch][width] native
    words."""
    from .fft import _words
    isrc, _ikeep, icount = _words(input_words)
    cols = batch * width
    if icount != cols:
        raise ValueError("inputs must hold batch*width 8-byte words (got %d words for batch=%d, width=%d)" % (icount, batch, width))
    coefs, exps, counts, degree = pack_step_polys(step_polys, width, p=modulus)
    plen = proof_len(steps, ext, width, degree, samples)
    if plen == 0:
        raise NotImplementedError("starks_amd.STARK: unsupported shape (steps=%d, ext=%d, width=%d, degree=%d)"
                                  % (steps, ext, width, degree))
    L, ctx = _lib.lib(), _lib.ctx()
    raw_in = isrc if isinstance(isrc, bytes) else bytes(isrc)
    di, dw, dp = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    try:
        for ptr, nbytes in ((di, 8 * cols), (dw, 8 * cols * steps), (dp, plen * batch)):
            _lib.check(L.sh_dev_alloc(ctx, nbytes, ctypes.byref(ptr)), "sh_dev_alloc")
        _lib.check(L.sh_dev_upload(ctx, raw_in, di, len(raw_in)), "sh_dev_upload")
        _lib.check(L.sh_dev_mod64_stark_witness(ctx, int(modulus), di, steps, width, coefs, exps, counts, batch, dw),
                   "sh_dev_mod64_stark_witness")
        _lib.check(L.sh_dev_mod64_stark_prove(ctx, int(modulus), dw, di, steps, ext, width, coefs, exps, counts, samples, batch, dp),
                   "sh_dev_mod64_stark_prove")
        rc = L.sh_stark_status(ctx)
        if rc == -8:  # a generated witness is a valid trace by construction: this would be a library fault
            raise AssertionError("constraint polynomial is not a multiple of Z: the generated witness is not a valid trace")
        _lib.check(rc, "sh_stark_status")
        proofs = ctypes.create_string_buffer(plen * batch)
        _lib.check(L.sh_dev_download(ctx, dp, proofs, plen * batch), "sh_dev_download")
        last = ctypes.create_string_buffer(8 * cols)  # witness[b][dim][steps - 1], plain canonical words
        _lib.check(L.sh_dev_download_2d(ctx, ctypes.c_void_p(dw.value + 8 * (steps - 1)), 8 * steps, last, 8, cols), "sh_dev_download_2d")
    finally:
        for ptr in (di, dw, dp):
            if ptr.value:
                L.sh_dev_free(ctx, ptr)
    return proofs.raw, last.raw


class STARK(object):
    """Generates and verifies STARKs (stark.py:179-402); same constructor arguments."""

    def __init__(self, field, steps, extension_factor, width, step_polys, spot_check_security_factor=80):
        self.field = field
        self.width = width
        self.steps = steps
        self.step_polys = step_polys
        self.extension_factor = extension_factor
        self.precision = steps * extension_factor
        self.spot_check_security_factor = spot_check_security_factor
        modulus = int(getattr(field, "p", MIMC_P))
        reason = unsupported_field_reason(modulus, self.precision)
        if reason:  # the MiMC prime runs sh_stark_prove, any other prime with a G2 of full order sh_mod_stark_prove
            raise NotImplementedError("starks_amd.STARK: " + reason)
        self.modulus = modulus
        self.G2 = field(7) ** ((modulus - 1) // self.precision)   # stark.py:205
        self.G1 = self.G2 ** extension_factor                      # stark.py:208
        self.last_step_position = self.G2 ** ((steps - 1) * extension_factor)  # xs[(steps-1)*extension_factor], :212

    def get_degree(self):
        return max([poly.degree() for poly in self.step_polys])

    # ---- prover ----
    def mk_proof(self, witness, boundary):
        """stark.py:233-279.  witness[dim][step]; boundary[dim] = (step, dim, input value)."""
        if len(witness) != self.width or any(len(col) != self.steps for col in witness):
            raise ValueError("witness must be width x steps")
        if len(boundary) < self.width:
            raise IndexError("boundary must hold one (step, dim, value) constraint per dimension")  # boundary[dim], stark.py:91
        p = self.modulus
        wb = b"".join(_lib.to_wire(col, p) for col in witness)
        ib = _lib.to_wire([constraint[2] for constraint in boundary[:self.width]], p)
        if p == MIMC_P:
            flat = prove_flat(wb, ib, self.steps, self.extension_factor, self.width, self.step_polys)
        else:
            flat = mod_prove_flat(p, wb, ib, self.steps, self.extension_factor, self.width, self.step_polys)
        return unpack_proof(flat, self.steps, self.extension_factor, self.width, self.get_degree())

    def compute_merkle_spot_checks(self, mtree, l_mtree, samples=80):
        return compute_merkle_spot_checks(mtree, l_mtree, self.precision, self.extension_factor, samples)

    # ---- verifier (host) ----
    def verify_proof(self, proof, witness, boundary):
        """stark.py:281-316"""
        m_root, l_root, branches, fri_proof = proof
        assert fri.verify_low_degree_proof(fri_proof, l_root, self.G2, self.steps * self.get_degree(),
                                           exclude_multiples_of=self.extension_factor, modulus=self.modulus)
        samples = self.spot_check_security_factor
        positions = get_pseudorandom_indices(l_root, self.precision, samples, exclude_multiples_of=self.extension_factor)
        ks = get_pseudorandom_ks(m_root, 4)
        for i, pos in enumerate(positions):
            self.verify_proof_at_position(witness, boundary, ks, proof, i, pos)
        return True

    def verify_proof_native(self, proof, witness, boundary):
        """The same decision from the library's C verifier (sh_stark_verify) on the packed proof -- about 50 times faster than the
        Python verifier above, which stays the line-by-line mirror of the reference (no arithmetic shared with the device code)."""
        if self.modulus != MIMC_P:
            raise NotImplementedError("starks_amd.STARK.verify_proof_native: there is no C STARK verifier over another modulus; "
                                      "verify_proof is the verifier there")
        inputs = _lib.to_wire([constraint[2] for constraint in boundary[:self.width]])
        outputs = _lib.to_wire([col[-1] for col in witness])
        return verify_flat(pack_proof(proof), inputs, outputs, self.steps, self.extension_factor, self.width, self.step_polys,
                           self.spot_check_security_factor)

    def verify_proof_mod_native(self, proof, witness, boundary):
        """The same decision from the library's C verifier over a run-time modulus (sh_mod_stark_verify) on the packed proof, for
        whatever modulus the STARK was built over, the MiMC prime included."""
        p = self.modulus
        inputs = _lib.to_wire([constraint[2] for constraint in boundary[:self.width]], p)
        outputs = _lib.to_wire([col[-1] for col in witness], p)
        return mod_verify_flat(p, pack_proof(proof), inputs, outputs, self.steps, self.extension_factor, self.width, self.step_polys,
                               self.spot_check_security_factor)

    def verify_proof_at_position(self, witness, boundary, ks, proof, i, pos):
        """stark.py:318-388 (the linear-combination check is commented out there, :376-384, and is not made here)."""
        p, width, ext = self.modulus, self.width, self.extension_factor
        m_root, l_root, branches, _ = proof
        x = pow(int(self.G2), pos, p)
        last = int(self.last_step_position)
        leaf1 = unpack_merkle_leaf(verify_branch(m_root, pos, branches[i * 3]), width, 3)
        leaf2 = unpack_merkle_leaf(verify_branch(m_root, (pos + ext) % self.precision, branches[i * 3 + 1]), width, 3)
        verify_branch(l_root, pos, branches[i * 3 + 2], output_as_int=True)
        v1 = [int.from_bytes(v, "big") % p for v in leaf1]
        p_of_x, d_of_x, b_of_x = v1[:width], v1[width:2 * width], v1[2 * width:]
        p_of_g1x = [int.from_bytes(v, "big") % p for v in leaf2[:width]]
        zvalue = (pow(x, self.steps, p) - 1) * pow((x - last) % p, p - 2, p) % p
        f_of_p_of_x = [int(self.step_polys[d](p_of_x)) for d in range(width)]
        for dim in range(width):  # transition constraints C(P(x)) = Z(x) * D(x)
            assert (p_of_g1x[dim] - f_of_p_of_x[dim] - zvalue * d_of_x[dim]) % p == 0
        z2 = (x - 1) * (x - last) % p
        inv = pow((last - 1) % p, p - 2, p)
        for dim in range(width):  # boundary constraints B(x) * Z2(x) + I(x) = P(x)
            input_value = int(boundary[dim][2])
            output_dim = int(witness[dim][-1])
            slope = (output_dim - input_value) * inv % p
            interpolant = (input_value - slope + slope * x) % p
            assert (p_of_x[dim] - b_of_x[dim] * z2 - interpolant) % p == 0


# the module-level building blocks of mk_proof under the reference's names (stark.py:27-177): see stark_polys.py
from .stark_polys import (construct_trace_polynomials, construct_constraint_polynomials, construct_remainder_polynomials,  # noqa: E402,F401
                          construct_boundary_polynomials, compute_pseudorandom_linear_combination_1d,
                          compute_pseudorandom_linear_combination)
