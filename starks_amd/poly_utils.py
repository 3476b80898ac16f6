"""Batch inversion, four-point interpolation, zpoly and Lagrange interpolation on the MI355X behind the reference's call sites
(starks/poly_utils.py:301-369, 412-440):

    multi_inv(field, values) -> sequence              (one field inversion for all values)
    multi_interp_4(field, xsets, ysets) -> [Poly]      (the cubic through each row's four points)
    zpoly(field, roots) -> Poly                        (prod (X - x_i): a product tree of batched NTTs, O(n log^2 n))
    lagrange_interp(field, xs, ys) -> Poly             (the reference's interpolant, O(n log^2 n) instead of its O(n^3))
    multi_eval(field, poly, xs) -> sequence          (poly(x) at every point: direct Horner lanes or a remainder tree)
    multi_inv_wire(data) -> bytes, multi_interp_4_wire(xs, ys, rows) -> bytes,
    zpoly_wire(xs) -> bytes, lagrange_interp_wire(xs, ys) -> bytes   (wire form in and out, for large inputs)
    mod_multi_inv_wire(p, data), mod_multi_interp_4_wire(p, xs, ys, rows), mod_zpoly_wire(p, xs), mod_lagrange_interp_wire(p, xs, ys)
    (and polynomial.mod_eval_wire(p, coefs, xs, batch))
                                                       (the same over any prime p < 2^256: sh_mod_*, always on the device)

For the MiMC prime they always run on the GPU through libstarkhip.so (sh_multi_inv, sh_multi_interp_4) and raise when the library
or the device is missing: there is no CPU fallback for them.  Another PRIME field goes to the device's generic entries (sh_mod_*)
when the process already holds a context, the call's largest transform fits the field's 2-adicity and the size is at or above the
operation's measured threshold (MOD_DEVICE_MIN, _lib.mod_poly_routable).  Everything else (the reference's own tests use Z/7) is
outside the hot path: there the reference's algorithm runs on the host on the field's own elements, as fft._host_dft does.

The reference's multi_inv tests the truthiness of each value (poly_utils.py:317): a zero Python int comes back as 0, a zero FIELD
ELEMENT -- always truthy -- as 1.  The device computes 0 for every zero; `multi_inv` puts the 1 back where the input was an element
(a WireList holds elements), so both forms give what the reference gives.  multi_interp_4 hands the reference's multi_inv field
elements only, so a row with a repeated x has e_k = 0 "inverted" to 1; the device does the same (include/starkhip.h).
"""
import ctypes

from . import _lib
from ._lib import MIMC_P
from .polynomial import polynomials_over
from .wireseq import WireList


def _on_device(field):
    return int(getattr(field, "p", 0)) == MIMC_P


# Another prime field goes to the device (sh_mod_*, include/starkhip.h) from this many values / rows / points on, when
# _lib.mod_poly_routable holds; None: routing is off for the operation.  Each is the smallest power of two from which the device call
# won end to end at every larger measured size (tools/mod_poly_time.py over BN254 against the host loop on the same inputs in the same
# run, profiles/r21_mod_poly.json, "routing": multi_inv 0.66 ms against 1.07 ms at 512 and 0.66 against 0.56 ms at 256; multi_interp_4
# 0.75 against 0.79 ms at 16 rows; zpoly 0.63 against 1.38 ms at 64 and 0.36 against 0.35 ms at 32; lagrange_interp 3.0 against 9.1 ms
# at 16 and 2.1 against 1.7 ms at 8).
MOD_DEVICE_MIN = {"multi_inv": 512, "multi_interp_4": 16, "zpoly": 64, "lagrange_interp": 16}


def _mod_on_device(field, what, size, op=None):
    least = MOD_DEVICE_MIN[what]
    p = getattr(field, "p", None)
    if least is None or p is None or size < least:
        return False
    return _lib.mod_poly_routable(p, op, size)


def _check_wire(*bufs):
    out = []
    for b in bufs:
        b = bytes(b) if not isinstance(b, bytes) else b
        if len(b) % 32:
            raise ValueError("wire form is a multiple of 32 bytes")
        out.append(b)
    return out


def mod_multi_inv_wire(modulus, data):
    """multi_inv_wire over any prime modulus below 2^256 (sh_mod_multi_inv): n 32-byte big-endian values (any 256-bit value) -> their
    inverses mod p, canonical, 0 for a value == 0 mod p.  Always on the device."""
    data, = _check_wire(data)
    n = len(data) // 32
    if n == 0:
        return b""
    out = ctypes.create_string_buffer(32 * n)
    _lib.check(_lib.lib().sh_mod_multi_inv(_lib.ctx(), int(modulus).to_bytes(32, "big"), data, n, out), "sh_mod_multi_inv")
    return out.raw


def mod_multi_interp_4_wire(modulus, xs, ys, rows):
    """multi_interp_4_wire over any prime modulus below 2^256 (sh_mod_multi_interp_4).  Always on the device."""
    xs, ys = _check_wire(xs, ys)
    if len(xs) != 128 * rows or len(ys) != 128 * rows:
        raise ValueError("xs and ys must hold 4 * rows 32-byte values")
    if rows == 0:
        return b""
    out = ctypes.create_string_buffer(128 * rows)
    _lib.check(_lib.lib().sh_mod_multi_interp_4(_lib.ctx(), int(modulus).to_bytes(32, "big"), xs, ys, rows, out), "sh_mod_multi_interp_4")
    return out.raw


def mod_zpoly_wire(modulus, xs, root=None):
    """zpoly_wire over any prime modulus below 2^256 (sh_mod_zpoly); root = (root of unity, log2 of its order), default
    _lib.two_adic_root(modulus).  Always on the device."""
    xs, = _check_wire(xs)
    n = len(xs) // 32
    m, w, k = _lib.mod_poly_args(modulus, root)
    out = ctypes.create_string_buffer(32 * (n + 1))
    _lib.check(_lib.lib().sh_mod_zpoly(_lib.ctx(), m, w, k, xs, n, out), "sh_mod_zpoly")
    return out.raw


def mod_lagrange_interp_wire(modulus, xs, ys, root=None):
    """lagrange_interp_wire over any prime modulus below 2^256 (sh_mod_lagrange_interp), repeated x's included.  Always on the device."""
    xs, ys = _check_wire(xs, ys)
    if len(ys) != len(xs):
        raise ValueError("xs and ys must hold the same number of 32-byte values")
    n = len(xs) // 32
    if n == 0:
        return b""
    m, w, k = _lib.mod_poly_args(modulus, root)
    out = ctypes.create_string_buffer(32 * n)
    _lib.check(_lib.lib().sh_mod_lagrange_interp(_lib.ctx(), m, w, k, xs, ys, n, out), "sh_mod_lagrange_interp")
    return out.raw


def mod64_multi_inv_words(modulus, data):
    """multi_inv over any prime modulus below 2^64 on packed 64-bit words (sh_mod64_multi_inv): native 8-byte words (a list of ints,
    bytes or any buffer of words; any 64-bit values) -> their inverses mod p, canonical, 0 for a word == 0 mod p; a memoryview of
    format 'Q' over a fresh bytearray.  An entry of its own: multi_inv keeps the 32-byte path.  Always on the device."""
    from .fft import _word_result, _words
    src, _keep, n = _words(data)
    if n == 0:
        return memoryview(bytearray()).cast("Q")
    out, dst = _word_result(n)
    _lib.check(_lib.lib().sh_mod64_multi_inv(_lib.ctx(), _lib.mod64_poly_args(modulus, (1, 0))[0], src, n, dst), "sh_mod64_multi_inv")
    del dst
    return memoryview(out).cast("Q")


def mod64_multi_interp_4_words(modulus, xs, ys):
    """multi_interp_4 over any prime modulus below 2^64 on packed words (sh_mod64_multi_interp_4): xs, ys = [rows][4] words ->
    [rows][4] coefficient words, operands and result as in `mod64_multi_inv_words`.  Always on the device."""
    from .fft import _word_result, _words
    sx, _kx, nx = _words(xs)
    sy, _ky, ny = _words(ys)
    if nx != ny or nx % 4:
        raise ValueError("xs and ys must hold 4 * rows words each")
    if nx == 0:
        return memoryview(bytearray()).cast("Q")
    out, dst = _word_result(nx)
    _lib.check(_lib.lib().sh_mod64_multi_interp_4(_lib.ctx(), _lib.mod64_poly_args(modulus, (1, 0))[0], sx, sy, nx // 4, dst),
               "sh_mod64_multi_interp_4")
    del dst
    return memoryview(out).cast("Q")


def mod64_zpoly_words(modulus, xs, root=None):
    """zpoly over any prime modulus below 2^64 on packed words (sh_mod64_zpoly): n words -> the n + 1 coefficients of
    prod (X - x_i), leading 1 included; root = (root of unity, log2 of its order), default _lib.two_adic_root(modulus).  Always on
    the device."""
    from .fft import _word_result, _words
    sx, _kx, n = _words(xs)
    m, w, k = _lib.mod64_poly_args(modulus, root)
    out, dst = _word_result(n + 1)
    _lib.check(_lib.lib().sh_mod64_zpoly(_lib.ctx(), m, w, k, sx if n else None, n, dst), "sh_mod64_zpoly")
    del dst
    return memoryview(out).cast("Q")


def mod64_lagrange_interp_words(modulus, xs, ys, root=None):
    """lagrange_interp over any prime modulus below 2^64 on packed words (sh_mod64_lagrange_interp), repeated x's included: n + n
    words -> n coefficient words.  Always on the device."""
    from .fft import _word_result, _words
    sx, _kx, n = _words(xs)
    sy, _ky, ny = _words(ys)
    if n != ny:
        raise ValueError("xs and ys must hold the same number of words")
    if n == 0:
        return memoryview(bytearray()).cast("Q")
    m, w, k = _lib.mod64_poly_args(modulus, root)
    out, dst = _word_result(n)
    _lib.check(_lib.lib().sh_mod64_lagrange_interp(_lib.ctx(), m, w, k, sx, sy, n, dst), "sh_mod64_lagrange_interp")
    del dst
    return memoryview(out).cast("Q")


def multi_inv_wire(data):
    """n 32-byte big-endian values (may be >= p) -> their n inverses, canonical, 0 for a value == 0 mod p (sh_multi_inv)."""
    data = bytes(data) if not isinstance(data, bytes) else data
    if len(data) % 32:
        raise ValueError("wire form is a multiple of 32 bytes")
    n = len(data) // 32
    if n == 0:
        return b""
    out = ctypes.create_string_buffer(32 * n)
    _lib.check(_lib.lib().sh_multi_inv(_lib.ctx(), data, n, out), "sh_multi_inv")
    return out.raw


def multi_interp_4_wire(xs, ys, rows):
    """xs, ys: [rows][4] wire form -> [rows][4] coefficients (constant first), canonical wire form (sh_multi_interp_4)."""
    xs = bytes(xs) if not isinstance(xs, bytes) else xs
    ys = bytes(ys) if not isinstance(ys, bytes) else ys
    if len(xs) != 128 * rows or len(ys) != 128 * rows:
        raise ValueError("xs and ys must hold 4 * rows 32-byte values")
    if rows == 0:
        return b""
    out = ctypes.create_string_buffer(128 * rows)
    _lib.check(_lib.lib().sh_multi_interp_4(_lib.ctx(), xs, ys, rows, out), "sh_multi_interp_4")
    return out.raw


def _zero_rows(raw):
    """indices of the all-zero 32-byte records of raw"""
    import numpy as np
    a = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 32)
    return np.flatnonzero(~a.any(axis=1)).tolist()


def multi_inv(field, values):
    """starks/poly_utils.py:301-320: the inverse of every value, one field inversion in all."""
    mimc = _on_device(field)
    if not mimc:
        values = values if isinstance(values, (list, tuple, WireList)) else list(values)
        if not _mod_on_device(field, "multi_inv", len(values)):
            return _host_multi_inv(field, list(values))
    elements = isinstance(values, WireList)
    if not elements and not isinstance(values, (list, tuple)):
        values = list(values)
    out = multi_inv_wire(_lib.to_wire(values)) if mimc else mod_multi_inv_wire(field.p, _lib.to_wire(values, int(field.p)))
    zeros = _zero_rows(out)  # an inverse is 0 exactly where the value is 0 mod p
    if zeros:
        buf = bytearray(out)
        for i in zeros:
            if elements or not isinstance(values[i], int):  # a zero field element is truthy (poly_utils.py:317): 1, not 0
                buf[32 * i + 31] = 1
        out = bytes(buf)
    return WireList(out, field)


def multi_interp_4(field, xsets, ysets):
    """starks/poly_utils.py:412-440: for each row, the polynomial of degree < 4 through (xs[k], ys[k]), k < 4, as a polynomial
    over `field` (trailing zero coefficients stripped, as polysOver does)."""
    xsets, ysets = list(xsets), list(ysets)
    if len(xsets) != len(ysets) or any(len(r) != 4 for r in xsets) or any(len(r) != 4 for r in ysets):
        raise ValueError("multi_interp_4 takes rows of four x and four y values")
    rows = len(xsets)
    if not _on_device(field):
        if not _mod_on_device(field, "multi_interp_4", rows):
            return _host_multi_interp_4(field, xsets, ysets)
        p = int(field.p)
        raw = mod_multi_interp_4_wire(p, b"".join(_lib.to_wire(list(r), p) for r in xsets), b"".join(_lib.to_wire(list(r), p) for r in ysets), rows)
    else:
        raw = multi_interp_4_wire(b"".join(_lib.to_wire(list(r)) for r in xsets), b"".join(_lib.to_wire(list(r)) for r in ysets), rows)
    coeffs = WireList(raw, field)
    polys_over = polynomials_over(field)
    return [polys_over(coeffs[4 * r:4 * r + 4]) for r in range(rows)]


def zpoly_wire(xs):
    """n 32-byte big-endian values (may be >= p) -> the n + 1 coefficients of prod (X - x_i), constant first, canonical (sh_zpoly)."""
    xs = bytes(xs) if not isinstance(xs, bytes) else xs
    if len(xs) % 32:
        raise ValueError("wire form is a multiple of 32 bytes")
    n = len(xs) // 32
    out = ctypes.create_string_buffer(32 * (n + 1))
    _lib.check(_lib.lib().sh_zpoly(_lib.ctx(), xs, n, out), "sh_zpoly")
    return out.raw


def lagrange_interp_wire(xs, ys):
    """n x and n y values in wire form -> the n coefficients (constant first, canonical, not trimmed) of the reference's
    lagrange_interp (sh_lagrange_interp), repeated x's included."""
    xs = bytes(xs) if not isinstance(xs, bytes) else xs
    ys = bytes(ys) if not isinstance(ys, bytes) else ys
    if len(xs) % 32 or len(ys) != len(xs):
        raise ValueError("xs and ys must hold the same number of 32-byte values")
    n = len(xs) // 32
    if n == 0:
        return b""
    out = ctypes.create_string_buffer(32 * n)
    _lib.check(_lib.lib().sh_lagrange_interp(_lib.ctx(), xs, ys, n, out), "sh_lagrange_interp")
    return out.raw


def zpoly(field, roots):
    """starks/poly_utils.py:322-335: the monic polynomial whose roots are `roots` (the reference's debug print is not kept)."""
    polys_over = polynomials_over(field)
    if not _on_device(field):
        roots = list(roots)
        if _mod_on_device(field, "zpoly", len(roots), _lib.MOD_POLY_ZPOLY):
            return polys_over(WireList(mod_zpoly_wire(field.p, _lib.to_wire(roots, int(field.p))), field))
        return polys_over(_host_zpoly(field, roots))
    return polys_over(WireList(zpoly_wire(_lib.to_wire(roots)), field))


def lagrange_interp(field, xs, ys):
    """starks/poly_utils.py:337-369: sum_i y_i / d_i prod_{j != i} (X - x_j), d_i = prod_{j != i} (x_i - x_j), where a zero d_i (a
    repeated x) counts as 1, as the reference's multi_inv has it for field elements (poly_utils.py:317)."""
    xs, ys = list(xs), list(ys)
    assert len(xs) == len(ys)  # the reference: assert len(root) == len(ys) + 1
    polys_over = polynomials_over(field)
    if not _on_device(field):
        if _mod_on_device(field, "lagrange_interp", len(xs), _lib.MOD_POLY_LAGRANGE):
            p = int(field.p)
            return polys_over(WireList(mod_lagrange_interp_wire(p, _lib.to_wire(xs, p), _lib.to_wire(ys, p)), field))
        return _host_lagrange_interp(field, xs, ys)
    return polys_over(WireList(lagrange_interp_wire(_lib.to_wire(xs), _lib.to_wire(ys)), field))


# multi_eval over another prime field makes one sh_mod_poly_eval call from this many coefficients x points on (and at least one of
# each), under _lib.mod_poly_routable with no transform requirement: the smallest power of two from which the device call won end to
# end at every larger measured size (tools/mod_poly_eval_time.py over BN254 against the host loop on the same inputs in the same run,
# profiles/r22_mod_poly_eval.json, "routing": at 8 points 0.109 ms against 0.128 ms for n m = 128 and 0.106 against 0.066 ms for 64; on
# square shapes 0.116 against 0.254 ms for 256 and 0.110 against 0.066 ms for 64).
MOD_EVAL_DEVICE_MIN_WORK = 128
_EVAL_MAX_COEFS, _EVAL_MAX_POINTS = 1 << 25, 1 << 20


def _mod_eval_on_device(field, n, m):
    p = getattr(field, "p", None)
    if p is None or not 0 < n <= _EVAL_MAX_COEFS or not 0 < m <= _EVAL_MAX_POINTS or n * m < MOD_EVAL_DEVICE_MIN_WORK:
        return False
    return _lib.mod_poly_routable(p, None, n)


def multi_eval(field, poly, xs):
    """Polynomial.__call__ (polynomial.py:158-164) at every x of xs: for the MiMC field one sh_poly_eval call, a WireList of the
    field's elements (raises without a device, like multi_inv); for another prime field one sh_mod_poly_eval call and a WireList when
    _mod_eval_on_device holds; for any other ring or size poly(x) per point on the host, a list.  poly is a Polynomial or a sequence
    of coefficients (constant first)."""
    coefficients = poly.coefficients if hasattr(poly, "coefficients") else list(poly)
    if not _on_device(field):
        xs = list(xs)
        if _mod_eval_on_device(field, len(coefficients), len(xs)) and all(isinstance(x, (int, field)) and not isinstance(x, bool) for x in xs):
            from .polynomial import mod_eval_wire
            p = int(field.p)
            return WireList(mod_eval_wire(p, _lib.to_wire(coefficients, p), _lib.to_wire(xs, p)), field)
        p = poly if callable(poly) else polynomials_over(field)(coefficients)
        return [p(x) for x in xs]
    from .polynomial import eval_wire
    return WireList(eval_wire(_lib.to_wire(coefficients), _lib.to_wire(list(xs))), field)


# ---- host forms for other moduli (never the MiMC field) ---------------------------------------------------------------------------
def _host_multi_inv(field, values):
    """The reference's algorithm on the field's own elements (poly_utils.py:301-320), its truthiness test included."""
    partials = [field(1)]
    for val in values:
        partials.append(partials[-1] * (1 if val == 0 else val))
    inv = field(1) / partials[-1]
    outputs = [0] * len(values)
    for i in range(len(values), 0, -1):
        outputs[i - 1] = partials[i - 1] * inv if values[i - 1] else 0
        if values[i - 1] != 0:
            inv = inv * values[i - 1]
    return outputs


def _host_multi_interp_4(field, xsets, ysets):
    """poly_utils.py:412-440 on the host: eq_k = prod_{j != k} (X - x_j) by its coefficients, e_k = eq_k(x_k), one _host_multi_inv
    over every e_k, coefficients sum_k eq_k y_k / e_k."""
    polys_over = polynomials_over(field)
    data, targets = [], []
    for xs, ys in zip(xsets, ysets):
        xs = [field(v) if isinstance(v, int) else v for v in xs]
        ys = [field(v) if isinstance(v, int) else v for v in ys]
        eqs = []
        for k in range(4):
            a, b, c = [xs[j] for j in range(4) if j != k]
            eqs.append([-(a * b * c), a * b + a * c + b * c, -(a + b + c), field(1)])
        for k in range(4):
            e = field(0)
            for coef in reversed(eqs[k]):
                e = e * xs[k] + coef
            targets.append(e)
        data.append((ys, eqs))
    invs = _host_multi_inv(field, targets)
    out = []
    for r, (ys, eqs) in enumerate(data):
        w = [ys[k] * invs[4 * r + k] for k in range(4)]
        out.append(polys_over([eqs[0][i] * w[0] + eqs[1][i] * w[1] + eqs[2][i] * w[2] + eqs[3][i] * w[3] for i in range(4)]))
    return out


def _host_zpoly(field, roots):
    """poly_utils.py:322-335 on the field's own elements"""
    root = [field(1)]
    for x in roots:
        root.insert(0, field(0))
        for j in range(len(root) - 1):
            root[j] -= root[j + 1] * x
    return root


def _host_lagrange_interp(field, xs, ys):
    """poly_utils.py:337-369 on the host: the reference's numerators by long division of zpoly, denominators through its multi_inv"""
    polys_over = polynomials_over(field)
    root = polys_over(_host_zpoly(field, xs))
    nums = [root / polys_over([-x, 1]) for x in xs]
    denoms = [nums[i](xs[i]) for i in range(len(xs))]
    invdenoms = _host_multi_inv(field, denoms)
    b = [0 for _ in ys]
    for i in range(len(xs)):
        yslice = ys[i] * invdenoms[i]
        num_coefficients = nums[i].coefficients
        for j in range(len(ys)):
            if num_coefficients[j] and ys[i]:
                b[j] += num_coefficients[j] * yslice
    return polys_over(b)
