"""Dense univariate polynomials over a ring (starks/polynomial.py): what `NonBinaryFFT.fft` takes and `.inv_fft` returns
(starks/fft.py:263-272), with the reference's arithmetic -- `+ - * divmod / % **`, ints and ring elements cast to polynomials as
its `typecheck` does (numbertype.py:31-54).

Over the MiMC field every product and division runs on the GPU at every size (sh_poly_mul, sh_poly_divmod: NTT products and a
Newton inverse, O(n log n)); the result is backed by the device's bytes (a WireList, trailing zeros stripped on the bytes).  Calling
such a device-backed polynomial at an int or field element runs sh_poly_eval from EVAL_DEVICE_MIN_COEFS coefficients on, when the
process already holds a device context; every other call is the reference's loop.  Over another PRIME field __call__ goes to
sh_mod_poly_eval from MOD_EVAL_DEVICE_MIN_COEFS coefficients on (a list of elements is converted), and products and
divisions go to the device's generic entries (sh_mod_poly_mul, sh_mod_poly_divmod; mod_mul_wire and mod_divmod_wire always do) when
the process already holds a context, the field's 2-adicity admits the call's transforms and the operands reach the measured threshold
(MOD_DEVICE_MIN).  Any other ring or size (the reference's own tests use Z/5, Z/7, Z/11 and Fraction) runs the reference's schoolbook
algorithms on the host.
Errors are the reference's: `/` and `%` by the zero polynomial raise ZeroDivisionError, `divmod` by it raises IndexError (the
reference reads the divisor's leading coefficient, polynomial.py:131)."""
import ctypes
from itertools import zip_longest

from .wireseq import WireList

_POLYS = {}


class Poly(object):
    pass


def polynomials_over(ring):
    if ring in _POLYS:
        return _POLYS[ring]

    class Polynomial(Poly):
        def __init__(self, c):
            if isinstance(c, WireList) and c.field is ring:
                # a transform's output (wireseq.py): trailing zeros are stripped on the bytes, no element is created
                k = (len(c.wire_bytes().rstrip(b"\0")) + 31) // 32
                self.coefficients = c[:k]
                return
            if isinstance(c, Polynomial):
                coeffs = list(c.coefficients)
            elif isinstance(c, bytes):
                if len(c) % 32:
                    raise ValueError("Bytelength must be multiple of 32")
                coeffs = [ring(c[i:i + 32]) for i in range(0, len(c), 32)]
            elif hasattr(c, "__iter__"):
                coeffs = [x if isinstance(x, ring) else ring(x) for x in c]
            else:
                coeffs = [c if isinstance(c, ring) else ring(c)]
            k = len(coeffs)
            while k and coeffs[k - 1] == 0:  # strip trailing zeros (polynomial.py:13-21,58)
                k -= 1
            self.coefficients = coeffs[:k]

        @classmethod
        def factory(cls, L):
            return cls(L)

        def is_zero(self):
            return not self.coefficients

        def degree(self):
            return len(self.coefficients) - 1

        def __len__(self):
            return len(self.coefficients)

        def __iter__(self):
            return iter(self.coefficients)

        def __eq__(self, other):
            if not isinstance(other, Polynomial):
                try:
                    other = Polynomial(other)
                except Exception:
                    return False
            return self.coefficients == other.coefficients

        def __ne__(self, other):
            return not self == other

        def __call__(self, x):  # polynomial.py:158-164
            if _eval_on_device(ring, self.coefficients, x):
                return WireList(eval_wire(_lib_mod().to_wire(self.coefficients), _lib_mod().to_wire([x])), ring)[0]
            if _mod_eval_on_device(ring, self.coefficients, x):
                p, to_wire = int(ring.p), _lib_mod().to_wire
                return WireList(mod_eval_wire(p, to_wire(self.coefficients, p), to_wire([x], p)), ring)[0]
            y = ring(0)
            pw = ring(1)
            for a in self.coefficients:
                y = y + pw * a
                pw = pw * x
            return y

        def __repr__(self):
            return "0" if self.is_zero() else " + ".join(
                ("%s *x**%d" % (a, i)) if i else "%s" % a for i, a in enumerate(self.coefficients))

        def leading_coefficient(self):
            return self.coefficients[-1]

        # ---- arithmetic (polynomial.py:84-150, numbertype.py:68-84) --------------------------------------------------------
        def __neg__(self):
            return Polynomial([-a for a in self.coefficients])

        def __add__(self, other):
            other = _cast(other)
            zero = ring(0)
            return Polynomial([x + y for x, y in zip_longest(self.coefficients, other.coefficients, fillvalue=zero)])

        __radd__ = __add__

        def __sub__(self, other):
            return self + (-_cast(other))

        def __rsub__(self, other):
            return _cast(other) + (-self)

        def __mul__(self, other):
            other = _cast(other)
            if self.is_zero() or other.is_zero():
                return Polynomial([])
            if _on_device(ring):
                return Polynomial(WireList(mul_wire(_wire(self), _wire(other)), ring))
            if _mod_on_device(ring, "mul", 0, len(self), len(other)):
                return Polynomial(WireList(mod_mul_wire(ring.p, _wire(self, ring.p), _wire(other, ring.p)), ring))
            return self._schoolbook(other)

        def _schoolbook(self, other):
            """the reference's product loop (polynomial.py:116-125), never routed: the host long division below multiplies by
            monomials with it"""
            out = [ring(0) for _ in range(len(self) + len(other) - 1)]
            for i, a in enumerate(self.coefficients):
                for j, b in enumerate(other.coefficients):
                    out[i + j] += a * b
            return Polynomial(out)

        __rmul__ = __mul__

        def __divmod__(self, divisor):
            divisor = _cast(divisor)
            lc = divisor.leading_coefficient()  # IndexError for the zero polynomial, as in the reference
            if _on_device(ring):
                q, r = divmod_wire(_wire(self), _wire(divisor))
                return Polynomial(WireList(q, ring)), Polynomial(WireList(r, ring))
            if _mod_on_device(ring, "divmod", 1, len(self), len(divisor)):
                q, r = mod_divmod_wire(ring.p, _wire(self, ring.p), _wire(divisor, ring.p))
                return Polynomial(WireList(q, ring)), Polynomial(WireList(r, ring))
            quotient, remainder = Polynomial([]), self
            deg = divisor.degree()
            while remainder.degree() >= deg:
                mono = Polynomial([ring(0)] * (remainder.degree() - deg) + [remainder.leading_coefficient() / lc])
                quotient = quotient + mono
                remainder = remainder - mono._schoolbook(divisor)
            return quotient, remainder

        def __rdivmod__(self, other):
            return divmod(_cast(other), self)

        def __truediv__(self, divisor):
            divisor = _cast(divisor)
            if divisor.is_zero():
                raise ZeroDivisionError
            return divmod(self, divisor)[0]

        def __rtruediv__(self, other):
            return _cast(other) / self

        def __mod__(self, divisor):
            divisor = _cast(divisor)
            if divisor.is_zero():
                raise ZeroDivisionError
            return divmod(self, divisor)[1]

        def __rmod__(self, other):
            return _cast(other) % self

        def __pow__(self, n):  # square-and-multiply (numbertype.py:68-84)
            if type(n) is not int:
                raise TypeError
            Q = self
            R = self if n & 1 else Polynomial(1)
            i = 2
            while i <= n:
                Q = Q * Q
                if n & i == i:
                    R = Q * R
                i = i << 1
            return R

    def _cast(other):
        """numbertype.typecheck: anything else is cast to a polynomial, and a failed cast is a TypeError"""
        if isinstance(other, Polynomial):
            return other
        try:
            return Polynomial(other)
        except Exception as e:
            raise TypeError("Not able to typecast %r of type %s to type %s: %s" % (other, type(other).__name__,
                                                                                      Polynomial.__name__, e))

    Polynomial.ring = ring
    Polynomial.operatorPrecedence = 2
    Polynomial.__name__ = "(%s)[x]" % ring.__name__
    _POLYS[ring] = Polynomial
    return Polynomial


# Polynomial.__call__ runs on the device from this many coefficients on: end to end on an MI355X, 0.06 ms against the host loop's
# 0.10 ms at 2^6 coefficients, 0.08 against 0.05 ms at 2^4 (tools/poly_eval_time.py, profiles/r10_poly_eval.json)
EVAL_DEVICE_MIN_COEFS = 64
_EVAL_MAX_COEFS = 1 << 25


def _lib_mod():
    from . import _lib
    return _lib


def _eval_on_device(ring, coefficients, x):
    """__call__ goes to the device only for the MiMC field, an int or element x, coefficients a device call returned (a WireList),
    at least EVAL_DEVICE_MIN_COEFS of them, and a device context this process already holds; anything else (composition with a
    Polynomial x included) keeps the host loop"""
    if not isinstance(coefficients, WireList) or not EVAL_DEVICE_MIN_COEFS <= len(coefficients) <= _EVAL_MAX_COEFS:
        return False
    if not (isinstance(x, ring) or (isinstance(x, int) and not isinstance(x, bool))) or not _on_device(ring):
        return False
    return getattr(_lib_mod(), "_ctx", None) is not None


def _on_device(ring):
    from ._lib import MIMC_P
    return int(getattr(ring, "p", 0)) == MIMC_P


# Another prime field: __call__ at an int or element goes to the device (sh_mod_poly_eval) from this many coefficients on, under
# _lib.mod_poly_routable with no transform requirement (the direct path runs none, so the field's 2-adicity does not matter).  Unlike
# the MiMC rule the coefficients need not be a WireList: converting a list of n elements to wire form costs 0.4 us per element
# against the host loop's 2.2 us per coefficient (two ring operations), measured on the host at n = 2^16 over BN254, so the conversion
# never decides.  The threshold is the smallest power of two from which the device call won end to end at every larger measured size
# (tools/mod_poly_eval_time.py over BN254 against the loop of __call__ on the same inputs in the same run,
# profiles/r22_mod_poly_eval.json, "routing": 0.082 ms against 0.139 ms at 128 coefficients, 0.077 against 0.066 ms at 64; at 2^20
# coefficients 1.44 ms against 1.48 s).
MOD_EVAL_DEVICE_MIN_COEFS = 128


def _mod_eval_on_device(ring, coefficients, x):
    p = getattr(ring, "p", None)
    if p is None or not MOD_EVAL_DEVICE_MIN_COEFS <= len(coefficients) <= _EVAL_MAX_COEFS:
        return False
    if not (isinstance(x, ring) or (isinstance(x, int) and not isinstance(x, bool))):
        return False
    return _lib_mod().mod_poly_routable(p, None, len(coefficients))


# Another prime field: products and divisions go to the device (sh_mod_poly_mul, sh_mod_poly_divmod) when _lib.mod_poly_routable holds
# and the SHORTER side of the work -- min(n_a, n_b) of a product, min(n_a - n_b + 1, n_b) (quotient and divisor lengths) of a division --
# has at least this many coefficients; None: routing is off for the operation.  The host loops cost n_a n_b and (n_a - n_b + 1) n_b
# ring products, so the shorter side bounds them from below by the measured square shapes.  Each value is the smallest power of two
# from which the device call won end to end at every larger measured size (tools/mod_poly_time.py over BN254 against the host loops
# above on the same inputs in the same run, profiles/r21_mod_poly.json, "routing": n x n products 0.22 ms against 0.67 ms at 32 and
# 0.24 against 0.19 ms at 16; 2n-by-n divisions 1.7 ms against 2.6 ms at n = 16 and 1.5 against 0.9 ms at 8).
MOD_DEVICE_MIN = {"mul": 32, "divmod": 16}


def _mod_on_device(ring, what, op, n_a, n_b):
    least = MOD_DEVICE_MIN[what]
    p = getattr(ring, "p", None)
    if least is None or p is None or min(n_a - n_b + 1 if what == "divmod" else n_a, n_b) < least:
        return False
    return _lib_mod().mod_poly_routable(p, op, n_a, n_b)


def _wire(poly, modulus=None):
    from . import _lib
    return _lib.to_wire(poly.coefficients) if modulus is None else _lib.to_wire(poly.coefficients, int(modulus))


def mod_mul_wire(modulus, a, b, root=None):
    """mul_wire over any prime modulus below 2^256 (sh_mod_poly_mul); root = (root of unity, log2 of its order), default
    _lib.two_adic_root(modulus).  Always on the device."""
    from . import _lib
    a, b = _as_bytes(a), _as_bytes(b)
    na, nb = len(a) // 32, len(b) // 32
    if na == 0 or nb == 0:
        return b""
    m, w, k = _lib.mod_poly_args(modulus, root)
    out = ctypes.create_string_buffer(32 * (na + nb - 1))
    _lib.check(_lib.lib().sh_mod_poly_mul(_lib.ctx(), m, w, k, a, na, b, nb, out), "sh_mod_poly_mul")
    return out.raw


def mod_divmod_wire(modulus, a, b, root=None):
    """divmod_wire over any prime modulus below 2^256 (sh_mod_poly_divmod).  Always on the device."""
    from . import _lib
    a, b = _as_bytes(a), _as_bytes(b)
    na, nb = len(a) // 32, len(b) // 32
    if nb == 0:
        raise ZeroDivisionError
    nq, nr = max(na - nb + 1, 0), min(na, nb - 1)
    m, w, k = _lib.mod_poly_args(modulus, root)
    q = ctypes.create_string_buffer(32 * max(nq, 1))
    r = ctypes.create_string_buffer(32 * max(nr, 1))
    _lib.check(_lib.lib().sh_mod_poly_divmod(_lib.ctx(), m, w, k, a, na, b, nb, q, r), "sh_mod_poly_divmod")
    return q.raw[:32 * nq], r.raw[:32 * nr]


def mod64_mul_words(modulus, a, b, root=None):
    """The exact product over any prime modulus below 2^64 on packed 64-bit words (sh_mod64_poly_mul): a, b = native 8-byte words (a
    list of ints, bytes or any buffer of words; any 64-bit values) -> len(a) + len(b) - 1 canonical coefficients, a memoryview of
    format 'Q' over a fresh bytearray (empty when either operand is).  root = (root of unity, log2 of its order), default
    _lib.two_adic_root(modulus).  An entry of its own: Polynomial.__mul__ keeps the 32-byte path.  Always on the device."""
    from . import _lib
    from .fft import _word_result, _words
    sa, _ka, na = _words(a)
    sb, _kb, nb = _words(b)
    if na == 0 or nb == 0:
        return memoryview(bytearray()).cast("Q")
    m, w, k = _lib.mod64_poly_args(modulus, root)
    out, dst = _word_result(na + nb - 1)
    _lib.check(_lib.lib().sh_mod64_poly_mul(_lib.ctx(), m, w, k, sa, na, sb, nb, dst), "sh_mod64_poly_mul")
    del dst
    return memoryview(out).cast("Q")


def mod64_divmod_words(modulus, a, b, root=None):
    """(quotient, remainder) over any prime modulus below 2^64 on packed 64-bit words (sh_mod64_poly_divmod), operands and results as
    in `mod64_mul_words`: len(a) - len(b) + 1 and len(b) - 1 words, or no quotient and a itself for len(a) < len(b).  Always on the
    device."""
    from . import _lib
    from .fft import _word_result, _words
    sa, _ka, na = _words(a)
    sb, _kb, nb = _words(b)
    if nb == 0:
        raise ZeroDivisionError
    nq, nr = max(na - nb + 1, 0), min(na, nb - 1)
    m, w, k = _lib.mod64_poly_args(modulus, root)
    q, dq = _word_result(max(nq, 1))
    r, dr = _word_result(max(nr, 1))
    _lib.check(_lib.lib().sh_mod64_poly_divmod(_lib.ctx(), m, w, k, sa if na else None, na, sb, nb, dq, dr), "sh_mod64_poly_divmod")
    del dq, dr
    return memoryview(q).cast("Q")[:nq], memoryview(r).cast("Q")[:nr]


def mod64_eval_words(modulus, coefs, xs, batch=1, root=None):
    """The values of `batch` polynomials of n coefficients each ([batch][n], ascending) at the m points xs over any prime modulus
    below 2^64 on packed 64-bit words (sh_mod64_poly_eval), operands as in `mod64_mul_words` -> [batch][m] canonical words, a
    memoryview of format 'Q' (empty for m = 0): out[b][i] = sum_k coefs[b][k] xs[i]^k.  n = 0 gives zeros.  root as there -- the
    direct path needs none, (1, 0) is valid.  An entry of its own: Polynomial.__call__ and multi_eval keep the 32-byte path.  Always
    on the device."""
    from . import _lib
    from .fft import _word_result, _words
    sc, _kc, nc = _words(coefs)
    sx, _kx, m = _words(xs)
    if batch < 1 or nc % batch:
        raise ValueError("coefs must hold batch polynomials of the same length")
    if m == 0:
        return memoryview(bytearray()).cast("Q")
    n = nc // batch
    p, w, k = _lib.mod64_poly_args(modulus, root)
    out, dst = _word_result(batch * m)
    _lib.check(_lib.lib().sh_mod64_poly_eval(_lib.ctx(), p, w, k, sc if n else None, n, batch, sx, m, dst), "sh_mod64_poly_eval")
    del dst
    return memoryview(out).cast("Q")


def _as_bytes(data):
    data = bytes(data) if not isinstance(data, bytes) else data
    if len(data) % 32:
        raise ValueError("wire form is a multiple of 32 bytes")
    return data


def mul_wire(a, b):
    """The exact product of two coefficient vectors in wire form (ascending, values may be >= p) -> len(a) + len(b) - 1 canonical
    coefficients, b"" when either is empty (sh_poly_mul).  Not trimmed."""
    from . import _lib
    a, b = _as_bytes(a), _as_bytes(b)
    na, nb = len(a) // 32, len(b) // 32
    if na == 0 or nb == 0:
        return b""
    out = ctypes.create_string_buffer(32 * (na + nb - 1))
    _lib.check(_lib.lib().sh_poly_mul(_lib.ctx(), a, na, b, nb, out), "sh_poly_mul")
    return out.raw


def eval_wire(coefs, xs, batch=1):
    """The values of `batch` polynomials of n coefficients each (wire form, ascending, [batch][n], values may be >= p) at the m
    points xs (wire form) -> [batch][m] canonical values in wire form (sh_poly_eval): out[b][i] = sum_k coefs[b][k] xs[i]^k.
    n = 0 gives zeros."""
    from . import _lib
    coefs, xs = _as_bytes(coefs), _as_bytes(xs)
    if batch < 1 or (len(coefs) // 32) % batch:
        raise ValueError("coefs must hold batch polynomials of the same length")
    n, m = len(coefs) // 32 // batch, len(xs) // 32
    if m == 0:
        return b""
    out = ctypes.create_string_buffer(32 * batch * m)
    _lib.check(_lib.lib().sh_poly_eval(_lib.ctx(), coefs if n else None, n, batch, xs, m, out), "sh_poly_eval")
    return out.raw


def mod_eval_wire(modulus, coefs, xs, batch=1, root=None):
    """eval_wire over any prime modulus below 2^256 (sh_mod_poly_eval): [batch][n] coefficients at m points -> [batch][m] canonical
    values, wire form in and out; root = (root of unity, log2 of its order), default _lib.two_adic_root(modulus) -- the direct path
    needs none, (1, 0) is valid.  Always on the device."""
    from . import _lib
    coefs, xs = _as_bytes(coefs), _as_bytes(xs)
    if batch < 1 or (len(coefs) // 32) % batch:
        raise ValueError("coefs must hold batch polynomials of the same length")
    n, m = len(coefs) // 32 // batch, len(xs) // 32
    if m == 0:
        return b""
    mod, w, k = _lib.mod_poly_args(modulus, root)
    out = ctypes.create_string_buffer(32 * batch * m)
    _lib.check(_lib.lib().sh_mod_poly_eval(_lib.ctx(), mod, w, k, coefs if n else None, n, batch, xs, m, out), "sh_mod_poly_eval")
    return out.raw


def divmod_wire(a, b):
    """(quotient, remainder) of a by b in wire form (sh_poly_divmod): max(len(a) - len(b) + 1, 0) and min(len(a), len(b) - 1)
    canonical coefficients, not trimmed.  b's last coefficient must be nonzero mod p (else StarkHipError)."""
    from . import _lib
    a, b = _as_bytes(a), _as_bytes(b)
    na, nb = len(a) // 32, len(b) // 32
    if nb == 0:
        raise ZeroDivisionError
    nq, nr = max(na - nb + 1, 0), min(na, nb - 1)
    q = ctypes.create_string_buffer(32 * max(nq, 1))
    r = ctypes.create_string_buffer(32 * max(nr, 1))
    _lib.check(_lib.lib().sh_poly_divmod(_lib.ctx(), a, na, b, nb, q, r), "sh_poly_divmod")
    return q.raw[:32 * nq], r.raw[:32 * nr]
