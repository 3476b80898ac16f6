"""The reference's OWN unit tests of univariate polynomials (starks/test/test_polynomial.py) and of zpoly / lagrange_interp
(starks/test/test_poly_utils.py:52-72, 107-122), restated against `starks_amd` under the same names.  The small rings (Z/5, Z/7, Z/11,
Fraction) run the reference's algorithms on the host; the same assertions in the MiMC field run on the GPU (marked gpu).  The F25 part
of test_lagrange_interp is out: there is no FiniteField here."""
from fractions import Fraction

import pytest

P = 2**256 - 2**32 * 351 + 1


def _rings():
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    return [polynomials_over(Fraction).factory, polynomials_over(IntegersModP(5)).factory, polynomials_over(IntegersModP(11)).factory]


@pytest.fixture(scope="module")
def mimc():
    from starks_amd import _lib, IntegersModP
    from starks_amd.polynomial import polynomials_over
    _lib.ctx()  # fails loudly when the extension or the GPU is missing
    return polynomials_over(IntegersModP(P)).factory


def check_equality(p):
    assert p([]) == p([])
    assert p([1, 2]) == p([1, 2])
    assert p([1, 2, 0]) == p([1, 2, 0, 0])


def check_addition(p):
    assert p([1, 2, 3]) == p([1, 0, 3]) + p([0, 2])
    assert p([1, 2, 3]) == p([1, 2, 3]) + p([])
    assert p([5, 2, 3]) == p([4]) + p([1, 2, 3])
    assert p([1, 2]) == p([1, 2, 3]) + p([0, 0, -3])


def check_subtraction(p):
    assert p([1, -2, 3]) == p([1, 0, 3]) - p([0, 2])
    assert p([1, 2, 3]) == p([1, 2, 3]) - p([])
    assert p([-1, -2, -3]) == p([]) - p([1, 2, 3])


def check_multiplication(p):
    assert p([1, 2, 1]) == p([1, 1]) * p([1, 1])
    assert p([2, 5, 5, 3]) == p([2, 3]) * p([1, 1, 1])
    assert p([0, 7, 49]) == p([0, 1, 7]) * p([7])


def check_division(p):
    assert p([1, 1, 1, 1, 1, 1]) == p([-1, 0, 0, 0, 0, 0, 1]) / p([-1, 1])
    assert p([-1, 1, -1, 1, -1, 1]) == p([1, 0, 0, 0, 0, 0, 1]) / p([1, 1])
    assert p([]) == p([]) / p([1, 1])
    assert p([1, 1]) == p([1, 1]) / p([1])
    assert p([1, 1]) == p([2, 2]) / p([2])


def check_modulus(p):
    assert p([]) == p([1, 7, 49]) % p([7])
    assert p([-7]) == p([-3, 10, -5, 3]) % p([1, 3])


def check_division_more(p, one_seventh):
    assert p([one_seventh, 1, 7]) == p([1, 7, 49]) / p([7])


CHECKS = [check_equality, check_addition, check_subtraction, check_multiplication, check_division, check_modulus]


def test_polynomial__test_equality():
    for p in _rings():
        check_equality(p)


def test_polynomial__test_addition():
    for p in _rings():
        check_addition(p)


def test_polynomial__test_subtraction():
    for p in _rings():
        check_subtraction(p)


def test_polynomial__test_multiplication():
    for p in _rings():
        check_multiplication(p)


def test_polynomial__test_division():
    for p in _rings():
        check_division(p)


def test_polynomial__test_modulus():
    for p in _rings():
        check_modulus(p)


def test_polynomial__test_division_more():
    """test_polynomial.py:104-115"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    Mod5, Mod11 = IntegersModP(5), IntegersModP(11)
    check_division_more(polynomials_over(Fraction).factory, Fraction(1, 7))
    check_division_more(polynomials_over(Mod5).factory, 1 / Mod5(7))
    check_division_more(polynomials_over(Mod11).factory, 1 / Mod11(7))


def test_polynomial__test_polynomial_call():
    """test_polynomial.py:117-129"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    mod5 = IntegersModP(5)
    polysMod5 = polynomials_over(mod5).factory
    poly = polysMod5([1, 1])
    z = mod5(3)
    assert z + 1 == poly(z)
    poly2 = polysMod5([1, 1, 1])
    assert 1 + z + z**2 == poly2(z)
    assert poly2(z) == mod5(3)


def test_polynomial__errors_and_casts():
    """the reference's typecheck casts ints and ring elements; / and % by zero raise ZeroDivisionError, divmod IndexError"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    m7 = IntegersModP(7)
    p = polynomials_over(m7).factory
    assert p([1, 1]) + 1 == p([2, 1]) and 1 + p([1, 1]) == p([2, 1]) and 3 - p([1, 1]) == p([2, 6])
    assert p([1, 1]) * m7(2) == p([2, 2]) and m7(2) * p([1, 1]) == p([2, 2])
    assert -p([1, 2]) == p([6, 5])
    assert p([1, 1]) ** 3 == p([1, 3, 3, 1]) and p([1, 1]) ** 0 == p([1])
    assert p([3, 0, 2]).leading_coefficient() == 2
    with pytest.raises(ZeroDivisionError):
        p([1, 2]) / p([])
    with pytest.raises(ZeroDivisionError):
        p([1, 2]) % 0
    with pytest.raises(IndexError):
        divmod(p([1, 2]), p([0]))
    with pytest.raises(TypeError):
        p([1]) + object()


def test_poly_utils__test_zpoly():
    """test_poly_utils.py:52-72"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    from starks_amd.poly_utils import zpoly
    mod7 = IntegersModP(7)
    polysMod7 = polynomials_over(mod7).factory
    poly = zpoly(mod7, [3])
    assert poly(mod7(3)) == 0
    assert poly == polysMod7([-3, 1])
    poly = zpoly(mod7, [1, 2])
    assert poly(mod7(1)) == 0
    assert poly(mod7(2)) == 0
    assert poly == polysMod7([2, -3, 1])


def test_poly_utils__test_lagrange_interp():
    """test_poly_utils.py:107-122 (the F25 part needs FiniteField: out of scope)"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    from starks_amd.poly_utils import lagrange_interp
    mod7 = IntegersModP(7)
    polysOverMod = polynomials_over(mod7).factory
    xs = [mod7(1), mod7(6)]
    assert lagrange_interp(mod7, xs, [mod7(1), mod7(6)]) == polysOverMod([0, 1])
    assert lagrange_interp(mod7, xs, [mod7(0), mod7(0)]) == polysOverMod([0])
    with pytest.raises(AssertionError):
        lagrange_interp(mod7, xs, [mod7(1)])


# ---- the same assertions in the MiMC field, on the GPU ---------------------------------------------------------------------------
MIMC_CHECKS = CHECKS + [check_division_more]


@pytest.mark.gpu
@pytest.mark.parametrize("check", MIMC_CHECKS, ids=[c.__name__ for c in MIMC_CHECKS])
def test_polynomial__mimc(mimc, check):
    if check is check_division_more:
        check(mimc, pow(7, P - 2, P))
    else:
        check(mimc)


@pytest.mark.gpu
def test_polynomial__mimc_results_are_device_bytes(mimc):
    from starks_amd.wireseq import WireList
    prod = mimc([1, 1]) * mimc([1, 1])
    assert isinstance(prod.coefficients, WireList) and [int(c) for c in prod] == [1, 2, 1]
    q, r = divmod(mimc([-3, 10, -5, 3]), mimc([1, 3]))
    assert isinstance(q.coefficients, WireList) and r == mimc([-7])
    with pytest.raises(ZeroDivisionError):
        mimc([1, 2]) / 0
    with pytest.raises(IndexError):
        divmod(mimc([1, 2]), mimc([]))
    assert mimc([1, 1]) ** 5 == mimc([1, 5, 10, 10, 5, 1])


@pytest.mark.gpu
def test_poly_utils__test_zpoly_mimc(mimc):
    from starks_amd import IntegersModP
    from starks_amd.poly_utils import zpoly
    F = IntegersModP(P)
    poly = zpoly(F, [3])
    assert poly(F(3)) == 0 and poly == mimc([-3, 1])
    poly = zpoly(F, [1, 2])
    assert poly(F(1)) == 0 and poly(F(2)) == 0 and poly == mimc([2, -3, 1])
    assert zpoly(F, []) == mimc([1])


@pytest.mark.gpu
def test_poly_utils__test_lagrange_interp_mimc(mimc):
    from starks_amd import IntegersModP
    from starks_amd.poly_utils import lagrange_interp
    F = IntegersModP(P)
    xs = [F(1), F(P - 1)]
    assert lagrange_interp(F, xs, [F(1), F(P - 1)]) == mimc([0, 1])
    assert lagrange_interp(F, xs, [F(0), F(0)]) == mimc([0])
    assert lagrange_interp(F, [], []) == mimc([])
    with pytest.raises(AssertionError):
        lagrange_interp(F, xs, [F(1)])
