"""The reference's OWN unit tests of multi_inv and multi_interp_4 (starks/test/test_poly_utils.py:74-105, 158-169), restated against
`starks_amd.poly_utils` in the style of test_reference_suite.py: same names, same inputs, stronger assertions -- every inverse the
reference's test touches is checked against pow(x, p - 2, p), not only the first four, and zeros against what the reference returns."""
import pytest

pytestmark = pytest.mark.gpu

P = 2**256 - 2**32 * 351 + 1


@pytest.fixture(scope="module")
def F():
    from starks_amd import _lib, IntegersModP
    _lib.ctx()  # fails loudly when the extension or the GPU is missing
    return IntegersModP(P)


def test_poly_utils__test_multi_inv(F):
    """test_poly_utils.py:74-105"""
    from starks_amd import IntegersModP
    from starks_amd.poly_utils import multi_inv
    from starks_amd.utils import get_power_cycle
    mod7 = IntegersModP(7)
    assert multi_inv(mod7, [mod7(6), mod7(6), mod7(6)]) == [6, 6, 6]   # 6^-1 = 6
    assert multi_inv(mod7, [mod7(6), mod7(1), mod7(6)]) == [6, 1, 6]   # 1^-1 = 1
    # the reference's test computes this one without asserting: a zero field element comes back as 1, zero ints as 0
    assert multi_inv(mod7, [mod7(0), mod7(1), mod7(1)]) == [1, 1, 1]
    assert multi_inv(mod7, [0, 1, 1]) == [0, 1, 1]

    G2 = F(7) ** ((P - 1) // 4096)
    xs = get_power_cycle(G2, F)
    xs_minus_1 = [x - 1 for x in xs]
    xs_minus_1_inv = multi_inv(F, xs_minus_1)
    for i in range(1, 5):  # the reference's own assertions
        assert xs_minus_1[i] * xs_minus_1_inv[i] == 1
    assert len(xs_minus_1_inv) == 4096
    assert [int(v) for v in xs_minus_1_inv[1:]] == [pow(int(v), P - 2, P) for v in xs_minus_1[1:]]
    assert int(xs_minus_1_inv[0]) == 1  # xs_minus_1[0] == 0: the reference skips it; its multi_inv returns 1 there

    steps, precision = 512, 4096
    z_evals = [xs[(i * steps) % precision] - 1 for i in range(precision)]
    z_inv = multi_inv(F, z_evals)
    for i in range(1, 5):
        assert z_evals[i] * z_inv[i] == 1
    assert [int(v) for v in z_inv] == [pow(int(v), P - 2, P) if int(v) else 1 for v in z_evals]


def test_poly_utils__test_multi_interp_4(F):
    """test_poly_utils.py:158-169, and the same identity data in the MiMC field on the GPU"""
    from starks_amd import IntegersModP
    from starks_amd.polynomial import polynomials_over
    from starks_amd.poly_utils import multi_interp_4
    mod7 = IntegersModP(7)
    polysOverMod = polynomials_over(mod7).factory
    xs = [mod7(1), mod7(2), mod7(3), mod7(6)]
    ys = [mod7(1), mod7(2), mod7(3), mod7(6)]
    interp = multi_interp_4(mod7, [xs, xs], [ys, ys])
    assert len(interp) == 2
    assert interp[0] == polysOverMod([0, 1])
    assert interp[1] == polysOverMod([0, 1])

    polysOver = polynomials_over(F).factory
    xs = [F(1), F(2), F(3), F(P - 1)]
    interp = multi_interp_4(F, [xs, xs], [xs, [x * x for x in xs]])
    assert len(interp) == 2
    assert interp[0] == polysOver([0, 1])
    assert interp[1] == polysOver([0, 0, 1])
    assert [int(c) for c in interp[1].coefficients] == [0, 0, 1]
