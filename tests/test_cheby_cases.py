"""What must hold of the operands of test_gpu_cheby.py before a GPU result is looked at (cheby_cases.py), without a device: the
restatement is the header's arithmetic and its polynomial is the Chebyshev polynomial of the interval; eight restated PCG
iterations on the 10 x 10 Poisson grid do with degree 3 what the issue promises of them; the integer operands keep every stored
value a float and both sums exact in any order; and on the general operands a lost element or a group taken from the wrong chunk
would exceed the dots' bound tenfold."""
import math

import numpy as np
import pytest
from numpy.polynomial import chebyshev

import cheby_cases as cb
import dots_cases as dc
import krylov_cases as kc


def test_the_sizes_are_the_issues_and_reach_the_reductions_second_stage():
    assert cb.SIZES == [1, 2, 3, 1023, 1024, 1026, 2049, 65537, 2097153] and cb.CHUNK == 1024
    assert max(cb.SIZES) == kc.DOTS_CHUNK * cb.CHUNK + 1 and max(cb.SIZES) * 8 < 2 ** 32
    assert sorted({(deg == 1, j == 0, j == deg - 1, dots) for _, deg, j, dots in cb.MODES}) == sorted(
        [(False, True, False, False), (False, False, False, False), (False, False, True, False), (False, False, True, True),
         (True, True, True, False), (True, True, True, True)])


def test_the_restatement_is_the_headers_arithmetic():
    # the bound: stored order (1e16 + 1 + 1 against 1 + 1 + 1e16), magnitudes, |m|, an empty row, a NaN, no rows
    p, v = np.array([0, 3, 3, 6]), np.array([-1e16, 1.0, -1.0, 1.0, 1.0, 1e16])
    assert cb.bound(3, p, v) == 1e16 + 2.0 and cb.bound(1, p, v) == 1e16
    assert cb.bound(3, p, v, np.array([-0.5, 7.0, 0.25])) == 0.5 * 1e16
    assert cb.bound(3, p, v, np.array([0.5, 7.0, 0.25], dtype=np.float32)) == 0.5 * 1e16
    assert cb.bound(0, np.array([0]), np.zeros(0)) == 0.0 and not np.signbit(cb.bound(0, np.array([0]), np.zeros(0)))
    assert np.isnan(cb.bound(3, p, np.array([1.0, np.nan, 1.0, 1.0, 1.0, 1.0]))) and cb.bound(3, p, np.array([1.0, -np.inf, 1.0, 1.0, 1.0, 1.0])) == np.inf
    assert np.isnan(cb.bound(3, p, np.array([1.0, np.inf, 1.0, 1.0, 1.0, 1.0]), np.array([0.0, 1.0, 1.0])))  # 0 inf
    # the coefficients by hand: lambda 2, scale 1, ratio 4: lmax 2, lmin 0.5, theta 1.25, delta 0.75
    t = cb.coeffs(3, 2.0, 1.0, 4.0)
    sigma = 1.25 / 0.75
    r0 = 1.0 / sigma
    r1 = 1.0 / (2.0 * sigma - r0)
    r2 = 1.0 / (2.0 * sigma - r1)
    assert t.tolist() == [0.0, 1.0 / 1.25, r1 * r0, (2.0 * r1) / 0.75, r2 * r1, (2.0 * r2) / 0.75]
    assert np.array_equal(cb.coeffs(16, 0.7, 1.1, 30.0)[:10], cb.coeffs(5, 0.7, 1.1, 30.0))  # a prefix is the table of a lower degree
    zero, nan = cb.coeffs(2, 0.0, 1.0, 30.0), cb.coeffs(2, np.nan, 1.0, 30.0)
    assert zero[0] == 0.0 and np.isinf(zero[1]) and np.all(np.isnan(zero[2:])) and nan[0] == 0.0 and np.all(np.isnan(nan[1:]))
    # the step: every product rounded, fl(m u) first, the sum of two rounded products, one cast last
    u, m, d, z = np.array([0.3]), np.array([0.7]), np.array([0.9]), np.array([0.1])
    coef = np.array([0.0, 0.6, 0.2, 1.7])
    d0, z0 = cb.step(coef, 2, 0, u, m, None, None, np.float64)
    assert d0[0] == np.float64(0.6) * (np.float64(0.7) * 0.3) == z0[0]
    d1, z1 = cb.step(coef, 2, 1, u, m, d, z, np.float64)
    assert d1 is None and z1[0] == np.float64(0.1) + (np.float64(0.2) * 0.9 + np.float64(1.7) * (np.float64(0.7) * 0.3))
    assert cb.step(coef, 2, 1, u, None, d, z, np.float64)[1][0] == np.float64(0.1) + (np.float64(0.2) * 0.9 + np.float64(1.7) * 0.3)
    assert cb.step(coef, 1, 0, u, m, None, None, np.float64)[0] is None
    # a float z takes the fp64 d, not the float d: d = 2^-24 + 2^-50 rounds to 2^-24 as a float, and 1 + 2^-24 would round to 1
    f = np.float32
    dm, zm = cb.step(np.array([0.0, 1.0, 1.0, 1.0]), 3, 1, np.array([2.0 ** -50], dtype=f), None, np.array([2.0 ** -24], dtype=f), np.array([1.0], dtype=f), f)
    assert dm[0] == f(2.0 ** -24) and zm[0] == f(1.0 + 2.0 ** -23) and dm.dtype == zm.dtype == f
    t0, t1 = cb.products(np.array([0.1]), np.array([0.7]))
    assert t0[0] == np.float64(0.1) * 0.7 and t1[0] == np.float64(0.1) * 0.1


@pytest.mark.parametrize("degree", [1, 2, 3, 5, 8, 16])
def test_the_residual_polynomial_is_the_chebyshev_polynomial_of_the_interval(degree):
    """On diag(lambda), 50 eigenvalues in [0.05, 2]: 1 - lambda p(lambda) = T_k((theta - lambda) / delta) / T_k(theta / delta)
    within 1e-13 (measured in numpy: 2.2e-15 at the most)."""
    lam = np.linspace(0.05, 2.0, 50)
    coef = cb.coeffs(degree, 2.0, 1.0, 40.0)
    z = cb.polynomial(lambda y: lam * y, coef, degree, np.ones(50), None, np.float64)
    theta, delta = (2.0 + 0.05) / 2.0, (2.0 - 0.05) / 2.0
    tk = [0.0] * degree + [1.0]
    want = chebyshev.chebval((theta - lam) / delta, tk) / chebyshev.chebval(theta / delta, tk)
    err = float(np.max(np.abs((1.0 - lam * z) - want)))
    print("degree %d: max |1 - lambda p(lambda) - T_k / T_k| %.3e" % (degree, err))
    assert err <= 1e-13
    assert np.max(np.abs(want)) < 1.0  # it damps the whole interval


def test_eight_restated_pcg_iterations_at_degree_3_beat_the_diagonal_a_thousandfold():
    rows, p, c, v, rhs, minv = cb.small_poisson()
    assert rows == 100 and cb.bound(rows, p, v, minv) == 2.0  # the Gershgorin bound of D^-1 A
    for dtype in cb.DTYPES:
        diag = cb.pcg_restated(rows, p, c, v, rhs, minv, dtype, 0)
        poly = cb.pcg_restated(rows, p, c, v, rhs, minv, dtype, cb.DEGREE)
        print("%s: r'r with the diagonal %s" % (np.dtype(dtype).name, ["%.3e" % x for x in diag]))
        print("%s: r'r with degree 3, ratio 30 %s" % (np.dtype(dtype).name, ["%.3e" % x for x in poly]))
        assert len(poly) == cb.ITERATIONS + 1 and np.all(np.isfinite(poly)) and diag[0] == poly[0] > 0
        assert poly[-1] < 1e-3 * diag[-1]


@pytest.mark.parametrize("n", cb.SIZES)
def test_integer_operands_are_exact_in_any_order(n):
    h = cb.int_case(n)
    assert all(float(x) == int(x) and math.log2(x) == int(math.log2(x)) for x in cb.INT_TABLE[1:])  # small powers of two
    for name, degree, j, dots in cb.MODES:
        for with_minv in (False, True):
            d, z, d0, d1 = h.results(degree, j, with_minv)  # (asserts the preconditions)
            assert float(d0) == d0 and float(d1) == d1 and d1 > 0
            if n > cb.GENERAL_LIMIT and not (dots and with_minv):
                continue  # the restatement at two million elements: the modes with dots and minv are enough
            for dtype in cb.DTYPES:
                u, m, dd, zz, r = h.arrays(dtype)
                ds, zs = cb.step(cb.INT_TABLE, degree, j, u, m if with_minv else None, dd, zz, dtype)
                assert (ds is None) == (d is None) and np.array_equal(zs.astype(np.float64), z)
                assert ds is None or np.array_equal(ds.astype(np.float64), d)
                t0, t1 = cb.products(zs, r)
                assert math.fsum(t0) == d0 and math.fsum(t1) == d1 and float(np.sum(t0[::-1])) == d0


@pytest.mark.parametrize("dtype", cb.DTYPES, ids=["float64", "float32"])
def test_a_lost_element_or_a_group_from_the_wrong_chunk_would_show(dtype):
    coef = cb.general_table()
    for n in [s for s in cb.SIZES if 3 < s <= cb.GENERAL_LIMIT]:
        u, m, d, z, r = cb.general_case(n).arrays(dtype)
        for name, degree, j, dots in cb.MODES:
            if not dots:
                continue
            for minv in (None, m):
                zs = cb.step(coef, degree, j, u, minv, d, z, dtype)[1]
                shares = [float(np.mean(np.abs(t) <= 10.0 * dc.bound(t))) for t in cb.products(zs, r)]
                assert all(s <= 0.01 for s in shares), (n, name, shares)  # a lost or doubled element shows in all the others
                if n >= 2 * cb.CHUNK:
                    bad = cb.step(coef, degree, j, cb.group_from_the_wrong_chunk(u), minv, d, z, dtype)[1]
                    assert np.array_equal(bad[:cb.CHUNK], zs[:cb.CHUNK]) and not np.array_equal(bad, zs)
                    for t, tb in zip(cb.products(zs, r), cb.products(bad, r)):
                        assert abs(math.fsum(tb) - math.fsum(t)) > 10.0 * dc.bound(t), (n, name)


def test_the_matrices_of_the_bound_have_what_the_bound_must_cope_with():
    rows, p, c, v = cb.ragged_matrix()
    lens = np.diff(p)
    assert p[0] == 0 and lens[0] == 0 and lens[-1] == 0 and np.any(lens > 64) and np.any(np.diff(c[p[1]:p[2]]) < 0)
    assert any(len(np.unique(c[p[i]:p[i + 1]])) < lens[i] for i in range(rows)), "no repeated column"
    backwards = np.zeros(rows)
    np.add.at(backwards, np.repeat(np.arange(rows), lens)[::-1], np.abs(v)[::-1])
    forwards = np.zeros(rows)
    np.add.at(forwards, np.repeat(np.arange(rows), lens), np.abs(v))
    assert cb.bound(rows, p, v) == forwards.max() and np.any(forwards != backwards), "the order of a row's sum does not show"
    rows, p, c, v = cb.last_row_matrix()
    s = np.add.reduceat(np.abs(v), p[:-1].astype(np.int64))
    assert rows == 3000 and int(np.argmax(s)) == rows - 1 and rows % 256 != 0
    for dtype in cb.DTYPES:
        m = cb.bound_minv(rows, dtype)
        assert m.dtype == dtype and np.any(m < 0) and cb.bound(rows, p, v, m) > 0
