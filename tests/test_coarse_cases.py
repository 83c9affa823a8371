"""The numpy restatement of include/spmv_hip_coarse.h (coarse_cases.py) without a device: it is the header's arithmetic, its
matrices hold what the set-up must cope with, the integer operands of the apply are exact in any order, and the restated inverse
is as good as numpy.linalg.inv's up to a constant."""
import numpy as np
import pytest

import coarse_cases as cc

# The largest ratio, over the well-posed cases, of max |A X - I| of the restated inverse to that of numpy.linalg.inv on the same
# matrix (an exact numpy residual counted as one rounding, 2^-53) is 6.20, on the 513 rows of a Poisson matrix (Poisson 19^2 5.20,
# the SPD matrix of condition 1e6 4.35, the 376-row level of the 512^2 grid 4.29, Poisson 15^2 3.25, the random matrices 0.44 to
# 2.44).  Gauss-Jordan and LAPACK's LU differ by rounding error, so a constant is expected, a blow-up is not: pinned
# at twice that, rounded up.
RESIDUAL_RATIO = 13.0


def test_the_sizes_are_the_issues_and_surround_every_tile():
    assert set((0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 129, 225, 257, 513)) <= set(cc.SIZES) and max(cc.SIZES) <= 513
    assert {n - cc.ld_of(n) for n in cc.SIZES} == {0, -1, -2, -3}, "the padding of 0 to 3 columns"
    assert {15, 16, 17} <= set(cc.SIZES), "the update's 16 rows a workgroup"
    assert {255, 256, 257} <= set(cc.SIZES), "the pivot kernel's 256 threads"
    assert [cc.ld_of(n) for n in (-1, 0, 1, 4, 5, 2047, 2048)] == [0, 0, 4, 4, 8, 2048, 2048]
    assert [cc.workspace_of(n) for n in (0, 1, 225, 2048)] == [16, 96, 822624, 67125248]


def test_the_restatement_is_the_headers_arithmetic():
    # densify: stored order, any column order, a position stored twice, one not stored, columns outside counted and not followed
    p, c = np.array([0, 5, 7]), np.array([1, 2, 0, 1, -1, 0, 7])
    v = np.array([1e16, 3.0, 2.0, 1.0, 9.0, 4.0, 5.0])
    B, skipped = cc.densify(2, p, c, v)
    assert skipped == 3 and B[0, 1] == np.float64(1e16) + 1.0 and B[0, 0] == 2.0 and B[1, 0] == 4.0 and B[1, 1] == 0.0
    v2 = np.array([1.0, 3.0, 2.0, 1e16, 9.0, 4.0, 5.0])  # the same position in the other order: 0 + 1 + 1e16
    assert cc.densify(2, p, c, v2)[0][0, 1] == 1e16 + 1.0
    # n == 1: fl(1 / a), padded to four columns of +0.0; a zero of either sign is singular at column 0
    inv, singular, column = cc.invert(np.array([[3.0]]), np.float64)
    assert inv.shape == (1, 4) and inv[0].tolist() == [1.0 / 3.0, 0.0, 0.0, 0.0] and not np.signbit(inv[0, 1:]).any() and (singular, column) == (0, -1)
    for zero in (0.0, -0.0):
        inv, singular, column = cc.invert(np.array([[zero]]), np.float32)
        assert inv.dtype == np.float32 and inv[0].tolist() == [1.0, 0.0, 0.0, 0.0] and (singular, column) == (1, 0)
    # 2 x 2 by hand: the pivot of column 0 is row 1 (|-4| > |1|)
    t = 1.0 / -4.0
    r0 = np.array([-4.0, 3.0, 0.0, 1.0]) * t
    r1 = np.array([1.0, 2.0, 1.0, 0.0]) - 1.0 * r0
    r1n = r1 * (1.0 / r1[1])
    r0n = r0 - r0[1] * r1n
    inv, singular, column = cc.invert(np.array([[1.0, 2.0], [-4.0, 3.0]]), np.float64)
    assert np.array_equal(inv[:, :2], np.array([r0n[2:], r1n[2:]])) and (singular, column) == (0, -1)
    assert np.array_equal(cc.invert(np.array([[0.0, 1.0], [1.0, 0.0]]), np.float64)[0][:, :2], np.array([[0.0, 1.0], [1.0, 0.0]]))
    # the first of equal magnitudes wins: with row 2 in front of row 0 at column 0 the bits differ
    n, p, c, v, _, _ = cc.case("tie")
    A = cc.densify(n, p, c, v)[0]
    assert abs(A[0, 0]) == abs(A[1, 0]) == abs(A[2, 0])
    m = np.concatenate([A, np.eye(3)], axis=1)
    for k in range(3):  # the elimination without any swap
        if k == 1:
            assert m[1, 1] == m[2, 1] != 0.0, "a second tie, at column 1"
        ec, f = m[k] * (1.0 / m[k, k]), m[:, k].copy()
        m = m - f[:, None] * ec[None, :]
        m[k] = ec
    assert np.array_equal(cc.invert(A, np.float64)[0][:, :3], m[:, 3:])
    # a NaN never wins the search, and a NaN in row c keeps row c
    inv, singular, _ = cc.invert(np.array([[1.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [-1.0, 0.0, 1.0]]), np.float64)
    assert singular == 0 and np.all(np.isnan(inv[:, :3]))  # row 1 is never swapped up: column 0 eliminates with its NaN
    assert cc.invert(np.array([[np.nan, 1.0], [5.0, 1.0]]), np.float64)[1] == 0 and cc.invert(np.array([[np.nan]]), np.float64)[1] == 0
    # singular at the second column: the identity, recorded; the columns behind do nothing
    inv, singular, column = cc.invert(np.array([[1.0, 2.0, 0.0], [2.0, 4.0, 0.0], [0.0, 0.0, 0.0]]), np.float64)
    assert np.array_equal(inv[:, :3], np.eye(3)) and (singular, column) == (1, 1)
    # the apply: lane l takes l, l + 64, ...; every product rounded; the butterfly; one cast last
    rng = np.random.default_rng(1)
    n = 130
    inv, r = rng.uniform(-1.0, 1.0, size=(n, cc.ld_of(n))), rng.uniform(-1.0, 1.0, size=n)
    lanes = [0.0] * 64
    for j in range(n):
        lanes[j % 64] = lanes[j % 64] + np.float64(inv[5, j]) * np.float64(r[j])
    step = 1
    while step < 64:
        lanes = [lanes[l] + lanes[l ^ step] for l in range(64)]
        step *= 2
    assert cc.apply(inv, n, r, np.float64)[5] == lanes[0] and cc.apply(inv, n, r, np.float32)[5] == np.float32(lanes[0])
    assert not np.signbit(cc.apply(np.array([[1.0, 0.0, 0.0, 0.0]]), 1, np.array([-0.0]), np.float64)[0])  # +0.0 + -0.0
    assert cc.apply(np.zeros((0, 0)), 0, np.zeros(0), np.float64).shape == (0,)
    # same(): NaN positions and every other bit
    assert cc.same([np.nan, 1.0, -0.0], [-np.nan, 1.0, -0.0]) and not cc.same([0.0], [-0.0]) and not cc.same([np.nan, 1.0], [1.0, np.nan])


@pytest.mark.parametrize("name", cc.CASES)
def test_every_case_is_what_it_is_for(name):
    n, p, c, v, status, good = cc.case(name)
    assert 0 <= n <= 513 and len(p) == n + 1 and p[0] == 0 and len(c) == len(v) == p[-1]
    for dtype in cc.DTYPES:
        inv, got = cc.restated(name, dtype)
        assert got == status and inv.dtype == dtype and inv.shape == (n, cc.ld_of(n))
        assert np.all(inv[:, n:] == 0.0) and not np.signbit(inv[:, n:]).any()
        if status[0]:
            assert np.array_equal(inv[:, :n], np.eye(n))
    row = np.repeat(np.arange(n), np.diff(p))
    if name == "duplicates_unsorted":
        assert len(np.unique(row.astype(np.int64) * n + c)) < len(c) and np.any(np.diff(c[p[0]:p[1]]) < 0)
        order = np.lexsort((-np.arange(len(c)), row))  # every row's entries in reverse: another order of the sums, other bits
        assert not cc.same(cc.densify(n, p, c[order], v[order])[0], cc.densify(n, p, c, v)[0])
    if name == "empty_row":
        assert p[2] == p[3]
    if name == "zero":
        assert len(v) > 0 and not np.any(v)
    if name == "columns_outside":
        assert {-1, n} <= set(c.tolist()) and c.min() == -2 ** 31 and c.max() == 2 ** 31 - 1
    if name in ("nan", "inf"):
        assert np.sum(~np.isfinite(v)) == 1
        if name == "nan":  # (an Inf is chosen as a pivot, t = 0, and what it leaves non-finite is its own dead column)
            assert np.any(np.isnan(cc.restated(name, np.float64)[0]))
    if name == "permutation_64":
        A = cc.densify(n, p, c, v)[0]
        assert np.sum(np.argmax(np.abs(A), axis=0) != np.arange(n)) > n // 2, "rows that swap"
    if name == "poisson2D_Ac":
        assert n == 38
    if name == "grid_512_level_3":
        assert n == 376


def test_the_restated_inverse_is_as_good_as_numpys_up_to_a_constant():
    worst = 0.0
    for name in cc.CASES:
        n, p, c, v, status, good = cc.case(name)
        if not good:
            continue
        A = cc.densify(n, p, c, v)[0]
        mine, numpys = cc.residual(A, cc.restated(name, np.float64)[0]), cc.residual(A, np.linalg.inv(A))
        ratio = mine / max(numpys, 2.0 ** -53)
        print("%-22s %4d rows: max |A X - I| %.3e, numpy's %.3e, ratio %.2f" % (name, n, mine, numpys, ratio))
        worst = max(worst, ratio)
    print("the largest ratio %.2f" % worst)
    assert worst <= RESIDUAL_RATIO


@pytest.mark.parametrize("dtype", cc.DTYPES, ids=["float64", "float32"])
def test_integer_operands_are_exact_in_any_order_and_a_lost_element_would_show(dtype):
    for n in cc.SIZES:
        inv, r, z = cc.int_operands(n, dtype)
        assert inv.shape == (n, cc.ld_of(n)) and np.all(inv[:, n:] == 7)
        assert np.array_equal(cc.apply(inv, n, r, dtype), z)
        if n > 1:
            lost = inv.copy()
            lost[:, n - 1] = 0
            assert not np.array_equal(cc.apply(lost, n, r, dtype), z) or not np.any(inv[:, n - 1])
        g, rg = cc.general_operands(n, dtype)
        assert np.all(np.isnan(g[:, n:])) and np.all(np.isfinite(cc.apply(g, n, rg, dtype)))


def test_the_2048_row_matrix_is_banded_and_dominant():
    n, p, c, v, A = cc.banded_2048()
    assert n == cc.MAX_N == 2048 and int(np.diff(p).max()) == 7
    d = np.abs(np.diag(A))
    assert np.all(d > np.sum(np.abs(A), axis=1) - d)
