"""The numpy restatement of the multicolour Gauss-Seidel / SSOR preconditioner (mcgs_cases.py) without a device: the colouring is a
proper one and uses the colours first fit allows, the plan is a permutation, the colour sweeps -- for every group size -- are a
plain sequential SOR in the colour order to a summation bound, the apply is symmetric, and eight PCG iterations on
tests/golden/poisson2D.mtx with the symmetric sweep at omega = 1 leave less than a tenth of the r'r the diagonal leaves."""
import numpy as np
import pytest

import mcgs_cases as mc


def _vectors(rows, dtype, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=rows).astype(dtype), rng.uniform(-1.0, 1.0, size=rows).astype(dtype)


def test_fmix32_is_the_murmur3_finaliser():
    # the finaliser's published fixed point and two values worked by hand in 32-bit arithmetic
    assert int(mc.fmix32(np.uint32(0))) == 0
    h = 1
    h ^= h >> 16
    h = h * 0x85ebca6b & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xc2b2ae35 & 0xFFFFFFFF
    h ^= h >> 16
    assert int(mc.fmix32(np.uint32(1))) == h == 0x514E28B7
    assert len(set(mc.keys(4099, 7).tolist())) == 4099


@pytest.mark.parametrize("seed", mc.SEEDS)
@pytest.mark.parametrize("name", mc.COLOURING)
def test_the_colouring_is_proper_and_every_row_took_the_first_free_colour(name, seed):
    rows, p, c, v = mc.matrix(name)
    col_of, status = mc.colour(rows, p, c, seed)
    colours, rounds, conflicts, overflowed = status
    print("%s, seed %#x: %d colours in %d rounds" % (name, seed, colours, rounds))
    assert conflicts == 0 and overflowed == 0
    assert col_of.dtype == np.int32 and len(col_of) == rows
    if rows == 0:
        assert status == [0, 0, 0, 0]
        return
    assert col_of.min() == 0 and col_of.max() == colours - 1 and colours <= mc.MAX_COLOURS
    row = np.repeat(np.arange(rows), np.diff(p))
    off = c != row
    assert not np.any(col_of[row[off]] == col_of[c[off]])
    # no row could have taken a smaller colour: every colour below its own is held by a neighbour
    degree = np.bincount(row[off], minlength=rows)
    assert np.all(col_of <= degree)
    for i in np.flatnonzero(col_of > 0)[:200]:
        nb = c[p[i]:p[i + 1]]
        assert set(range(col_of[i])) <= set(col_of[nb[nb != i]].tolist())
    if not off.any():
        assert colours == 1 and rounds == 1


def test_two_seeds_colour_differently_and_a_clique_overflows():
    rows, p, c, v = mc.matrix("grid_37x29")
    a, b = (mc.colour(rows, p, c, s)[0] for s in mc.SEEDS)
    assert np.any(a != b)
    n, p, c, v = mc.clique(66)
    col_of, status = mc.colour(n, p, c, 0)
    assert status[0] == 64 and status[1] == 66 and status[3] == 2 and status[2] == 3 * 2  # three rows at colour 63: six ordered pairs
    rows, p, c, v = mc.one_sided()
    _, status = mc.colour(rows, p, c, 0)
    assert status[3] == 0  # (whether the one-sided entry makes a conflict depends on the keys)


@pytest.mark.parametrize("name", mc.SWEEPS)
def test_the_plan_is_a_permutation_of_the_matrix(name):
    rows, p, c, v = mc.matrix(name)
    pl, col_of, status = mc.plan(name)
    assert sorted(pl.order.tolist()) == list(range(rows))
    assert pl.colour_ptr[0] == 0 and np.all(np.diff(pl.colour_ptr) >= 0) and np.all(pl.colour_ptr[pl.colours:] == rows) and len(pl.colour_ptr) == 65
    for ci in range(pl.colours):
        seg = pl.order[pl.colour_ptr[ci]:pl.colour_ptr[ci + 1]]
        assert len(seg) and np.all(col_of[seg] == ci) and np.all(np.diff(seg) > 0)
    for k in (0, rows // 2, rows - 1) if rows else ():
        i = pl.order[k]
        assert np.array_equal(pl.c[pl.p[k]:pl.p[k + 1]], c[p[i]:p[i + 1]]) and np.array_equal(pl.v[pl.p[k]:pl.p[k + 1]], v[p[i]:p[i + 1]])
    assert pl.p[-1] == len(c) and pl.group in (4, 8, 16, 32, 64)
    assert mc.default_group(10, 50) == 8 and mc.default_group(10, 40) == 4 and mc.default_group(10, 41) == 8 and mc.default_group(1, 9999) == 64
    assert mc.default_group(0, 0) == 4 and mc.default_group(7, 0) == 4


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["poisson2D", "grid_37x29", "ragged", "long_row", "path_65"])
def test_the_colour_sweeps_are_a_sequential_sor_to_a_summation_bound(name, dtype):
    rows, p, c, v = mc.matrix(name)
    pl, _, status = mc.plan(name)
    assert status[2] == 0
    b, x0 = _vectors(rows, dtype)
    minv = mc.minv_of(rows, p, c, v, dtype)
    last = pl.colours - 1
    for omega in mc.OMEGAS:
        for first, to in ((0, last), (last, 0), (last // 2, last // 2)):
            # colour by colour, the sequential run restarted from the restatement's state so that the bound is one row's
            x = x0.copy()
            step = -1 if to < first else 1
            worst = 0.0
            for ci in range(first, to + step, step):
                want, bound = mc.sequential_sor(pl, ci, ci, omega, b, minv, x, dtype)
                seen = None
                for group in mc.GROUPS:
                    got = mc.sweep(pl, ci, ci, omega, b, minv, x, dtype, group)
                    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
                    assert np.all(err <= bound), (name, omega, ci, group, float(np.max(err - bound)))
                    worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
                    touched = got != x
                    assert not np.any(touched[np.setdiff1d(np.arange(rows), pl.order[pl.colour_ptr[ci]:pl.colour_ptr[ci + 1]])])
                    seen = got if group == pl.group else seen
                x = seen
            assert np.array_equal(x, mc.sweep(pl, first, to, omega, b, minv, x0, dtype))
            print("%s, %s, omega %.1f, colours %d ... %d: worst error / bound %.3f" % (name, np.dtype(dtype).name, omega, first, to, worst))
    # rows of up to `group` entries have one product per lane: the sum does not depend on the lanes left empty
    if name == "grid_37x29":
        a = mc.sweep(pl, 0, last, 1.0, b, minv, x0, dtype, 8)
        assert np.array_equal(a, mc.sweep(pl, 0, last, 1.0, b, minv, x0, dtype, 64))


def test_a_nan_reaches_only_the_rows_that_store_its_column():
    rows, p, c, v = mc.matrix("grid_37x29")
    pl, col_of, _ = mc.plan("grid_37x29")
    b, x0 = _vectors(rows, np.float64)
    minv = mc.minv_of(rows, p, c, v, np.float64)
    j = 517
    x0[j] = np.nan
    ci = int(col_of[j - 1])  # a colour that holds a neighbour of j, and so not j's own
    got = mc.sweep(pl, ci, ci, 1.0, b, minv, x0, np.float64)
    row = np.repeat(np.arange(rows), np.diff(p))
    stores = np.unique(row[c == j])
    want = np.intersect1d(stores, pl.order[pl.colour_ptr[ci]:pl.colour_ptr[ci + 1]])
    assert len(want) and np.array_equal(np.flatnonzero(np.isnan(got)), np.union1d(want, [j]))


def test_the_apply_is_a_symmetric_operator_at_every_omega():
    rows, p, c, v = mc.matrix("grid_37x29")  # (symmetric in its values, which the golden poisson2D.mtx is not quite)
    pl, _, _ = mc.plan("grid_37x29")
    minv = mc.minv_of(rows, p, c, v, np.float64)
    u, w = _vectors(rows, np.float64, seed=9)
    for omega in mc.OMEGAS:
        mu, mw = mc.apply(pl, omega, u, minv, np.float64), mc.apply(pl, omega, w, minv, np.float64)
        assert abs(w @ mu - u @ mw) <= 1e-13 * (np.abs(w) @ np.abs(mu)) and u @ mu > 0 and w @ mw > 0


def test_eight_pcg_iterations_on_poisson2d_leave_a_tenth_of_the_diagonals_residual():
    rows, p, c, v = mc.matrix("poisson2D")
    assert rows == 367
    pl, _, status = mc.plan("poisson2D")
    minv = mc.minv_of(rows, p, c, v, np.float64)
    b = np.ones(rows)
    diag = mc.pcg(rows, p, c, v, b, lambda r: minv * r)
    ssor = mc.pcg(rows, p, c, v, b, lambda r: mc.apply(pl, 1.0, r, minv, np.float64))
    over = mc.pcg(rows, p, c, v, b, lambda r: mc.apply(pl, 1.5, r, minv, np.float64))
    print("poisson2D, %d colours in %d rounds: r'r 367 -> the diagonal %.4g, the symmetric sweep at omega 1 %.4g, at omega 1.5 %.4g" % (
        status[0], status[1], diag[-1], ssor[-1], over[-1]))
    assert ssor[-1] < 0.1 * diag[-1]
    assert over[-1] < diag[-1]
