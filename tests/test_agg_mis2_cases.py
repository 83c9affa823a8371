"""The numpy restatement of include/spmv_hip_agg_mis2.h (agg_mis2_cases.py) without a device: the distance-2 aggregates partition
the rows and are numbered by ascending root; on a symmetric pattern no two roots lie within two steps of each other, every row
lies within two steps of its root and every aggregate is connected; the statuses are the recorded ones; the 512 x 512 grid reaches
<= 1000 rows in three coarsenings that each shrink by more than 4 and leave no single row; eight PCG iterations on
tests/golden/poisson2D.mtx with the two-level cycle over these aggregates leave less than the recorded fraction of the r'r the
diagonal leaves; and the grouped restriction is the plain one at a group of one lane and within members 2^-53 sum |r_m| of
math.fsum at every group."""
import math

import numpy as np
import pytest

import agg_cases as ac
import agg_mis2_cases as a2
import mcgs_cases as mc


def _symmetric(name):
    """Whether the stored pattern of the matrix is that of its transpose (looked at, not assumed)."""
    import scipy.sparse as sp
    rows, p, c, v = ac.matrix(name)
    S = sp.csr_matrix((np.ones(len(c)), c.copy(), p.copy()), shape=(rows, rows))  # (sum_duplicates works in place)
    S.sum_duplicates()
    S.data[:] = 1.0
    return (S - S.T).nnz == 0


def test_the_one_pattern_that_is_not_symmetric_is_the_one_sided_grid():
    """The distance properties below are held on every matrix whose stored pattern is symmetric: looked at here, all but one_sided
    (long_row stores its far couplings both ways)."""
    assert [n for n in ac.MATRICES if not _symmetric(n)] == ["one_sided"]


@pytest.mark.parametrize("theta", ac.THETAS)
@pytest.mark.parametrize("seed", ac.SEEDS)
@pytest.mark.parametrize("name", ac.MATRICES)
def test_the_aggregates_partition_the_rows_and_the_roots_are_a_distance_two_independent_set(name, seed, theta):
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    rows, p, c, v = ac.matrix(name)
    agg, status, joins = a2.aggregate_and_roots(rows, p, c, v, theta, seed)
    aggregates, rounds, largest, singletons = status
    print("%s, seed %#x, theta %.2f: %d rows in %d aggregates, %d rounds, largest %d, %d singletons" % (name, seed, theta, rows, aggregates, rounds,
                                                                                                        largest, singletons))
    assert agg.dtype == np.int32 and len(agg) == rows
    if rows == 0:
        assert status == [0, 0, 0, 0]
        return
    assert agg.min() == 0 and agg.max() == aggregates - 1 and len(np.unique(agg)) == aggregates
    sizes = np.bincount(agg, minlength=aggregates)
    assert sizes.min() >= 1 and sizes.max() == largest and int(np.sum(sizes == 1)) == singletons
    roots = np.flatnonzero(joins == np.arange(rows))
    assert len(roots) == aggregates and np.array_equal(agg[roots], np.arange(aggregates)) and np.array_equal(agg, agg[joins])
    row, col = ac.neighbours(rows, p, c, v, theta)
    degree = np.bincount(row, minlength=rows)
    assert np.all(sizes[agg[degree == 0]] == 1), "a row without a neighbour is an aggregate of its own"
    S = sp.csr_matrix((np.ones(len(row)), (row, col)), shape=(rows, rows))
    S.sum_duplicates()
    S.data[:] = 1.0
    two = (S + S @ S).tocsr()  # > 0 where a row reaches another in one or two stored steps
    # every row reaches its root in at most two stored steps (the joins follow stored entries, whatever the pattern)
    others = np.flatnonzero(joins != np.arange(rows))
    assert not len(others) or np.all(np.asarray(two[others, joins[others]]).ravel() > 0), "a row further than two steps from its root"
    if theta != 0.0 or not _symmetric(name):  # (a threshold makes "neighbour" one-sided, as a one-sided pattern does)
        return
    assert (S - S.T).nnz == 0
    between = two[roots][:, roots].tolil()
    between.setdiag(0)
    assert between.nnz == 0, "two roots within two steps of each other"
    inside = S.tocoo()
    same = agg[inside.row] == agg[inside.col]
    parts, label = csgraph.connected_components(sp.csr_matrix((np.ones(int(same.sum())), (inside.row[same], inside.col[same])), shape=(rows, rows)),
                                                directed=False)
    assert parts == aggregates and len(set(zip(label.tolist(), agg.tolist()))) == aggregates, "an aggregate that is not connected"


RECORDED = {  # {aggregates, rounds, largest, singletons} at theta 0 under the two seeds
    "poisson2D": ([38, 4, 19, 0], [38, 3, 18, 0]),
    "grid_37x29": ([160, 4, 12, 0], [152, 4, 13, 0]),
    "grid_13x13x13": ([218, 5, 20, 0], [226, 5, 20, 0]),
    "bus1138_like": ([400, 4, 25, 144], [393, 4, 18, 144]),
    "path_4099": ([1124, 4, 5, 0], [1126, 3, 5, 0]),
    "star_5000": ([1, 1, 5001, 0], [1, 1, 5001, 0]),
    "clique_66": ([1, 1, 66, 0], None),
    "one_sided": ([12, 3, 7, 0], [12, 3, 8, 0]),
    "isolated": ([45, 3, 11, 7], [47, 3, 10, 7]),
    "path_0": ([0, 0, 0, 0], None),
    "path_1": ([1, 1, 1, 1], None),
    "path_2": ([1, 1, 2, 0], None),
}


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_the_statuses_are_the_recorded_ones(name):
    for seed, want in zip(ac.SEEDS, RECORDED[name]):
        if want is not None:
            got = a2.aggregate(*ac.matrix(name), 0.0, seed)[1]
            print("%s, seed %#x: %s" % (name, seed, got))
            assert got == want, (name, seed)


def test_the_hierarchy_on_the_512_grid_reaches_a_thousand_rows_in_three_coarsenings_without_a_single_row():
    levels = a2.grid_512_hierarchy()
    sizes, entries = [n for n, _, _ in levels], [e for _, e, _ in levels]
    print("grid 512 x 512: rows per level %s, operator complexity %.2f, statuses %s" % (sizes, sum(entries) / entries[0], [s for _, _, s in levels[:-1]]))
    assert len(sizes) <= 4 and sizes[-1] <= 1000
    assert sizes == [262144, 36783, 3806, 376]
    for (fine, _, status), (below, _, _) in zip(levels, levels[1:]):
        assert fine >= 4 * below and status[0] == below and status[3] == 0, (fine, below, status)


def test_eight_pcg_iterations_on_poisson2d_with_the_two_level_cycle_beat_the_diagonal_by_the_recorded_factor():
    import scipy.sparse as sp
    rows, p, c, v = ac.matrix("poisson2D")
    A = sp.csr_matrix((v, c, p), shape=(rows, rows))
    b = np.ones(rows)
    minv = mc.minv_of(rows, p, c, v, np.float64)
    pl, _ = a2.plan("poisson2D")
    co = a2.coarse("poisson2D")
    Ac = co.dense(co.values(v))
    assert np.all(np.linalg.eigvalsh(Ac + Ac.T) > 0)
    smooth = ac.smoother_of(rows, p, c, v, np.float64)
    diagonal = ac.pcg(rows, p, c, v, b, lambda r: minv * r)
    for omega in (1.0, 1.5):
        cycle = ac.pcg(rows, p, c, v, b, ac.two_level_cycle(A, pl, smooth, lambda rc: np.linalg.solve(Ac, rc), omega))
        print("omega %.1f: r'r 367 -> %.3e with the two-level cycle over %d distance-2 aggregates, %.3e with the diagonal: ratio %.2e" % (
            omega, cycle[-1], pl.aggregates, diagonal[-1], cycle[-1] / diagonal[-1]))
        assert np.isfinite(cycle[-1]) and cycle[-1] < a2.PCG_FACTOR * diagonal[-1]


def _plans():
    out = [("blocks of %d rows" % n, ac.blocks(n, 7)) for n in ac.SIZES]
    return out + [(name, a2.plan(name)[0]) for name in ("grid_13x13x13", "long_row", "star_5000")]


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_the_grouped_restriction_is_the_plain_one_at_one_lane_and_within_the_bound_of_fsum_at_every_group(dtype):
    for what, pl in _plans():
        r = np.random.default_rng(pl.rows + 3).uniform(-1.0, 1.0, size=pl.rows).astype(dtype)
        one = a2.restrict_group(pl, 1, r, dtype)
        assert one.dtype == dtype and np.array_equal(one.view(np.uint8), ac.restrict(pl, r, dtype).view(np.uint8)), what
        r64 = r.astype(np.float64)
        exact = np.array([math.fsum(r64[pl.member[a:b]]) for a, b in zip(pl.member_ptr[:-1], pl.member_ptr[1:])])
        mag = np.array([math.fsum(np.abs(r64[pl.member[a:b]])) for a, b in zip(pl.member_ptr[:-1], pl.member_ptr[1:])])
        bound = np.diff(pl.member_ptr.astype(np.int64)) * 2.0 ** -53 * mag
        for group in a2.GROUPS:
            got = a2.restrict_group(pl, group, r, np.float64)  # the sums before the store's rounding
            assert np.all(np.abs(got - exact) <= bound), (what, group)
            stored = a2.restrict_group(pl, group, r, dtype)
            assert np.array_equal(stored.view(np.uint8), got.astype(dtype).view(np.uint8)), "one rounding, at the store"
    # a NaN stays in its aggregate at every group
    pl = a2.plan("grid_13x13x13")[0]
    bad = np.random.default_rng(4).uniform(-1.0, 1.0, size=pl.rows).astype(dtype)
    bad[500] = np.nan
    for group in a2.GROUPS:
        assert np.flatnonzero(np.isnan(a2.restrict_group(pl, group, bad, dtype))).tolist() == [int(pl.agg[500])]


def test_the_recommended_group_is_the_smallest_power_of_two_that_holds_the_mean_aggregate():
    for rows, aggregates, want in ((262144, 36783, 8), (110592, 10145, 16), (5001, 1, 64), (10, 10, 1), (10, 5, 2), (11, 5, 4), (64, 1, 64)):
        assert a2.group_of(rows, aggregates) == want
