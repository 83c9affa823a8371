"""The numpy restatement of the aggregation multigrid level (agg_cases.py) without a device: the aggregates partition the rows,
the roots are an independent set that covers, on a symmetric pattern every row is its root or beside it, the member lists are
ascending and complete, the coarse matrix is the dense P'AP -- exactly on small integers, to run 2^-53 sum |t| on general values
-- restriction and prolongation are P' and P, a hierarchy ends, and eight PCG iterations on tests/golden/poisson2D.mtx with the
two-level cycle leave less than the recorded fraction of the r'r the diagonal leaves."""
import numpy as np
import pytest

import agg_cases as ac
import mcgs_cases as mc

SYMMETRIC = tuple(n for n in ac.MATRICES if n != "one_sided")


@pytest.mark.parametrize("theta", ac.THETAS)
@pytest.mark.parametrize("seed", ac.SEEDS)
@pytest.mark.parametrize("name", ac.MATRICES)
def test_the_aggregates_partition_the_rows_and_the_member_lists_are_ascending_and_complete(name, seed, theta):
    rows, p, c, v = ac.matrix(name)
    agg, status = ac.aggregate(rows, p, c, v, theta, seed)
    aggregates, rounds, largest, singletons = status
    print("%s, seed %#x, theta %.2f: %d rows in %d aggregates, %d rounds, largest %d, %d singletons" % (name, seed, theta, rows, aggregates, rounds,
                                                                                                        largest, singletons))
    assert agg.dtype == np.int32 and len(agg) == rows
    if rows == 0:
        assert status == [0, 0, 0, 0]
        return
    assert agg.min() == 0 and agg.max() == aggregates - 1 and len(np.unique(agg)) == aggregates
    pl = ac.Plan(rows, agg, status)
    assert sorted(pl.member.tolist()) == list(range(rows)) and pl.member_ptr[0] == 0 and pl.member_ptr[-1] == rows
    sizes = np.diff(pl.member_ptr)
    assert sizes.min() >= 1 and sizes.max() == largest and int(np.sum(sizes == 1)) == singletons
    for I in range(aggregates):
        m = pl.member[pl.member_ptr[I]:pl.member_ptr[I + 1]]
        assert np.all(np.diff(m) > 0) and np.all(agg[m] == I)
    # every row joined a root beside it, and the aggregates are numbered by their roots in ascending row index
    _, _, joins = ac.aggregate_and_roots(rows, p, c, v, theta, seed)
    roots = np.flatnonzero(joins == np.arange(rows))
    assert len(roots) == aggregates and np.array_equal(agg[roots], np.arange(aggregates)) and np.array_equal(agg, agg[joins])
    row, col = ac.neighbours(rows, p, c, v, theta)
    beside = set(zip(row.tolist(), col.tolist()))
    if name in SYMMETRIC and theta == 0.0:  # (a threshold makes "neighbour" one-sided, as a one-sided pattern does)
        assert not any((int(a), int(b)) in beside for a in roots[:60] for b in roots[:60]), "two roots are neighbours"
    others = np.flatnonzero(joins != np.arange(rows))
    assert all((int(i), int(joins[i])) in beside for i in others)
    if name in SYMMETRIC and theta == 0.0:
        assert all((int(joins[i]), int(i)) in beside for i in others), "a non-root is a neighbour of its root"
    degree = np.bincount(row, minlength=rows)
    assert np.all(sizes[agg[degree == 0]] == 1), "a row without a neighbour is an aggregate of its own"


def test_the_named_cases_are_what_they_are_for():
    pl, status = ac.plan("star_5000")
    assert status == [1, 1, 5001, 0] and ac.coarse("star_5000").nnz_c == 1
    assert np.diff(ac.coarse("star_5000").entry_ptr).tolist() == [3 * 5000 + 1]
    rows, p, c, v = ac.matrix("isolated")
    lens = np.diff(p)
    assert int(np.sum(lens == 0)) == 4 and int(np.sum((lens == 1) & (c[np.minimum(p[:-1], len(c) - 1)] == np.arange(rows)))) >= 3
    assert ac.plan("clique_66")[1] == [1, 1, 66, 0] and ac.plan("path_2")[1] == [1, 1, 2, 0] and ac.plan("path_0")[1] == [0, 0, 0, 0]
    assert int(np.diff(ac.coarse("long_row").entry_ptr).max()) >= 20
    # theta changes the neighbours where the values differ: the long row's far couplings are weak
    assert ac.aggregate(*ac.matrix("long_row"), 0.25, 0)[1] != ac.aggregate(*ac.matrix("long_row"), 0.0, 0)[1]


@pytest.mark.parametrize("name", ac.MATRICES)
def test_the_coarse_matrix_is_the_dense_galerkin_product(name):
    rows, p, c, v = ac.matrix(name)
    pl, _ = ac.plan(name)
    co = ac.coarse(name)
    assert co.row_ptr[0] == 0 and co.row_ptr[-1] == co.nnz_c and len(co.row_ptr) == pl.aggregates + 1
    assert sorted(co.order.tolist()) == list(range(co.nnz)) and co.entry_ptr[-1] == co.nnz
    for I in range(pl.aggregates):
        assert np.all(np.diff(co.column[co.row_ptr[I]:co.row_ptr[I + 1]]) > 0), "distinct ascending columns"
    # ties keep the member-major order: ascending fine row, then stored position -- positions ascend inside a run
    for e in range(co.nnz_c):
        assert np.all(np.diff(co.order[co.entry_ptr[e]:co.entry_ptr[e + 1]]) > 0)
    # small integers: every order gives the same sum
    ints = np.random.default_rng(3).integers(-8, 9, size=len(v)).astype(np.float64)
    assert np.array_equal(co.dense(co.values(ints)), ac.dense_galerkin(pl, rows, p, c, ints))
    # general values: to the bound of two summation orders
    g = ac.general_values(name)
    got, want = co.dense(co.values(g)), ac.dense_galerkin(pl, rows, p, c, g)
    assert np.all(np.abs(got - want) <= co.dense(co.bound(g)))
    assert np.all(want[co.dense(np.ones(co.nnz_c)) == 0] == 0), "an entry of P'AP outside the pattern"


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_restriction_and_prolongation_are_the_transposed_pair(dtype):
    import scipy.sparse as sp
    name = "grid_37x29"
    rows = ac.matrix(name)[0]
    pl, _ = ac.plan(name)
    P = sp.csr_matrix((np.ones(rows), (np.arange(rows), pl.agg)), shape=(rows, pl.aggregates))
    ints = np.random.default_rng(4).integers(-8, 9, size=rows).astype(dtype)
    assert np.array_equal(ac.restrict(pl, ints, dtype), (P.T @ ints.astype(np.float64)).astype(dtype))
    e = np.random.default_rng(5).integers(-8, 9, size=pl.aggregates).astype(dtype)
    for omega in ac.OMEGAS:
        assert np.array_equal(ac.prolong_add(pl, omega, e, ints, dtype), (ints + omega * (P @ e.astype(np.float64))).astype(dtype))
    bad = ints.copy()
    bad[500] = np.nan
    assert np.flatnonzero(np.isnan(ac.restrict(pl, bad, dtype))).tolist() == [pl.agg[500]]
    for n in ac.SIZES:
        b = ac.blocks(n, 7)
        assert sorted(b.member.tolist()) == list(range(n)) and b.member_ptr[-1] == n


def test_the_hierarchy_on_the_grid_ends():
    rows, p, c, v = ac.matrix("grid_37x29")
    sizes, entries = [rows], [len(c)]
    while rows > 1 and len(sizes) < 20:
        agg, status = ac.aggregate(rows, p, c, v, 0.0, ac.SEEDS[0])
        pl = ac.Plan(rows, agg, status)
        co = ac.Coarse(pl, p, c)
        v = co.values(v)
        rows, p, c = pl.aggregates, co.row_ptr, co.column
        if rows == sizes[-1]:
            break
        sizes.append(rows)
        entries.append(len(c))
    print("grid_37x29: rows per level %s, operator complexity %.2f" % (sizes, sum(entries) / entries[0]))
    assert sizes[-1] == 1 and all(b < a for a, b in zip(sizes, sizes[1:])) and len(sizes) <= 12
    assert sizes[1] < 0.5 * sizes[0]


def test_eight_pcg_iterations_on_poisson2d_with_the_two_level_cycle_beat_the_diagonal_by_the_recorded_factor():
    import scipy.sparse as sp
    rows, p, c, v = ac.matrix("poisson2D")
    A = sp.csr_matrix((v, c, p), shape=(rows, rows))
    b = np.ones(rows)
    minv = mc.minv_of(rows, p, c, v, np.float64)
    pl, _ = ac.plan("poisson2D")
    co = ac.coarse("poisson2D")
    Ac = co.dense(co.values(v))
    assert np.all(np.linalg.eigvalsh(Ac + Ac.T) > 0)  # (the file's matrix is symmetric to 7 % of its largest entry only)
    smooth = ac.smoother_of(rows, p, c, v, np.float64)
    diagonal = ac.pcg(rows, p, c, v, b, lambda r: minv * r)
    for omega in (1.0, 1.5):
        cycle = ac.pcg(rows, p, c, v, b, ac.two_level_cycle(A, pl, smooth, lambda rc: np.linalg.solve(Ac, rc), omega))
        print("omega %.1f: r'r 367 -> %.3e with the two-level cycle over %d aggregates, %.3e with the diagonal" % (omega, cycle[-1], pl.aggregates,
                                                                                                                 diagonal[-1]))
        assert np.isfinite(cycle[-1]) and cycle[-1] < ac.PCG_FACTOR * diagonal[-1]
