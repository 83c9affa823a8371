"""graph_size_cases.py without a device: every figure it quotes -- rows, chunks of the chunk scan and the lanes of its last trip, the
aggregates, the bits of the Galerkin key and of the plan's sort, the four levels of the 512 x 512 grid's distance-1 hierarchy --
computed by the restatements, and the restated Galerkin product of every level of that hierarchy held to sums formed another way:
the pattern to scipy's P' A P, the values to long-double sums grouped by (agg[row], agg[column]) within Coarse.bound, and to
scipy's own fp64 triple product within twice that."""
import numpy as np
import pytest

import agg_cases as ac
import graph_size_cases as gs


def test_bits_of_is_the_smallest_width_that_holds_every_key():
    assert [gs.bits_of(k) for k in (0, 1, 2, 3, 4, 5, 2 ** 16, 2 ** 16 + 1, 2 ** 32, 2 ** 32 + 1)] == [1, 1, 1, 2, 2, 3, 16, 17, 32, 33]
    for keys in (1, 2, 3, 65536 ** 2, 65537 ** 2, 95432 ** 2, 2 ** 63, 2 ** 64):
        bits = gs.bits_of(keys)
        assert (1 << bits) >= min(keys, 2 ** 64) and (bits == 1 or (1 << (bits - 1)) < keys)
    # the edge: 65 536 aggregates are the last whose key an unsigned holds
    assert gs.bits_of(65536 ** 2) == 32 and 65536 ** 2 - 1 == 2 ** 32 - 1
    assert gs.bits_of(65537 ** 2) == 33 and 65537 ** 2 - 1 > 2 ** 32 - 1


@pytest.mark.parametrize("name", gs.MATRICES)
def test_rows_and_chunks_are_the_quoted_ones(name):
    rows, p, c, v = gs.matrix(name)
    want_rows, chunks, last, trips = gs.CHUNKS[name]
    assert rows == want_rows and len(p) == rows + 1 and p[-1] == len(c) == len(v)
    assert gs.chunks_of(rows) == (chunks, last, trips)
    assert chunks == -(-rows // 1024) and trips == -(-chunks // 64) and last == chunks - 64 * (trips - 1)
    d, g = gs.distinct_values(name), gs.general_values(name)
    for values in (d, g):
        assert len(values) == len(v) and np.all(values.astype(np.float32).astype(np.float64) != values), "doubles that no float holds"
    # no two entries of a row alike: a copy from another entry of the row shows
    row = np.repeat(np.arange(rows), np.diff(p))
    order = np.lexsort((d, row))
    assert not np.any((row[order][1:] == row[order][:-1]) & (d[order][1:] == d[order][:-1]))


def test_the_two_paths_lie_on_either_side_of_the_chunk_scans_first_carry():
    assert gs.chunks_of(65536) == (64, 64, 1) and gs.chunks_of(65537) == (65, 1, 2)
    assert gs.chunks_of(90000) == (88, 24, 2) and gs.chunks_of(200001) == (196, 4, 4) and gs.chunks_of(262144) == (256, 64, 4)


@pytest.mark.parametrize("name", gs.GALERKIN)
def test_aggregates_and_key_bits_are_the_quoted_ones(name):
    agg, status = gs.aggregates(name)
    aggregates, key_bits, plan_bits = gs.FIGURES[name]
    assert status[0] == aggregates == int(agg.max()) + 1
    assert gs.bits_of(aggregates ** 2) == key_bits and gs.bits_of(aggregates) == plan_bits
    assert (key_bits > 32) == (aggregates > 65536)
    co = gs.coarse(name)
    assert co.nnz_c == co.row_ptr[-1] == len(co.column) and co.entry_ptr[-1] == co.nnz
    if name == "grid_512x512":
        assert status == gs.HIERARCHY[0][1] and co.nnz_c == gs.HIERARCHY[0][2] and status[3] == 30877
    # the largest key the sort sees: above 2^32 exactly where the case is there for it
    a = agg.astype(np.int64)
    largest = int(a.max()) * aggregates + int(a.max())
    assert largest < 1 << key_bits and (largest >= 1 << 32) == (key_bits > 32)


def test_the_distance_2_aggregates_are_the_quoted_ones():
    _, status = gs.aggregates("path_200001", 2)
    assert status[0] == gs.DISTANCE_2_AGGREGATES["path_200001"] == 54967 and status[3] == 0
    _, status = gs.aggregates("grid_512x512", 2)
    assert status[0] == 36783 and status[0] < 65536, "no distance-2 plan above 65 536 aggregates: the symbolic code is shared"


@pytest.mark.parametrize("name", gs.BLOCKS)
def test_the_hand_made_plans_have_exactly_the_aggregates_of_the_edge(name):
    pl = gs.plan(name)
    rows = gs.BLOCKS[name]
    aggregates, key_bits, plan_bits = gs.FIGURES[name]
    assert (pl.rows, pl.aggregates, pl.largest) == (rows, aggregates, 2) and gs.matrix(name)[0] == rows
    assert gs.bits_of(aggregates ** 2) == key_bits and gs.bits_of(aggregates) == plan_bits
    assert np.array_equal(np.unique(pl.agg), np.arange(aggregates)) and np.all(np.diff(pl.agg) >= 0)
    co = gs.coarse(name)
    assert co.nnz_c == 3 * aggregates - 2, "the coarse matrix of a path under consecutive blocks is a path"
    a = pl.agg.astype(np.int64)
    row = np.repeat(np.arange(rows), np.diff(gs.matrix(name)[1]))
    key = a[row] * aggregates + a[gs.matrix(name)[2]]
    assert (int(key.max()) >= 1 << 32) == (name == "blocks_65537") and int(key.max()) == aggregates ** 2 - 1


def test_the_hierarchy_is_the_quoted_one():
    levels = gs.hierarchy()
    assert len(levels) == len(gs.HIERARCHY) == 4
    for L, (rows, status, nnz_c, key_bits, longest) in zip(levels, gs.HIERARCHY):
        assert (L.rows, L.status, L.coarse.nnz_c, L.key_bits, L.longest) == (rows, status, nnz_c, key_bits, longest)
    for fine, coarse in zip(levels, levels[1:]):
        assert coarse.rows == fine.plan.aggregates and coarse.p is fine.coarse.row_ptr and coarse.c is fine.coarse.column and coarse.v is fine.cv
    assert [gs.bits_of(L.plan.aggregates) for L in levels] == [17, 16, 14, 13]
    # at theta 0 no aggregate depends on a value: the grid's own values give the same first level
    rows, p, c, v = gs.matrix("grid_512x512")
    agg, status = gs.aggregates("grid_512x512")
    assert status == levels[0].status and np.array_equal(agg, levels[0].agg)


@pytest.mark.parametrize("level", range(len(gs.HIERARCHY)))
def test_the_restated_product_of_every_level_is_p_transposed_a_p_by_two_other_ways(level):
    import scipy.sparse as sp
    L = gs.hierarchy()[level]
    rows, na, co = L.rows, L.plan.aggregates, L.coarse
    # (a) the pattern: scipy's P' A P with sorted indices
    A = sp.csr_matrix((L.v, L.c, L.p), shape=(rows, rows))
    P = sp.csr_matrix((np.ones(rows), (np.arange(rows), L.agg)), shape=(rows, na))
    G = (P.T @ A @ P).tocsr()
    G.sort_indices()
    assert G.nnz == co.nnz_c and np.array_equal(G.indptr, co.row_ptr) and np.array_equal(G.indices, co.column)
    crow = np.repeat(np.arange(na), np.diff(co.row_ptr))
    assert np.all((np.diff(co.column) > 0) | (np.diff(crow) > 0)), "the columns of every coarse row are distinct and ascending"
    # (b) the values: the fine values grouped by (agg[row], agg[column]) through a lexicographic sort of the two numbers -- no
    # combined key -- and added in long doubles (64 bits of mantissa: their own error is run 2^-64 sum |t|, 2^-11 of the bound)
    frow = np.repeat(np.arange(rows), np.diff(L.p.astype(np.int64)))
    ar, acol = L.agg[frow], L.agg[L.c]
    order = np.lexsort((acol, ar))
    head = np.ones(len(order), dtype=bool)
    head[1:] = (ar[order][1:] != ar[order][:-1]) | (acol[order][1:] != acol[order][:-1])
    at = np.flatnonzero(head)
    assert np.array_equal(ar[order][at], crow) and np.array_equal(acol[order][at], co.column)
    assert np.finfo(np.longdouble).nmant >= 63, "long doubles of 64 bits of mantissa"
    near_exact = np.add.reduceat(L.v.astype(np.longdouble)[order], at)
    bound = co.bound(L.v)
    assert np.array_equal(np.diff(np.concatenate([at, [len(order)]])), np.diff(co.entry_ptr)) and np.all(bound > 0.0)
    off = np.abs(L.cv.astype(np.longdouble) - near_exact).astype(np.float64)
    print("level %d: %d rows -> %d aggregates, %d coarse entries, the longest run %d; the restated values within %.3f of the bound of the long-double "
          "sums" % (level, rows, na, co.nnz_c, L.longest, float(np.max(off / bound))))
    assert np.all(off <= bound)
    # (c) scipy's own fp64 triple product: two independent orders of one sum, twice the bound
    off2 = np.abs(L.cv - G.data)
    print("level %d: within %.3f of the single bound of scipy's product (asserted: 2)" % (level, float(np.max(off2 / bound))))
    assert np.all(off2 <= 2.0 * bound)


def test_the_general_values_of_the_edge_plans_sum_within_the_bound():
    for name in gs.BLOCKS:
        co, g = gs.coarse(name), gs.general_values(name)
        near_exact = np.add.reduceat(g.astype(np.longdouble)[co.order], co.entry_ptr[:-1].astype(np.int64))
        assert np.all(np.abs(gs.coarse_values(name).astype(np.longdouble) - near_exact).astype(np.float64) <= co.bound(g))
