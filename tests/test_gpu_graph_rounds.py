"""The counters of the rounds of graph_rounds.hpp at the edges of a wave and of a workgroup: paths of 63, 64, 65, 256 and 257 rows
through spmv_hip_agg_aggregate and spmv_hip_agg_aggregate_mis2 at both seeds and both thetas, and the paths of 256 and 257 rows
through spmv_hip_mcgs_colour (63, 64 and 65 are among mcgs_cases.COLOURING already).  A round's winners or decided rows are
counted once per wave, by a lane of the wave that is still there: in the last wave of these sizes the lanes behind the last row
have returned, or hold no row.  A miscount shows in the rounds of the status, or ends the call with a state error.  The
aggregates, the colours and all four status words are held to the numpy restatements (agg_cases, agg_mis2_cases, mcgs_cases) with
exact equality; the first test holds the restatements themselves to these sizes without a device -- their `assert win.any()`
is every round deciding a row."""
import functools

import numpy as np
import pytest

import agg_cases as ac
import agg_mis2_cases as a2
import mcgs_cases as mc
from test_gpu_agg_mis2 import Level2
from test_gpu_mcgs import Matrix

SIZES = (63, 64, 65, 256, 257)
COLOURED = (256, 257)


@functools.lru_cache(maxsize=None)
def _want(what, rows, theta, seed):
    n, p, c, v = mc.path(rows)
    if what == "colour":
        return mc.colour(n, p, c, seed)
    return (ac if what == "distance 1" else a2).aggregate(n, p, c, v, theta, seed)


def test_the_restatements_run_these_sizes_and_every_round_decides_a_row():
    for rows in SIZES:
        for seed in ac.SEEDS:
            for theta in ac.THETAS:
                for what in ("distance 1", "distance 2"):
                    agg, status = _want(what, rows, theta, seed)
                    assert 1 <= status[1] <= rows and status[0] == agg.max() + 1 and len(agg) == rows, (what, rows, theta, seed)
            colour, status = _want("colour", rows, 0.0, seed)
            assert 1 <= status[1] <= rows and status[0] == colour.max() + 1 and status[2:] == [0, 0], (rows, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", SIZES)
def test_both_aggregations_of_a_path_are_the_restatement_at_both_seeds_and_thetas(rows):
    m = Level2(*mc.path(rows))
    for seed in ac.SEEDS:
        for theta in ac.THETAS:
            for what, run in (("distance 1", m.aggregate), ("distance 2", m.aggregate_mis2)):
                want, status = _want(what, rows, theta, seed)
                got, got_status = run(seed, theta)
                print("path_%d, %s, seed %#x, theta %.2f: status %s" % (rows, what, seed, theta, got_status))
                assert got_status == status, (what, seed, theta)
                assert np.array_equal(got, want), (what, seed, theta)
    m.unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("rows", COLOURED)
def test_the_colours_of_a_path_are_the_restatement_at_both_seeds(rows):
    n, p, c, v = mc.path(rows)
    for seed in mc.SEEDS:
        want, status = _want("colour", rows, 0.0, seed)
        m = Matrix(n, p, c, v, seed)
        print("path_%d, seed %#x: status %s" % (rows, seed, m.status_h[:4].tolist()))
        assert m.status_h[:4].tolist() == status
        assert np.array_equal(m.colour_h[:n], want)
        m.unchanged()
