"""Each matrix of compact_device_cases.py does what its name says, by spmv_hip_c16_plan_preview and the recount of
compact_cases.py, under both flags; no GPU.  (That the C16Plan they are made for has its device entry points is asserted too: these
cases exist for C16Plan.from_device.)"""
import numpy as np
import pytest

import compact_cases as cc
import compact_device_cases as dc
from spmv_amd import capi

FLAGS = [0, capi.FLAG_EXACT_ORDER]


def _preview(name, flags):
    rows, cols, p, c, _ = dc.matrix(name)
    info, tab, codes = capi.c16_plan_preview(rows, cols, p, c, flags, codes=True)
    cc.recount(rows, cols, p, c, flags, info, tab, codes)
    return (rows, cols, p, c), info, tab, codes


def test_the_entry_points_these_cases_are_for_exist():
    assert callable(capi.C16Plan.from_device) and callable(capi.C16Plan.table)


@pytest.mark.parametrize("flags", FLAGS)
def test_unsorted_repeats(flags):
    (rows, cols, p, c), info, tab, codes = _preview("unsorted_repeats", flags)
    per_row = c.reshape(rows, 11)
    assert np.all(np.any(np.diff(per_row, axis=1) < 0, axis=1)), "every row is out of order"
    assert all(len(set(r.tolist())) < 11 for r in per_row), "every row repeats a column"
    assert info["wide_tiles"] == 0 and info["tiles_with_5_windows"] > 0
    w = int(np.nonzero(tab[:, 0] <= 63)[0][-1])
    assert tab[w, 5] == 3 and c[p[63] + 10] == 3, "the first base is found in the tile's last entry"


@pytest.mark.parametrize("flags", FLAGS)
def test_tile_starts(flags):
    _, info, tab, _ = _preview("tile_starts_1_2_3", flags)
    assert tab[:, 1].tolist() == [0, 193, 386, 579] and (tab[:, 1] % 4).tolist() == [0, 1, 2, 3]
    assert np.all(tab[:, 4] == 2) and info["compact_tiles"] == 4


@pytest.mark.parametrize("flags", FLAGS)
def test_empty_run(flags):
    (rows, cols, p, c), info, tab, _ = _preview("empty_run_70", flags)
    assert np.all(np.diff(p)[64:134] == 0) and np.diff(p)[63] > 0 and np.diff(p)[134] > 0
    assert tab[1, :5].tolist()[:3] == [64, 320, 64] and tab[2, 1] == 320, "the second tile has no entry"
    assert tab[1, 4] == 1 and not np.any(tab[1, 5:]), "... and counts as compact with one window and bases 0"


@pytest.mark.parametrize("flags", FLAGS)
def test_window_edge(flags):
    _, info, tab, codes = _preview("window_edge", flags)
    assert info["tiles"] == 1 and tab[0, 4] == 2 and tab[0, 5:].tolist() == [100, 100 + dc.SPAN] + [100 + dc.SPAN] * 6
    assert codes.tolist() == [1 << 13, 0, 8191, 8191, 1]


@pytest.mark.parametrize("flags", FLAGS)
def test_long_rows(flags):
    (rows, cols, p, c), info, tab, _ = _preview("long_row_1500_three_windows", flags)
    w = int(np.nonzero(tab[:, 0] == 5)[0][0])
    assert info["long_row_tiles"] == 1 and tab[w, 2] == 1 and tab[w, 4] == 3 and p[6] - p[5] == 1500
    assert np.any(np.diff(c[p[5]:p[6]]) < 0)
    (rows, cols, p, c), info, tab, _ = _preview("long_row_1500_nine_windows", flags)
    w = int(np.nonzero(tab[:, 0] == 5)[0][0])
    assert info["long_row_tiles"] == 1 and tab[w, 2] == 1 and tab[w, 4] == 0 and info["wide_tiles"] == 1
    assert cc.greedy_bases(c[p[5]:p[6]])[0] == 9, "exactly nine windows: the ninth minimum decides"


@pytest.mark.parametrize("flags", FLAGS)
def test_high_columns(flags):
    (rows, cols, p, c), info, tab, codes = _preview("high_columns", flags)
    assert cols == 2 ** 31 - 1 and rows == 3 and c.tolist() == [0, 2 ** 31 - 8194, 2 ** 31 - 8193, 2 ** 31 - 2]
    assert info["tiles"] == 1 and tab[0, 4] == 3
    assert tab[0, 5:].tolist() == [0, 2 ** 31 - 8194] + [2 ** 31 - 2] * 6
    assert codes.tolist() == [0, 1 << 13, (1 << 13) | 1, 2 << 13]


def test_three_tiles():
    rows, cols, p, c, _ = dc.three_tiles()
    info = capi.c16_plan_preview(rows, cols, p, c, 0, table=False)[0]
    assert info["tiles"] == 3 and info["stored_entries"] == 576
