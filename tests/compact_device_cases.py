"""Small matrices for the places where the kernels that plan the compact multiply on the device (c16_plan_kernels.hpp) can go wrong
and the matrices of compact_cases.py do not reach: what test_compact_device_cases.py (no GPU: each case does what its name says,
by the preview) and test_gpu_compact_device.py share."""
import functools

import numpy as np

import compact_cases as cc

SPAN = cc.SPAN
HIGH_COLS = 2 ** 31 - 1


def _unsorted_repeats():
    """300 rows of 11 columns drawn WITH replacement from 40 000 (five windows) in no order, a column repeated inside every row and
    the smallest column of the matrix in the last place of its tile."""
    rng = np.random.default_rng(23)
    rows = [rng.integers(7, 40000, size=11) for _ in range(300)]
    for r in rows:
        r[rng.integers(1, 10)] = r[0]
    rows[63][10] = 3
    return cc.from_rows(rows, 40000)


def _tile_starts():
    """Four tiles of 64 rows; the first three hold 193 entries each, so the later ones start at entry 193, 386 and 579: k0 % 4 =
    1, 2, 3.  Every tile's columns lie in two windows."""
    rng = np.random.default_rng(24)
    lens = [3] * 63 + [4]
    rows = []
    for t in range(4):
        rows += [np.sort(rng.choice(2 * SPAN, size=n if t < 3 else 3, replace=False)) + 50 * t for n in lens]
    return cc.from_rows(rows, 2 * SPAN + 200)


def _empty_run():
    """64 rows of entries, 70 rows without, 30 rows of entries: the second tile is 64 rows without an entry."""
    rng = np.random.default_rng(25)
    return cc.from_lengths([5] * 64 + [0] * 70 + [4] * 30, 3000, 26, lambda r, n: rng.choice(3000, size=n, replace=False))


def _window_edge():
    """One tile with a column at exactly base + 8191 (the last offset of window 0) and one at base + 8192 (the base of window 1)."""
    return cc.from_rows([[100 + SPAN, 100, 100 + SPAN - 1], [100 + SPAN - 1, 101]], 100 + SPAN + 1)


def _long_row(cols, seed):
    """Short rows around one row of 1500 distinct columns out of `cols`, in no order."""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(cols, size=3, replace=False)) for _ in range(10)]
    rows.insert(5, rng.permutation(rng.choice(cols, size=1500, replace=False)))
    return cc.from_rows(rows, cols)


def _high_columns():
    """cols = 2^31 - 1; base[1] + 8192 = 2^31 - 2 is the last column there is, and base[2] + 8192 is no int32."""
    return cc.from_rows([[0, HIGH_COLS - SPAN - 1], [HIGH_COLS - SPAN], [HIGH_COLS - 1]], HIGH_COLS)


CASES = {
    "unsorted_repeats": _unsorted_repeats,
    "tile_starts_1_2_3": _tile_starts,
    "empty_run_70": _empty_run,
    "window_edge": _window_edge,
    "long_row_1500_three_windows": lambda: _long_row(3 * SPAN - 500, 27),
    "long_row_1500_nine_windows": lambda: _long_row(9 * SPAN - 300, 28),
    "high_columns": _high_columns,
}
NAMES = sorted(CASES)
NO_X = ("high_columns",)  # plan, table and verify only: no vector of 2^31 - 1 elements


@functools.lru_cache(maxsize=None)
def matrix(name):
    return CASES[name]()


def three_tiles():
    """192 rows of three entries: three tiles, for the refusals."""
    return cc.from_lengths([3] * 192, 500, 29)
