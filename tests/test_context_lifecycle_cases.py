"""The preconditions of test_gpu_context_lifecycle.py that need no device: the pair table covers all hundred ordered pairs of
formats, consecutive uploads never share rows, cols or stored entries (a stale size cannot coincide with a correct one), and
every pool matrix passes the host-side checks of the formats it is given to."""
import itertools

import numpy as np
import pytest

import lifecycle_cases as lc


def test_any_two_pool_matrices_differ_in_rows_cols_and_entries():
    for m, n in itertools.combinations(lc.POOL + (lc.TINY, lc.HOLLOW), 2):
        for fm, fn in ((1, 1), (6, 1), (1, 6), (6, 6)):  # as stored, or as the transposed operator of format 6
            assert lc.differ(lc.operator_shape(fm, m), lc.operator_shape(fn, n)), (m, n, fm, fn)
    assert all(int(lc.matrix(n)[2][-1]) < 3_000_000 for n in lc.GENERATORS)
    assert lc.matrix("no_entries")[0] == 50 and len(lc.matrix("no_entries")[3]) == 0


def test_the_pair_table_covers_all_hundred_ordered_pairs_with_changing_shapes():
    assert set(lc.PAIRS) == set(itertools.product(lc.FORMATS, lc.FORMATS)) and len(lc.PAIRS) == 100
    met = set()
    for (a, b), ((fa, ma), (fb, mb)) in lc.PAIRS.items():
        assert (fa, fb) == (a, b) and ma in lc.ACCEPTS[a] and mb in lc.ACCEPTS[b]
        assert lc.differ(lc.operator_shape(a, ma), lc.operator_shape(b, mb)), (a, ma, b, mb)
        met.update((ma, mb))
    assert met == set(lc.POOL)


def test_the_multi_gpu_pairs_cover_sixteen_and_cross_the_number_of_parts():
    assert set(lc.MULTI_PAIRS) == set(itertools.product(lc.MULTI_FORMATS, lc.MULTI_FORMATS))
    down = up = False
    for (a, b), ((fa, ma), (fb, mb)) in lc.MULTI_PAIRS.items():
        assert (fa, fb) == (a, b)
        assert lc.differ(lc.operator_shape(a, ma), lc.operator_shape(b, mb)), (a, ma, b, mb)
        down |= lc.matrix(ma)[0] > 3 > lc.matrix(mb)[0]
        up |= lc.matrix(ma)[0] < 3 < lc.matrix(mb)[0]
    assert down and up


def test_the_walk_visits_every_format_four_times_and_never_repeats_a_shape():
    w = lc.walk()
    assert len(w) == 60 and w == lc.walk()  # seeded
    for fmt in lc.FORMATS:
        assert sum(1 for f, _ in w if f == fmt) >= 4
    for (fa, ma), (fb, mb) in zip(w, w[1:]):
        assert ma in lc.ACCEPTS[fa] and lc.differ(lc.operator_shape(fa, ma), lc.operator_shape(fb, mb)), (fa, ma, fb, mb)
    assert any(m == lc.SCATTERED for _, m in w)


def test_the_reproducible_set_is_what_the_headers_guarantee():
    for fmt in (1, 3, 7, 8, 9, 10):
        for name in lc.ACCEPTS[fmt]:
            assert ((fmt, name) in lc.REPRODUCIBLE) == (name != lc.SCATTERED)
    for fmt, name in itertools.chain.from_iterable((((f, n) for n in lc.ACCEPTS[f]) for f in lc.FORMATS)):
        if (fmt, name) not in lc.REPRODUCIBLE:  # only these may fall back to the tolerance
            assert fmt in (5, 6) or name == lc.SCATTERED
    # "rows summed by their owners" without atomics holds for rows of up to 512 entries: no pool matrix has a longer one
    assert all(int(np.diff(lc.matrix(n)[2]).max()) <= 512 for n in lc.GENERATORS)


@pytest.mark.parametrize("fmt", lc.FORMATS)
def test_every_pool_matrix_passes_the_host_side_checks_of_its_formats(fmt):
    for name in lc.ACCEPTS[fmt] + ((lc.TINY,) if fmt in lc.MULTI_FORMATS else ()):
        lc.host_check(fmt, name)
