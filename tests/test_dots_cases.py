"""What must hold of the operands of test_gpu_dots.py before a GPU result is looked at (dots_cases.py), without a device: the
exact operands keep every y_out below 2^24 and both sums of magnitudes below 2^53 through three chained calls, in Python
integers; and on the general operands a lost or doubled row would show -- in all but 1 % of the rows with entries |t_i| exceeds
ten times the bound rows 2^-53 sum |t_i| that the GPU's dots are held to."""
import numpy as np
import pytest

import dots_cases as dc
from test_gpu_scaled import MATRICES, PAIRS


@pytest.mark.parametrize("name", MATRICES)
def test_exact_operands_stay_exact_through_three_chained_calls(name):
    h = dc.int_host(name)
    assert np.all(h.v == h.a32) and np.all(h.x == h.x32) and np.all(h.y0 == h.y0_32) and np.all(h.w == h.w32)  # floats hold them
    if len(h.vi):
        assert np.all(h.vi != 0)
    for alpha, beta in dc.INT_PAIRS:
        assert alpha in (1, -1, 2, 0) and beta in (1, -1, 2, 0)
        for which in ("null", "own") + (("x",) if h.rows == h.cols else ()):
            steps = h.chain(alpha, beta, which)  # (asserts the precondition)
            assert len(steps) == dc.CALLS
            if which == "null":
                assert all(s[2] == 0 for s in steps)
    # the sums are not all trivially zero: the row sums reach the dots
    if h.rows and len(h.vi):
        assert h.chain(1, 0, "own")[0][1] > 0


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("name", MATRICES)
def test_a_lost_row_would_show_on_the_general_operands(name, kind):
    for alpha, beta in PAIRS:
        shares = dc.visible(name, kind, alpha, beta)
        print("%s, %s, alpha %g, beta %g: share of rows with entries within 10 x the bound, per dot: %s" % (name, kind, alpha, beta, shares))
        if alpha == 0.0 and beta == 0.0:
            assert all(s is None for s in shares)  # y_out is +0.0: both dots are +0.0 exactly
        for s in shares:
            assert s is None or s <= 0.01, (name, kind, alpha, beta, shares)


def test_the_bound_is_the_a_priori_one():
    t = np.array([1.0, -2.0, 0.5])
    assert dc.bound(t) == 3 * 2.0 ** -53 * 3.5
