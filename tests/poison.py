"""Non-finite operands for test_gpu_nonfinite.py: where NaN and Inf go in x, in the stored values and in y0, what the CPU
reference must show before a GPU result is looked at, and how two results are compared.  The reference forms exactly the products
a row stores, and no stored value is zero, so the class of every y_i -- NaN, +Inf, -Inf or finite -- follows from the sparsity
pattern alone, whatever the order of the sum: classes are compared exactly, finite rows bitwise or within helpers.assert_close."""
import numpy as np

import helpers

FINITE, NAN, PINF, NINF = 0, 1, 2, 3
VALUE_ROW_STRIDE = 37  # every 37th non-empty row gets its first and last stored entry poisoned
Y0_ROW_STRIDE = 29     # every 29th row of y0 is non-finite
Y_GUARD_BITS = 0xC01D000000000000 | 0x5EED  # -7.25 with a marked mantissa: one fixed pattern, finite, never a result


def mean_row_length(row_ptr):
    lens = np.diff(np.asarray(row_ptr, dtype=np.int64))
    return float(lens.sum()) / max(1, int((lens > 0).sum()))


def columns(cols, m, seed):
    """The poison rule: every column with probability min(0.25, 0.3 / m), plus column 0 and column cols - 1 (what a clamped
    gather reads); returns (the first half in index order: NaN, the second half: +Inf)."""
    f = min(0.25, 0.3 / max(m, 1e-9))
    pick = np.random.default_rng(seed).random(cols) < f
    pick[0] = pick[cols - 1] = True
    P = np.nonzero(pick)[0]
    return P[:len(P) // 2], P[len(P) // 2:]


def x_vector(x, row_ptr, seed=1234):
    """x with the poison rule applied for a matrix whose rows are row_ptr's (x keeps its dtype: float NaN / Inf for a float x)."""
    nan, inf = columns(len(x), mean_row_length(row_ptr), seed)
    out = np.array(x, copy=True)
    assert np.all(out != 0)
    out[nan] = np.nan
    out[inf] = np.inf
    return out


def values(row_ptr, val):
    """The first (NaN) and the last (+Inf) stored entry of every 37th non-empty row: the entries that share a quad with the
    neighbouring row or tile.  A row of one entry gets +Inf.  Returns (the poisoned copy, the rows that were hit)."""
    p = np.asarray(row_ptr, dtype=np.int64)
    rows = np.nonzero(np.diff(p) > 0)[0][::VALUE_ROW_STRIDE]
    out = np.array(val, copy=True)
    assert np.all(out != 0)
    out[p[rows]] = np.nan
    out[p[rows + 1] - 1] = np.inf
    return out, rows


def y0_vector(y0):
    """Every 29th row non-finite: NaN, +Inf, -Inf in turn."""
    out = np.array(y0, copy=True)
    hit = np.arange(0, len(out), Y0_ROW_STRIDE)
    out[hit[0::3]] = np.nan
    out[hit[1::3]] = np.inf
    out[hit[2::3]] = -np.inf
    return out


def classes(y):
    y = np.asarray(y)
    c = np.zeros(y.shape, dtype=np.int8)
    c[np.isnan(y)] = NAN
    c[np.isposinf(y)] = PINF
    c[np.isneginf(y)] = NINF
    return c


def shares(y_ref):
    """(non-finite, finite, finite with a non-finite neighbour row r - 1 or r + 1) as shares of the rows."""
    bad = classes(y_ref) != FINITE
    near = np.zeros_like(bad)
    near[1:] |= bad[:-1]
    near[:-1] |= bad[1:]
    n = max(1, bad.size)
    return bad.sum() / n, (~bad).sum() / n, (~bad & near).sum() / n


def assert_not_vacuous(y_ref, what):
    """From the reference's result alone: enough rows of every kind that a kernel using what it must not, or skipping what it
    must use, cannot pass."""
    bad, fin, near = shares(y_ref)
    print("%s: reference rows %.1f %% non-finite, %.1f %% finite, %.1f %% finite beside a non-finite row" % (
        what, 100 * bad, 100 * fin, 100 * near))
    assert bad >= 0.05, "%s: only %.2f %% of the reference's rows are non-finite" % (what, 100 * bad)
    assert fin >= 0.50, "%s: only %.2f %% of the reference's rows are finite" % (what, 100 * fin)
    assert near >= 0.05, "%s: only %.2f %% finite rows beside a non-finite one" % (what, 100 * near)


def assert_classes(got, ref, what):
    """isnan, and isinf with its sign, row by row."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    cg, cr = classes(got), classes(ref)
    off = np.nonzero((cg != cr).ravel())[0]
    if off.size:
        names = ["finite", "NaN", "+Inf", "-Inf"]
        k = int(off[0])
        made = int(((cg != FINITE) & (cr == FINITE)).sum())
        lost = int(((cg == FINITE) & (cr != FINITE)).sum())
        raise AssertionError("%s: %d of %d rows in another class than the reference's (%d finite rows made non-finite, %d "
                             "non-finite rows made finite), first row %d: %s, reference %s" % (
                                 what, off.size, cr.size, made, lost, k, names[cg.ravel()[k]], names[cr.ravel()[k]]))


def assert_finite_rows_bitwise(got, clean, ref, what, only=None):
    """The rows the reference keeps finite hold the same products as in the clean run: the same bits.  `only`: a mask of the
    rows this is claimed for (the others' partial sums meet in atomics)."""
    got, clean = np.ascontiguousarray(got), np.ascontiguousarray(clean, dtype=np.asarray(got).dtype)
    assert got.shape == clean.shape, what
    keep = (classes(ref) == FINITE).ravel()
    if only is not None:
        keep &= np.asarray(only, dtype=bool).ravel()
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    a, b = got.ravel().view(u)[keep], clean.ravel().view(u)[keep]
    if not np.array_equal(a, b):
        k = int(np.nonzero(keep)[0][np.nonzero(a != b)[0][0]])
        raise AssertionError("%s: %d of %d finite rows differ bitwise from the clean run, first row %d: %r vs %r" % (
            what, int((a != b).sum()), int(keep.sum()), k, got.ravel()[k], clean.ravel()[k]))


def assert_finite_rows_close(got, ref, scale, what, nterms=4096):
    """Where partial sums meet in atomics: the finite rows within the project's tolerance of the reference."""
    keep = classes(ref) == FINITE
    helpers.assert_close(np.asarray(got)[keep], np.asarray(ref)[keep], np.asarray(scale)[keep], what=what, nterms=nterms)
