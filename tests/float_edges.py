"""Float x and y at the edges of the float format, for test_gpu_compact32.py (y <- fl32(y + fl32(A) x)) and test_gpu_scaled.py
(y_out <- fl32(alpha fl32(A) x + beta y_in)): one matrix whose stored values and x are non-zero small integers, so that every row
sum n_i is the same exact integer in ANY summation order, and operand sets that put the one rounding to float of a row on a tie,
at FLT_MAX and in the denormals.  Every t_i below is exact in fp64, so both orders must give, bit for bit, t.astype(float32):
numpy's cast rounds to nearest even, into the denormals and to +-Inf at the tie above FLT_MAX (self_check).  Everything here is
numpy: the row-kind census runs without a device, before a GPU result is looked at."""
import functools

import numpy as np

import compact_cases as cc

FLT_MAX = float(np.finfo(np.float32).max)  # 2^128 - 2^104
DEN = 2.0 ** -149                          # the smallest float denormal


def f32(a):
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


def self_check():
    """The restatement's own rounding, on known cases."""
    want = {1 * 2.0 ** -150: 0.0, 3 * 2.0 ** -150: 2 * DEN, 5 * 2.0 ** -150: 2 * DEN, 7 * 2.0 ** -150: 4 * DEN,
            1.0 + 2.0 ** -24: 1.0, 1.0 + 3 * 2.0 ** -24: 1.0 + 2.0 ** -22, FLT_MAX + 2.0 ** 102: FLT_MAX, FLT_MAX + 2.0 ** 103: np.inf,
            -FLT_MAX - 2.0 ** 103: -np.inf}
    for t, r in want.items():
        assert float(f32([t])[0]) == r, (t, r)
    assert np.signbit(f32([-2.0 ** -150])[0]) and f32([-2.0 ** -150])[0] == 0.0
    assert float(np.float32(DEN)) == DEN and float(np.float32(DEN)) > 0.0  # (no flush on the host)


class Edges:
    """About 3000 rows of 0 to 7 entries, one row of 9000 entries within three windows (a compact long row), and a last row that
    leaves nnz % 4 != 0: dense_row_9000_compact with the ragged end of rows_0_to_7_ragged_end.  Values in +-1...3, x in +-1...4."""

    name = "float_edges"

    def __init__(self):
        rng = np.random.default_rng(41)
        lens = rng.integers(0, 8, size=3001)
        lens[1717] = 9000
        lens[-1] = 5
        if int(lens.sum()) % 4 == 0:
            lens[-1] = 6
        cols = 20000
        pick = lambda r, n: r.choice(min(cols, 3 * cc.SPAN) if n > 100 else cols, size=n, replace=False)
        self.rows, self.cols, self.p, self.c, _ = cc.from_lengths(lens, cols, 42, pick)
        nnz = len(self.c)
        assert nnz % 4 != 0 and self.rows == 3001
        self.a32 = (rng.integers(1, 4, size=nnz) * rng.choice([-1, 1], size=nnz)).astype(np.float32)
        self.x32 = (rng.integers(1, 5, size=cols) * rng.choice([-1, 1], size=cols)).astype(np.float32)
        self.v = self.a32.astype(np.float64)
        self.lens = np.diff(self.p.astype(np.int64))
        r = np.repeat(np.arange(self.rows), self.lens)
        self.n = np.bincount(r, weights=self.v * self.x32.astype(np.float64)[self.c], minlength=self.rows)  # exact: integers
        assert np.all(self.n == np.rint(self.n)) and np.max(np.abs(self.n)) < 2 ** 20 and np.all(self.a32 != 0) and np.all(self.x32 != 0)
        self.x_den = (self.x32.astype(np.float64) * DEN).astype(np.float32)  # float denormals, exact
        assert np.array_equal(self.x_den.astype(np.float64), self.x32.astype(np.float64) * DEN)
        self.k_den = ((np.arange(self.rows) % 4) * DEN).astype(np.float32)    # k 2^-149, k in 0...3

    # what test_gpu_scaled.Dev asks of a host matrix
    def values(self, kind):
        return self.a32

    def vectors(self, kind):
        return self.x32, np.zeros(self.rows, dtype=np.float32), np.float32

    def calls(self):
        """{name: (alpha, beta, x, y_in or None, t)}: the four scaled calls, t the exact fp64 result before its one rounding."""
        n, i = self.n, np.arange(self.rows)
        ties = np.array([1.0, 1.0 + 2.0 ** -23, 3.0, -1.0], dtype=np.float32)[i % 4]
        # +-FLT_MAX: the sign of n_i (it may overflow) in two rows of three, the other sign (it stays finite) in the third
        sign = np.where(n < 0, -1.0, 1.0) * np.where(i % 3 == 0, -1.0, 1.0)
        big = (sign * FLT_MAX).astype(np.float32)
        out = {"ties": (2.0 ** -24, 1.0, self.x32, ties, 2.0 ** -24 * n + ties.astype(np.float64)),
               "overflow": (2.0 ** 102, 1.0, self.x32, big, 2.0 ** 102 * n + big.astype(np.float64)),
               "denormal results": (2.0 ** -150, 1.0, self.x32, self.k_den, 2.0 ** -150 * n + self.k_den.astype(np.float64)),
               "denormal x": (2.0 ** 149, 0.0, self.x_den, None, n.copy())}
        for name, (alpha, beta, x, y_in, t) in out.items():  # every t is exact: an integer multiple of a power of two, < 2^53 of them
            unit = {"ties": 2.0 ** -24, "overflow": 2.0 ** 102, "denormal results": 2.0 ** -150, "denormal x": 1.0}[name]
            m = t / unit
            assert np.all(m == np.rint(m)) and np.max(np.abs(m)) < 2.0 ** 53, name
        return out

    def census(self):
        """From the restatement alone: every targeted kind of row occurs.  Returns the counts."""
        self_check()
        calls = self.calls()
        n, i = self.n, np.arange(self.rows)
        count = {}

        def rounded(t):
            r = f32(t).astype(np.float64)
            with np.errstate(over="ignore", invalid="ignore"):
                other = np.nextafter(f32(t), np.where(t > r, np.inf, -np.inf).astype(np.float32)).astype(np.float64)
                tie = (t != r) & np.isfinite(r) & (np.abs(t - r) == np.abs(other - t))
            return r, tie

        t = calls["ties"][4]
        r, tie = rounded(t)
        y = calls["ties"][3].astype(np.float64)
        count["ties rounded towards zero"] = int((tie & (np.abs(r) < np.abs(t))).sum())
        count["ties rounded away from zero"] = int((tie & (np.abs(r) > np.abs(t))).sum())
        count["n = 1 on 1.0 gives 1.0"] = int(((n == 1) & (y == 1.0) & (r == 1.0)).sum())
        count["n = 1 on 1 + 2^-23 gives 1 + 2^-22"] = int(((n == 1) & (y == 1.0 + 2.0 ** -23) & (r == 1.0 + 2.0 ** -22)).sum())
        count["n = 3 on 1.0 gives 1 + 2^-22"] = int(((n == 3) & (y == 1.0) & (r == 1.0 + 2.0 ** -22)).sum())
        t = calls["overflow"][4]
        r, _ = rounded(t)
        y = calls["overflow"][3].astype(np.float64)
        same = np.sign(y) == np.where(n < 0, -1.0, 1.0)
        count["+FLT_MAX, n = 2: the tie gives +Inf"] = int(((n == 2) & (y > 0) & np.isposinf(r)).sum())
        count["-FLT_MAX, n = -2: the tie gives -Inf"] = int(((n == -2) & (y < 0) & np.isneginf(r)).sum())
        count["|n| = 1 stays FLT_MAX"] = int(((np.abs(n) == 1) & same & (np.abs(r) == FLT_MAX)).sum())
        count["|n| >= 3 overflows"] = int(((np.abs(n) >= 3) & same & np.isinf(r)).sum())
        count["n of the other sign stays finite"] = int(((n != 0) & ~same & np.isfinite(r)).sum())
        assert not np.any(~same & ~np.isfinite(r))
        t = calls["denormal results"][4]
        r, tie = rounded(t)
        m = t / 2.0 ** -150
        count["denormal results"] = int(((r != 0) & (np.abs(r) < 2.0 ** -126)).sum())
        count["1 2^-150 gives +0"] = int(((m == 1) & (r == 0) & ~np.signbit(r)).sum())
        count["3 2^-150 gives 2 2^-149"] = int(((m == 3) & (r == 2 * DEN)).sum())
        count["5 2^-150 gives 2 2^-149"] = int(((m == 5) & (r == 2 * DEN)).sum())
        count["negative t gives -0.0"] = int(((t < 0) & (r == 0) & np.signbit(r)).sum())
        count["denormal ties"] = int(tie.sum())
        count["rows without entries"] = int((self.lens == 0).sum())
        count["denormal x: non-zero n"] = int((n != 0).sum())
        for what, k in count.items():
            assert k > 0, "float_edges: no row of the kind '%s'" % what
        return count


@functools.lru_cache(maxsize=1)
def edges():
    return Edges()
