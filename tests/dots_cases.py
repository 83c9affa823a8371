"""Operands for the tests of the scaled multiplies with dots (include/spmv_hip_dots.h), and what must hold of them before a GPU
result is looked at (test_dots_cases.py asserts it without a device; test_gpu_dots.py uses the same operands).

EXACT operands (IntHost): values, x, y_in and w are small integers and alpha, beta come from {1, -1, 2, 0}, so every row sum,
every y_out and every product of the dots is an integer that fp64 (and, below 2^24, float) holds exactly, whatever the order:
both dots must equal the integer sums bit for bit.  chain() computes them in integers and asserts the precondition.

GENERAL operands (test_gpu_scaled.Host's, and general_w): the dots are held to rows 2^-53 sum |t_i| of math.fsum(t), t_i the
rounded products of the y_out the GPU returned.  visible() asserts, from the restatement of y_out, that a lost or doubled row
would move a sum by more than ten times that bound in all but 1 % of the rows with entries."""
import functools

import numpy as np

import compact_cases as cc
from test_gpu_scaled import host, restate

INT_PAIRS = [(1, 0), (-1, 1), (2, -1), (0, 2), (0, 0), (1, 1)]
CALLS = 3
KINDS = ("f32", "c16", "c16_f64", "c16_f32xy")


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


class IntHost:
    """The pattern of compact_cases.matrix(name) with integer values in +-{1, 2, 3}, x in [-4, 4], y0 and w in [-8, 8]; the
    interface of test_gpu_scaled.Host that its Dev reads."""

    def __init__(self, name):
        self.name, self._chains = name, {}
        self.rows, self.cols, self.p, self.c, v = cc.matrix(name)
        rng = np.random.default_rng(len(name) + 5)
        self.vi = rng.integers(1, 4, size=len(v)) * rng.choice([-1, 1], size=len(v))
        self.xi = rng.integers(-4, 5, size=self.cols)
        self.yi = rng.integers(-8, 9, size=self.rows)
        self.wi = rng.integers(-8, 9, size=self.rows)
        self.v, self.x, self.y0, self.w = (a.astype(np.float64) for a in (self.vi, self.xi, self.yi, self.wi))
        self.a32, self.x32, self.y0_32, self.w32 = _f32(self.v), _f32(self.x), _f32(self.y0), _f32(self.w)
        row = np.repeat(np.arange(self.rows, dtype=np.int64), np.diff(self.p.astype(np.int64)))
        self.zi = np.zeros(self.rows, dtype=np.int64)
        if len(v):
            np.add.at(self.zi, row, self.vi.astype(np.int64) * self.xi.astype(np.int64)[self.c])

    def values(self, kind):
        return self.v if kind == "c16_f64" else self.a32

    def vectors(self, kind):
        return (self.x32, self.y0_32, np.float32) if kind == "c16_f32xy" else (self.x, self.y0, np.float64)

    def w_for(self, kind, which):
        """(host array or None, integers) of w: "null", "x" (square matrices) or "own"."""
        if which == "null":
            return None, np.zeros(self.rows, dtype=np.int64)
        wi = self.xi if which == "x" else self.wi
        return wi.astype(np.float32 if kind == "c16_f32xy" else np.float64), wi.astype(np.int64)

    def chain(self, alpha, beta, which, calls=CALLS):
        """[(y, sum y^2, sum w y)] after each of `calls` chained calls y <- alpha z + beta y from y0 with w "null", "x" or "own",
        in Python integers, with the precondition asserted: every |y_i| < 2^24 (a float holds it), both sums of magnitudes
        < 2^53 (any order is exact)."""
        key = (alpha, beta, which, calls)
        if key not in self._chains:
            out, y = [], self.yi.astype(np.int64)
            w = self.w_for("c16", which)[1].tolist()
            for _ in range(calls):
                y = int(alpha) * self.zi + int(beta) * y  # (int64: |y| stays far below 2^63, and is asserted below 2^24)
                yl = y.tolist()
                assert all(abs(v) < 2 ** 24 for v in yl), self.name
                yy, wy = sum(v * v for v in yl), sum(a * v for a, v in zip(w, yl))
                assert yy < 2 ** 53 and sum(abs(a * v) for a, v in zip(w, yl)) < 2 ** 53, self.name
                out.append((y.copy(), yy, wy))
            self._chains[key] = out
        return self._chains[key]


@functools.lru_cache(maxsize=2)
def int_host(name):
    return IntHost(name)


def general_w(h, kind):
    """w of its own for the general operands: uniform in (-1, 1), in the vectors' type."""
    w = np.random.default_rng(len(h.name) + 41).uniform(-1.0, 1.0, size=h.rows)
    return w.astype(np.float32) if kind == "c16_f32xy" else w


def products(v, w):
    """(t0, t1): the rounded products of the dots over v (y_out as stored) and w (None: no second dot)."""
    v = np.asarray(v).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return v * v, (np.zeros(len(v)) if w is None else np.asarray(w).astype(np.float64) * v)


def bound(t):
    """rows 2^-53 sum |t_i|: the a-priori bound of any summation order over identically rounded products."""
    return len(t) * 2.0 ** -53 * float(np.sum(np.abs(t)))


def visible(name, kind, alpha, beta):
    """The share of the rows with entries whose |t_i| does not exceed ten times the bound, per dot (None where every t_i is 0:
    the dot is then +0.0 exactly), from the restatement of y_out."""
    h = host(name)
    z, _ = h.z(kind)
    x, y0, dtype = h.vectors(kind)
    v = restate(alpha, beta, z, y0, dtype)
    has = np.diff(h.p.astype(np.int64)) > 0
    shares = []
    ws = [general_w(h, kind)] + ([x] if h.rows == h.cols else [])
    for t in [products(v, None)[0]] + [products(v, w)[1] for w in ws]:
        if not np.any(t != 0):
            shares.append(None)
        else:
            shares.append(float(np.mean(np.abs(t[has]) <= 10.0 * bound(t))) if has.any() else 0.0)
    return shares
