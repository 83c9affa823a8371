"""Operands for the tests of the Chebyshev polynomial preconditioner (include/spmv_hip_cheby.h), the header's three contracts
restated in numpy, and what must hold of the operands before a GPU result is looked at (test_cheby_cases.py asserts it without a
device; test_gpu_cheby.py uses the same operands).

The restatement: bound() adds a row's |a_ij| in stored order (np.add.at is unbuffered: index order) and takes numpy's maximum,
which a NaN wins; coeffs() is the header's recurrence in np.float64 scalars, one operation per line; step() forms fl(m u), the two
products and the sums in fp64, every numpy operation rounding on its own, with one cast to the vectors' type last.

INTEGER operands (int_case): u, d, z, r in +-{1 ... 8}, minv in {1, 2, 4} and INT_TABLE's entries in {1, 2}: every stored d and z is
an integer below 2^24 (a float holds it), every product of the dots an integer and the sums far below 2^53: any order is exact, so
d, z and both dots must equal the integer results bit for bit.

GENERAL operands (general_case, n <= 65537): uniform in (-1, 1), minv in (0.5, 2), the table coeffs() gives for lambda 2, ratio 30.
The vectors are held bit for bit to the restatement, the dots to n 2^-53 sum |t_i| of math.fsum(t) (dots_cases.bound)."""
import functools

import numpy as np

import dots_cases as dc
import krylov_cases as kc
from spmv_amd.capi import cheby_bound, cheby_coeffs, cheby_step  # noqa: F401  (no feature, no operands)

CHUNK = kc.CHUNK
DTYPES = (np.float64, np.float32)
MAX_DEGREE = 16
# the sizes of the issue, and the first whose slots take the reduction's second stage (it is the last of them)
SIZES = sorted({1, 2, 3, 1023, 1024, 1026, 2049, 65537, 2097153, kc.DOTS_CHUNK * CHUNK + 1})
GENERAL_LIMIT = 65537  # general operands up to here; above, integers only (the bound would hide elements)
# (name, degree, j, dots): every mode of the step
MODES = (("first", 3, 0, False), ("middle", 3, 1, False), ("last", 3, 2, False), ("last+dots", 3, 2, True), ("sole", 1, 0, False),
         ("sole+dots", 1, 0, True))
INT_TABLE = np.array([0.0, 2.0, 2.0, 1.0, 1.0, 2.0])  # degree 3; its first pair is a table of degree 1
ITERATIONS = 8
DEGREE, RATIO = 3, 30.0


def _f64(a):
    return np.asarray(a).astype(np.float64)


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def bound(rows, p, v, minv=None):
    """max_i fl(|m_i| s_i) as a np.float64, s_i the row's |a_ij| added in stored order to +0.0; +0.0 without rows."""
    p, v = np.asarray(p, dtype=np.int64), np.asarray(v, dtype=np.float64)
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(p[:rows + 1]))
    s = np.zeros(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(s, row, np.abs(v[p[0]:p[rows]]))
        t = s if minv is None else np.abs(_f64(minv)) * s
        return np.float64(np.max(t, initial=0.0)) if not np.any(np.isnan(t)) else np.float64(np.nan)


def coeffs(degree, lam, scale, ratio):
    """The table of 2 degree doubles, with the header's roundings."""
    assert 1 <= degree <= MAX_DEGREE
    lam, scale, ratio, half, two, one = (np.float64(a) for a in (lam, scale, ratio, 0.5, 2.0, 1.0))
    out = np.zeros(2 * degree)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        lmax = scale * lam
        lmin = lmax / ratio
        theta = (lmax + lmin) * half
        delta = (lmax - lmin) * half
        sigma = theta / delta
        rho = one / sigma
        out[1] = one / theta
        twice = two * sigma
        for j in range(1, degree):
            nxt = one / (twice - rho)
            out[2 * j] = nxt * rho
            out[2 * j + 1] = (two * nxt) / delta
            rho = nxt
    return out


def step(coef, degree, j, u, minv, d, z, dtype):
    """(d, z) as step j of `degree` stores them; d is None where the step does not store it."""
    assert 0 <= j < degree
    c, e = np.float64(coef[2 * j]), np.float64(coef[2 * j + 1])
    with np.errstate(invalid="ignore", over="ignore"):
        s = _f64(u) if minv is None else _f64(minv) * _f64(u)
        es = e * s
        if j == 0:
            dn = es
            zn = dn.astype(dtype)
        else:
            cd = c * _f64(d)
            dn = cd + es
            zn = (_f64(z) + dn).astype(dtype)
        return (dn.astype(dtype) if j < degree - 1 else None), zn


def products(z, r):
    """(t0, t1): the rounded products of the last step's dots over z as stored."""
    z, r = _f64(z), _f64(r)
    with np.errstate(invalid="ignore", over="ignore"):
        return z * r, z * z


def residual(multiply, r, z, dtype):
    """u = r - A z as the scaled multiply forms it from the row sums `multiply` gives (alpha -1, beta 1: two products, one sum)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (-1.0 * _f64(multiply(z)) + 1.0 * _f64(r)).astype(dtype)


def polynomial(multiply, coef, degree, r, minv, dtype):
    """z of one whole application: `degree` steps and the degree - 1 multiplies between them."""
    d, z = step(coef, degree, 0, r, minv, None, None, dtype)
    for j in range(1, degree):
        dn, z = step(coef, degree, j, residual(multiply, r, z, dtype), minv, d, z, dtype)
        d = dn if dn is not None else d
    return z


# ---- operands of the step ----------------------------------------------------------------------------------------------------------

class IntCase:
    def __init__(self, n):
        self.n = n
        rng = np.random.default_rng(n % 9973 + 17)

        def signed(size):
            return rng.integers(1, 9, size=size) * rng.choice([-1, 1], size=size)

        self.ui, self.di, self.zi, self.ri = (signed(n) for _ in range(4))
        self.mi = rng.choice([1, 2, 4], size=n)

    def arrays(self, dtype):
        """(u, minv, d, z, r) in the vectors' type."""
        return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (self.ui, self.mi, self.di, self.zi, self.ri))

    def results(self, degree, j, with_minv):
        """(d or None, z as int64, r'z, z'z as Python ints) of step j of `degree` over INT_TABLE, the preconditions asserted."""
        c, e = int(INT_TABLE[2 * j]), int(INT_TABLE[2 * j + 1])
        s = (self.mi if with_minv else 1) * self.ui.astype(np.int64)
        d = e * s if j == 0 else c * self.di.astype(np.int64) + e * s
        z = d if j == 0 else self.zi.astype(np.int64) + d
        assert int(np.max(np.abs(d), initial=0)) < 2 ** 24 and int(np.max(np.abs(z), initial=0)) < 2 ** 24
        t0, t1 = z * self.ri, z * z
        assert int(np.sum(np.abs(t0))) < 2 ** 53 and int(np.sum(t1)) < 2 ** 53, "a sum of magnitudes leaves fp64's integers"
        return (d if j < degree - 1 else None), z, int(np.sum(t0)), int(np.sum(t1))


@functools.lru_cache(maxsize=4)
def int_case(n):
    return IntCase(n)


class GeneralCase:
    def __init__(self, n):
        assert n <= GENERAL_LIMIT
        rng = np.random.default_rng(n % 9967 + 31)
        self.n = n
        self.u, self.d, self.z, self.r = (rng.uniform(-1.0, 1.0, size=n) for _ in range(4))
        self.minv = rng.uniform(0.5, 2.0, size=n)

    def arrays(self, dtype):
        return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (self.u, self.minv, self.d, self.z, self.r))


@functools.lru_cache(maxsize=16)
def general_case(n):
    return GeneralCase(n)


def general_table():
    return coeffs(DEGREE, 2.0, 1.0, RATIO)


def group_from_the_wrong_chunk(u):
    """A seeded defect in numpy: the lane's first 16-byte group of the second chunk of u read at the same place of the first
    chunk (needs more than a chunk and a group)."""
    w = 16 // np.asarray(u).dtype.itemsize
    assert len(u) >= CHUNK + w
    out = np.array(u)
    out[CHUNK:CHUNK + w] = out[:w]
    return out


# ---- matrices of the bound -----------------------------------------------------------------------------------------------------------

def ragged_matrix():
    """(rows, p, c, v): rows of 0 ... 70 entries, some empty (the first and the last among them), unsorted and repeated columns,
    row_ptr[0] == 0; magnitudes over twelve decades, so the order of a row's sum shows in its last bits."""
    rng = np.random.default_rng(77)
    rows = 211
    lens = rng.integers(0, 71, size=rows)
    lens[[0, 5, 6, 100, rows - 1]] = 0
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c = rng.integers(0, rows, size=int(p[-1])).astype(np.int32)  # (repeats and any order; the bound reads no column)
    v = rng.uniform(-1.0, 1.0, size=int(p[-1])) * 10.0 ** rng.integers(-6, 7, size=int(p[-1]))
    return rows, p, c, v


def last_row_matrix():
    """3000 rows (a dozen workgroups of the bound, the last one partly filled) whose largest row sum is the last row's."""
    rng = np.random.default_rng(78)
    rows = 3000
    lens = rng.integers(1, 9, size=rows)
    p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c = rng.integers(0, rows, size=int(p[-1])).astype(np.int32)
    v = rng.uniform(-1.0, 1.0, size=int(p[-1]))
    v[p[rows - 1]:] = rng.uniform(3.0, 4.0, size=int(lens[-1])) * rng.choice([-1.0, 1.0], size=int(lens[-1]))
    return rows, p, c, v


def bound_minv(rows, dtype):
    return np.random.default_rng(rows + 9).uniform(0.5, 1.0, size=rows).astype(dtype) * np.where(np.arange(rows) % 3 == 0, -1, 1).astype(dtype)


# ---- the chains: preconditioned CG with the polynomial ---------------------------------------------------------------------------------

def poisson_grid(g):
    """(rows, p, c, v) of the 5-point Laplacian on a g x g grid, columns sorted."""
    cols, vals, p = [], [], [0]
    for i in range(g):
        for j in range(g):
            k = i * g + j
            row = [(k - g, -1.0)] * (i > 0) + [(k - 1, -1.0)] * (j > 0) + [(k, 4.0)] + [(k + 1, -1.0)] * (j < g - 1) + [(k + g, -1.0)] * (i < g - 1)
            cols += [a for a, _ in row]
            vals += [b for _, b in row]
            p.append(len(cols))
    return g * g, np.array(p, dtype=np.int32), np.array(cols, dtype=np.int32), np.array(vals)


def multiplier(rows, p, c, values):
    """z -> A z, row sums in numpy's order (not the GPU's)."""
    values, first = _f64(values), np.asarray(p[:-1], dtype=np.int64)
    return lambda z: np.add.reduceat(values * _f64(z)[c], first)


def pcg_restated(rows, p, c, v, rhs, minv, dtype, degree, lam=None, ratio=RATIO, iterations=ITERATIONS):
    """The header's PCG composition in numpy from x0 = 0: [r'r] of r0 and after every iteration.  degree 0: the diagonal alone
    (z = minv r).  lam defaults to bound() of the matrix and minv."""
    mult = multiplier(rows, p, c, v if dtype == np.float64 else np.asarray(v).astype(np.float32))
    m = np.asarray(minv).astype(dtype)
    coef = coeffs(max(degree, 1), bound(rows, p, v, m) if lam is None else lam, 1.0, ratio)

    def precondition(r):
        if degree == 0:
            with np.errstate(invalid="ignore", over="ignore"):
                return (_f64(m) * _f64(r)).astype(dtype)
        return polynomial(mult, coef, degree, r, m, dtype)

    zero = np.zeros(rows, dtype=dtype)
    x, r = zero.copy(), np.asarray(rhs).astype(dtype)
    z = precondition(r)
    rz_old = float(np.sum(products(z, r)[0]))
    pd = kc.restate_direction(0.0, 1.0, z, None, zero, dtype)
    norms = [float(np.sum(_f64(r) * _f64(r)))]
    for _ in range(iterations):
        q = mult(pd).astype(dtype)
        pq = float(np.sum(_f64(pd) * _f64(q)))
        x, r = kc.restate_step(rz_old, pq, pd, q, x, r, dtype)
        z = precondition(r)
        rz_new = float(np.sum(products(z, r)[0]))
        pd = kc.restate_direction(rz_new, rz_old, z, None, pd, dtype)
        rz_old = rz_new
        norms.append(float(np.sum(_f64(r) * _f64(r))))
    return norms


@functools.lru_cache(maxsize=1)
def small_poisson():
    """The 10 x 10 grid of the issue, 1 / diag and a right-hand side; the seed is fixed."""
    rows, p, c, v = poisson_grid(10)
    return rows, p, c, v, np.random.default_rng(100).uniform(-1.0, 1.0, size=rows), np.full(rows, 0.25)


def bound_of(t):
    return dc.bound(t)
