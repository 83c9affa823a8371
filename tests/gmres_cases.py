"""Operands for the tests of the GMRES updates (include/spmv_hip_gmres.h), the header's contract restated in numpy, and what must
hold of the operands before a GPU result is looked at (test_gmres_cases.py asserts it without a device; test_gpu_gmres.py uses
the same operands).

The basis of a case is one array of (k + 1) ldv elements: vector j at j ldv, and w -- "the vector right behind them" -- at k ldv;
ldv is n rounded up to a 16-byte group plus one group, so that padding lies between the vectors.

INTEGER operands (int_case): basis and w in +-{1 ... 8}, h and y from {-2, -1, 0, 1, 2, 0.5}, minv from {0.5, 1, 2}, x in
+-{1 ... 8}.  Every stored value is a multiple of 1/4 of magnitude at most 8 + 32 * 2 * 8 = 520 (a float holds it), every product
of a dot is a multiple of 1/4 and 4 sum |t| < 2^53 at 2 M elements: any summation order is exact, so h and dots must equal the
sums formed in integers bit for bit.

GENERAL operands (general_case, n <= 4097 only): seeded normals, minv uniform in (0.5, 2).  The vectors are held bit for bit to
restate_update / restate_scale / restate_correct; each h[j] and dots[0] to n 2^-53 sum |t_i| of math.fsum(t) (dots_cases.bound).

The CHAIN (gmres_restated): GMRES(8) from x0 = 0 on bicgstab_cases.chain_matrix(), the loop of the header in numpy with numpy's
own sums."""
import functools
import math
from fractions import Fraction

import numpy as np

import dots_cases as dc
from bicgstab_cases import chain_matrix
from krylov_cases import CHUNK, DOTS_CHUNK, SIZES
from spmv_amd.capi import GMRES_MAX_BASIS, gmres_project, gmres_state_layout, gmres_update  # noqa: F401  (no feature, no operands)

bound = dc.bound
DTYPES = (np.float64, np.float32)
BLOCK = 8  # gmres_updates.hpp: kGmresBlock, the vectors whose sums a lane keeps at once
KS = [0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1, GMRES_MAX_BASIS]
BIG_SIZES = [DOTS_CHUNK * CHUNK, DOTS_CHUNK * CHUNK + 1]  # one and two stages of the reduction
BIG_K = 3
COEFFICIENTS = np.array([-2.0, -1.0, 0.0, 1.0, 2.0, 0.5])
CYCLE, CYCLES = 8, 2


def _f64(a):
    return np.asarray(a).astype(np.float64)


def ldv_of(n, dtype):
    w = 16 // np.dtype(dtype).itemsize
    return ((n + w - 1) // w + 1) * w


# ---- the streaming calls restated -------------------------------------------------------------------------------------------------------

def project_products(V, w):
    """[t_0 ... t_k]: the rounded products of h[j], j < k, over V (k rows) and of h[k] = w' w."""
    wd = _f64(w)
    with np.errstate(invalid="ignore", over="ignore"):
        return [_f64(v) * wd for v in V] + [wd * wd]


def restate_update(V, h, w, dtype):
    """w as the update stores it: one rounded product and one rounded difference per vector, j ascending, one cast last."""
    run = _f64(w).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for hj, v in zip(h, V):
            run = run - np.float64(hj) * _f64(v)
    return run.astype(dtype)


def restate_scale(scale, v, minv, dtype):
    """(v, vhat) as stored (vhat None without minv), vhat from v AS STORED."""
    with np.errstate(invalid="ignore", over="ignore"):
        out = (_f64(v) * np.float64(scale)).astype(dtype)
        return out, (None if minv is None else (_f64(minv) * _f64(out)).astype(dtype))


def restate_correct(V, y, minv, x, dtype):
    """x as the correction stores it; u starts from its first product.  No vector: x as it is."""
    if len(V) == 0:
        return np.asarray(x, dtype=dtype).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.float64(y[0]) * _f64(V[0])
        for yj, v in zip(y[1:], V[1:]):
            u = u + np.float64(yj) * _f64(v)
        if minv is not None:
            u = _f64(minv) * u
        return (_f64(x) + u).astype(dtype)


# ---- the small calls restated: Python floats are IEEE doubles, one rounding per operation, numpy's sqrt correctly rounded -----------------

def state_doubles(m):
    return (3 + 3 * m + m * (m + 1) // 2 + 1) & ~1


def restate_start(m, nrm2):
    lay = gmres_state_layout(m)
    st = np.full(state_doubles(m), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        beta = float(np.sqrt(np.float64(nrm2)))
        st[1] = np.float64(1.0) / np.float64(beta)
    st[0] = beta
    st[lay["g"]:lay["g"] + m + 1] = 0.0
    st[lay["g"]] = beta
    return st


def restate_column(state, k, m, h1, h2, nrm2):
    """The state after column k (a copy), the operations in the header's order."""
    lay = gmres_state_layout(m)
    st = np.array(state, dtype=np.float64)
    g, c, s, r = lay["g"], lay["c"], lay["s"], lay["r"] + k * (k + 1) // 2
    h = [float(h1[j]) + float(h2[j]) for j in range(k + 1)]
    with np.errstate(invalid="ignore"):
        below = float(np.sqrt(np.float64(nrm2)))
    for i in range(k):
        ci, si, a, b = float(st[c + i]), float(st[s + i]), h[i], h[i + 1]
        h[i] = ci * a + si * b
        h[i + 1] = ci * b - si * a
    a = h[k]
    d = float(np.sqrt(np.float64(a * a + below * below)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ck, sk = float(np.float64(a) / np.float64(d)), float(np.float64(below) / np.float64(d))
        st[1] = np.float64(1.0) / np.float64(below)
    st[c + k], st[s + k] = ck, sk
    h[k] = ck * a + sk * below
    st[r:r + k + 1] = h
    gk = float(st[g + k])
    st[g + k + 1] = -(sk * gk)
    st[g + k] = ck * gk
    st[0] = abs(st[g + k + 1])
    return st


def triangle(state, k, m):
    """R[0:k, 0:k] of the state as a dense upper triangle."""
    r = gmres_state_layout(m)["r"]
    R = np.zeros((k, k))
    for j in range(k):
        R[:j + 1, j] = state[r + j * (j + 1) // 2:r + j * (j + 1) // 2 + j + 1]
    return R


def restate_solve(state, k, m):
    lay = gmres_state_layout(m)
    R, y = triangle(state, k, m), [0.0] * k
    for i in range(k - 1, -1, -1):
        acc = float(state[lay["g"] + i])
        for j in range(i + 1, k):
            acc = acc - float(R[i, j]) * y[j]
        y[i] = acc / float(R[i, i])
    return np.array(y, dtype=np.float64)


def column_bound(k, h, below, gk):
    """8 (k + 2) 2^-53 max(||(h, h_{k+1})||_2, |g_k|): each of at most k + 1 rotations is orthogonal and costs a handful of
    roundings, sqrt is allowed 1 ulp."""
    return 8.0 * (k + 2) * 2.0 ** -53 * max(math.sqrt(sum(float(x) ** 2 for x in h) + float(below) ** 2), abs(float(gk)))


def solve_residual_and_bound(state, k, m, y):
    """(|R y - g|, gamma_k |R| |y|) per row: the triangular solve's backward bound.  Both sides are formed exactly, in
    Fractions: the bound is a few units of the last place, and a residual evaluated in fp64 would add roundings of its own."""
    R, g = triangle(state, k, m), state[gmres_state_layout(m)["g"]:][:k]
    u = Fraction(k, 2 ** 53)
    gamma = u / (1 - u)
    Rf, yf = [[Fraction(float(v)) for v in row] for row in R], [Fraction(float(v)) for v in y]
    resid = [abs(sum(Rf[i][j] * yf[j] for j in range(i, k)) - Fraction(float(g[i]))) for i in range(k)]
    bnd = [gamma * sum(abs(Rf[i][j] * yf[j]) for j in range(i, k)) for i in range(k)]
    return resid, bnd


# ---- operands ---------------------------------------------------------------------------------------------------------------------------

class Case:
    """k vectors and w in one array (basis: (k + 1) ldv elements of `dtype`, the padding NaN), h and y (k doubles), x, minv."""

    def __init__(self, n, k, dtype, V, w, h, y, x, minv):
        self.n, self.k, self.dtype, self.ldv = n, k, np.dtype(dtype), ldv_of(n, dtype)
        self.basis = np.full((k + 1) * self.ldv, np.nan, dtype=dtype)
        for j in range(k):
            self.basis[j * self.ldv:j * self.ldv + n] = V[j]
        self.basis[k * self.ldv:k * self.ldv + n] = w
        self.V = [self.basis[j * self.ldv:j * self.ldv + n].copy() for j in range(k)]
        self.w = self.basis[k * self.ldv:k * self.ldv + n].copy()
        self.h, self.y = np.asarray(h, dtype=np.float64), np.asarray(y, dtype=np.float64)
        self.x, self.minv = np.ascontiguousarray(x, dtype=dtype), np.ascontiguousarray(minv, dtype=dtype)


class IntOperands:
    def __init__(self, n, k):
        rng = np.random.default_rng(1000 * k + n % 997 + 7)

        def signed(size):
            return (rng.integers(1, 9, size=size) * rng.choice([-1, 1], size=size)).astype(np.int64)

        self.n, self.k = n, k
        self.V, self.w, self.x = signed((k, n)), signed(n), signed(n)
        self.h4 = (4 * rng.choice(COEFFICIENTS, size=k)).astype(np.int64)  # 4 h
        self.y4 = (4 * rng.choice(COEFFICIENTS, size=k)).astype(np.int64)
        self.m2 = rng.choice([1, 2, 4], size=n).astype(np.int64)           # 2 minv

    def case(self, dtype):
        return Case(self.n, self.k, dtype, self.V, self.w, self.h4 / 4.0, self.y4 / 4.0, self.x, self.m2 / 2.0)

    def sums(self):
        """(h of a project, 4 w after the update as integers, dots[0] of the update) formed in integers."""
        h = [int(np.sum(self.V[j] * self.w)) for j in range(self.k)] + [int(np.sum(self.w * self.w))]
        w4 = 4 * self.w - self.h4 @ self.V if self.k else 4 * self.w
        assert int(np.max(np.abs(w4), initial=0)) <= 4 * 520
        d16 = int(np.sum(w4 * w4))
        assert d16 < 2 ** 53 and d16 % 1 == 0
        return np.array(h, dtype=np.float64), w4, d16 / 16.0


@functools.lru_cache(maxsize=8)
def int_case(n, k):
    return IntOperands(n, k)


@functools.lru_cache(maxsize=None)
def general_case(n, k, dtype):
    assert n <= 4 * CHUNK + 1, "general operands are for small n (the module docstring)"
    rng = np.random.default_rng(100 * n + k + 17)
    return Case(n, k, dtype, rng.standard_normal((k, n)), rng.standard_normal(n), rng.standard_normal(k), rng.standard_normal(k),
                rng.standard_normal(n), rng.uniform(0.5, 2.0, size=n))


def small_cases():
    return [(n, k) for n in SIZES for k in KS]


# ---- the chain: GMRES(8) on the upwind operator ---------------------------------------------------------------------------------------

def row_sums(p, c, values, x):
    """A x with numpy's row sums, in fp64."""
    return np.add.reduceat(values * _f64(x)[c], p[:-1].astype(np.int64))


def orthogonality(V, dtype):
    """(max |V' V - I|, max over the entries of |V' V - I|_ij / bound_ij), the inner products formed by math.fsum: a product
    of 1369 terms evaluated in fp64 would add some 1e-15 of its own.  bound_ij = 6 sigma_ij + 8 * 2^-53 (six deviations: the
    largest of 45 entries in each of eight bases is looked at).  sigma_ij: a stored element has been rounded to its type twice,
    at the store of the update (or of the residual) and at the store of the scale; each is a relative delta uniform in +-u (u = 2^-53 or 2^-24) that is a function of the
    element's significand -- elements equal up to their sign and a power of two share one delta (V_0 is the integer right-hand
    side scaled: 1, 2, 4 and 8 share one, 3 and 6 another; five in all), different significands are taken as independent.  So
    sum_i v_i (1 + delta_i) w_i (1 + delta'_i) is off by a sum of variance 2 u^2 / 3 * (sum over the significands a of v of
    (sum_{i with a} v_i w_i)^2 + the same over the significands of w) -- 2 for the two roundings, the second one grouped as
    the first --; on the
    diagonal the two deltas are one, which doubles the deviation.  8 * 2^-53: the scale 1 / sqrt(w' w) is three roundings
    off in fp64 (twice that in the norm's square) and CGS2 leaves the projections at the level of fp64's rounding."""
    u = 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24
    B = [_f64(v) for v in V]
    groups = [np.unique(np.frexp(np.abs(v))[0], return_inverse=True)[1] for v in B]

    def grouped(t, g):
        return float(np.sum(np.bincount(g, weights=t) ** 2))

    worst = share = 0.0
    for i in range(len(B)):
        for j in range(i, len(B)):
            t = B[i] * B[j]
            g = abs(math.fsum(t.tolist()) - (1.0 if i == j else 0.0))
            var = 4.0 * grouped(t, groups[i]) if i == j else grouped(t, groups[i]) + grouped(t, groups[j])
            sigma = u * math.sqrt(2.0 / 3.0) * math.sqrt(var)
            worst, share = max(worst, g), max(share, g / (6.0 * sigma + 8.0 * 2.0 ** -53))
    return worst, share


def gmres_restated(dtype, with_minv, m=CYCLE, cycles=CYCLES):
    """The two walk-throughs of the header in numpy, from x0 = 0.  (The multiply's row sums and the sums of the dots are numpy's,
    not the GPU's: this shows what the loop does on this matrix, not the GPU's bits.)  {rr: r' r of r0 and after every cycle,
    estimate: state[0]^2 at the end of every cycle, subdiagonal: every h_{k+1,k}, orthogonality: max |V' V - I| per cycle,
    orthogonality_over_bound: orthogonality()'s second figure per cycle}."""
    rows, cols, p, c, v, b, minv = chain_matrix()
    mh = minv.astype(dtype) if with_minv else None
    x = np.zeros(rows, dtype=dtype)
    out = {"rr": [], "estimate": [], "subdiagonal": [], "orthogonality": [], "orthogonality_over_bound": []}

    def residual():
        r = (-1.0 * row_sums(p, c, v, x) + 1.0 * _f64(b.astype(dtype))).astype(dtype)
        return r, float(np.sum(_f64(r) * _f64(r)))

    r, rr = residual()
    out["rr"].append(rr)
    for _ in range(cycles):
        state = restate_start(m, rr)
        V = [None] * (m + 1)
        V[0], vhat = restate_scale(state[1], r, mh, dtype)
        for k in range(m):
            w = row_sums(p, c, v, V[k] if vhat is None else vhat).astype(dtype)
            h1 = [float(np.sum(t)) for t in project_products(V[:k + 1], w)]
            w = restate_update(V[:k + 1], h1[:k + 1], w, dtype)
            h2 = [float(np.sum(t)) for t in project_products(V[:k + 1], w)]
            w = restate_update(V[:k + 1], h2[:k + 1], w, dtype)
            nrm2 = float(np.sum(_f64(w) * _f64(w)))
            out["subdiagonal"].append(math.sqrt(nrm2))
            state = restate_column(state, k, m, h1, h2, nrm2)
            V[k + 1], vhat = restate_scale(state[1], w, mh, dtype)
        y = restate_solve(state, m, m)
        x = restate_correct(V[:m], y, mh, x, dtype)
        r, rr = residual()
        out["rr"].append(rr)
        out["estimate"].append(float(state[0]) ** 2)
        worst, share = orthogonality(V, dtype)
        out["orthogonality"].append(worst)
        out["orthogonality_over_bound"].append(share)
    return out
