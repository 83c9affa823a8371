"""Operands for the tests of the conjugate-gradient updates (include/spmv_hip_krylov.h), the header's contract restated in numpy,
and what must hold of the operands before a GPU result is looked at (test_krylov_cases.py asserts it without a device;
test_gpu_krylov.py uses the same operands).

INTEGER operands (int_case): p, q, x, r in +-{1 ... 8}, a = num / den in {1, -2, 0.5, 0}, minv in {0.5, 1, 2}.  Every stored x and
r is a multiple of 1/2 below 2^24 (a float holds it), no r - a q is zero, and every product of the dots is a multiple of 1/8
with 8 sum |t| < 2^53: any summation order is exact, so both dots must equal the sums formed in integers bit for bit.

GENERAL operands (general_case, n <= 4097 only): uniform in (-1, 1), minv uniform in (0.5, 2).  The vectors are held bit for bit
to restate_step / restate_direction; the dots to n 2^-53 sum |t_i| of math.fsum(t) (dots_cases.bound).  visible_share() is the
share of the elements whose |t_i| does not exceed ten times that bound: a lost or doubled element shows in all the others.  At
n of a million the bound would hide 2 % of the elements, which is why the large sizes use integer operands only."""
import functools
import os
from fractions import Fraction

import numpy as np

import compact_cases as cc
import dots_cases as dc
from spmv_amd.capi import cg_direction, cg_step, krylov_workspace_bytes  # noqa: F401  (no feature, no operands)

CHUNK = 1024              # SPMV_HIP_KRYLOV_CHUNK: elements of a wave and of a slot
SPAN = 4 * CHUNK          # elements of a workgroup
DOTS_CHUNK = 2048         # slots per workgroup of the reduction's first stage (csr_dots.hpp: kDotsChunk)
DTYPES = (np.float64, np.float32)
# 0, the smallest, around the wave (63, 64, 65 elements: 16, 32 groups of floats and doubles with and without a tail), around
# the chunk, two chunks and a part with a tail of 3 floats, around the workgroup
SIZES = [0, 1, 2, 3, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, SPAN - 1, SPAN + 1]
# the largest n whose slots one workgroup of the reduction adds, and the smallest that takes two stages: integer operands only
BIG_SIZES = [DOTS_CHUNK * CHUNK, DOTS_CHUNK * CHUNK + 1]
QUOTIENTS = [(3.0, 3.0), (-4.0, 2.0), (1.0, 2.0), (0.0, 1.0)]  # a = 1, -2, 0.5, 0
GENERAL_QUOTIENTS = [(0.7310585786300049, -1.3), (1.0, 3.0)]
POISSON_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poisson2D.mtx")
POISSON_B = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poisson2D_b.txt")
ITERATIONS = 8


def quotient(num, den):
    """One IEEE fp64 division, whatever the operands."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.float64(num) / np.float64(den)


def _f64(a):
    return np.asarray(a).astype(np.float64)


def restate_step(num, den, p, q, x, r, dtype):
    """(x, r) as the step stores them: every product and sum rounded in fp64, one cast to the vectors' type last."""
    a = quotient(num, den)
    with np.errstate(invalid="ignore", over="ignore"):
        ap, aq = a * _f64(p), a * _f64(q)
        return (_f64(x) + ap).astype(dtype), (_f64(r) - aq).astype(dtype)


def restate_direction(num, den, r, minv, p, dtype):
    """p as the direction stores it."""
    b = quotient(num, den)
    with np.errstate(invalid="ignore", over="ignore"):
        z = _f64(r) if minv is None else _f64(minv) * _f64(r)
        bp = b * _f64(p)
        return (z + bp).astype(dtype)


def step_products(r, minv):
    """(t0, t1): the rounded products of the step's dots over r as stored; t1 is +0.0 without minv."""
    v = _f64(r)
    with np.errstate(invalid="ignore", over="ignore"):
        return v * v, (np.zeros(len(v)) if minv is None else (_f64(minv) * v) * v)


class IntCase:
    """Integer operands of n elements; step(num, den, minv) is what a step over them stores, in integers."""

    def __init__(self, n):
        self.n = n
        rng = np.random.default_rng(n + 11)

        def signed(size):
            return rng.integers(1, 9, size=size) * rng.choice([-1, 1], size=size)

        self.pi, self.qi, self.xi, ri = signed(n), signed(n), signed(n), signed(n)
        # no r - a q == 0 for a in {1, -2, 0.5, 0}: r is none of q, -2 q, q / 2 (and not 0)
        for cand in (1, -1, 3, -3):
            bad = (ri == self.qi) | (ri == -2 * self.qi) | (2 * ri == self.qi)
            ri = np.where(bad, cand, ri)
        self.ri = ri
        self.m2 = rng.choice([1, 2, 4], size=n)  # 2 minv

    def arrays(self, dtype):
        """(p, q, x, r, minv) in the vectors' type."""
        return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (self.pi, self.qi, self.xi, self.ri, self.m2 / 2.0))

    def step(self, num, den, with_minv):
        """(2 x, 2 r as int64 arrays, dots[0], dots[1] as Fractions) of a step with a = num / den, the preconditions asserted."""
        a2 = Fraction(num) / Fraction(den) * 2
        assert a2.denominator == 1 and Fraction(a2, 2) in (1, -2, Fraction(1, 2), 0)
        a2 = int(a2)
        x2, r2 = 2 * self.xi.astype(np.int64) + a2 * self.pi, 2 * self.ri.astype(np.int64) - a2 * self.qi
        assert np.all(r2 != 0), "an r - a q is zero"
        # (int64 holds all of this exactly: |x2|, |r2| <= 48, a product at most 4 * 48^2, a sum at most n times that)
        assert int(np.max(np.abs(x2), initial=0)) < 2 ** 24 and int(np.max(np.abs(r2), initial=0)) < 2 ** 24
        t0 = r2 * r2                        # 4 v v
        t1 = self.m2.astype(np.int64) * t0  # 8 (m v) v
        assert 8 * int(np.sum(t0)) < 2 ** 53 and int(np.sum(t1)) < 2 ** 53, "a sum of magnitudes leaves fp64's integers"
        return x2, r2, Fraction(int(np.sum(t0)), 4), (Fraction(int(np.sum(t1)), 8) if with_minv else Fraction(0))


@functools.lru_cache(maxsize=4)
def int_case(n):
    return IntCase(n)


class GeneralCase:
    def __init__(self, n):
        rng = np.random.default_rng(n + 29)
        self.n = n
        self.p, self.q, self.x, self.r = (rng.uniform(-1.0, 1.0, size=n) for _ in range(4))
        self.minv = rng.uniform(0.5, 2.0, size=n)

    def arrays(self, dtype):
        return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (self.p, self.q, self.x, self.r, self.minv))


@functools.lru_cache(maxsize=32)
def general_case(n):
    assert n <= SPAN + 1, "general operands are for small n (the module docstring)"
    return GeneralCase(n)


def visible_share(n, num, den, dtype, with_minv):
    """Per dot, the share of the elements with |t_i| <= 10 x the bound, from the restatement of r (None: no element)."""
    p, q, x, r, minv = general_case(n).arrays(dtype)
    rn = restate_step(num, den, p, q, x, r, dtype)[1]
    return [float(np.mean(np.abs(t) <= 10.0 * dc.bound(t))) if n else None
            for t in step_products(rn, minv if with_minv else None)[:2 if with_minv else 1]]


# ---- the chain: preconditioned CG on tests/golden/poisson2D.mtx ---------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def poisson():
    """(rows, cols, p, c, v, b, 1 / diag) of the golden Poisson matrix and its right-hand side."""
    rows, cols, p, c, v = cc._load(POISSON_FILE)
    b = np.loadtxt(POISSON_B)
    assert rows == cols == len(b) and np.all(np.diff(p) > 0)
    row = np.repeat(np.arange(rows), np.diff(p))
    diag = np.zeros(rows)
    diag[row[c == row]] = v[c == row]
    assert np.all(diag > 0)
    return rows, cols, p, c, v, b, 1.0 / diag


def pcg_restated(dtype, with_minv, iterations=ITERATIONS):
    """The loop of the header in numpy, from x0 = 0: [r' r] of r0 and after every iteration.  (The multiply's row sums are
    numpy's, not the GPU's: this shows what the loop does on this matrix, not the GPU's bits.)"""
    rows, cols, p, c, v, b, minv = poisson()
    values = v if dtype == np.float64 else v.astype(np.float32).astype(np.float64)
    m = minv.astype(dtype) if with_minv else None
    x, r = np.zeros(rows, dtype=dtype), b.astype(dtype)
    zero = np.zeros(rows, dtype=dtype)
    x, r = restate_step(0.0, 1.0, zero, zero, x, r, dtype)
    rz_old = [float(np.sum(t)) for t in step_products(r, m)]
    pd = restate_direction(0.0, 1.0, r, m, zero, dtype)
    k = 1 if with_minv else 0
    norms = [rz_old[0]]
    for _ in range(iterations):
        q = np.add.reduceat(values * _f64(pd)[c], p[:-1].astype(np.int64)).astype(dtype)
        pq = float(np.sum(_f64(pd) * _f64(q)))
        x, r = restate_step(rz_old[k], pq, pd, q, x, r, dtype)
        rz_new = [float(np.sum(t)) for t in step_products(r, m)]
        pd = restate_direction(rz_new[k], rz_old[k], r, m, pd, dtype)
        rz_old = rz_new
        norms.append(rz_new[0])
    return norms
