"""Operands for the tests of the BiCGStab updates (include/spmv_hip_bicgstab.h), the header's contract restated in numpy, and what
must hold of the operands before a GPU result is looked at (test_bicgstab_cases.py asserts it without a device;
test_gpu_bicgstab.py uses the same operands).

INTEGER operands (int_case): v, r, phat, t, rhat, x, p in +-{1 ... 8}, every quotient in {1, -2, 0.5, 0} (w never 0 where b is
formed), minv in {0.5, 1, 2}.  Every stored value is a multiple of 1/32 of magnitude below 2^9 (a float holds it), no r after a
step is zero, and every product of the dots is a multiple of 1/4 with 4 sum |t| < 2^53: any summation order is exact, so both dots
must equal the sums formed in integers bit for bit.

GENERAL operands (general_case, n <= 4097 only): uniform in (-1, 1), minv uniform in (0.5, 2).  The vectors are held bit for bit
to restate_s / restate_step / restate_direction; the dots to n 2^-53 sum |t_i| of math.fsum(t) (dots_cases.bound).
visible_share() is the share of the elements whose |t_i| does not exceed ten times that bound: a lost or doubled element shows in
all the others.

The CHAIN matrix (chain_matrix): the 5-point upwind operator on a 37 x 37 grid -- 1369 rows: one whole chunk and a part, with a
tail of one element for doubles and floats alike -- diagonal 4, west -1.5, east -0.5, south -1.25, north -0.75, every row scaled
by a seeded choice from {1, 2, 4}: nonsymmetric, every value a float, and a Jacobi preconditioner that is not the identity."""
import functools
from fractions import Fraction

import numpy as np

import dots_cases as dc
from krylov_cases import BIG_SIZES, CHUNK, SIZES, quotient
from spmv_amd.capi import bicgstab_direction, bicgstab_s, bicgstab_step  # noqa: F401  (no feature, no operands)

bound = dc.bound
DTYPES = (np.float64, np.float32)
QUOTIENTS = [(3.0, 3.0), (-4.0, 2.0), (1.0, 2.0), (0.0, 1.0)]  # 1, -2, 0.5, 0
# (a, w, r) of a chained s, step and direction on integer operands, as indices into QUOTIENTS: every value in every place; w == 0
# has no direction behind it (r None)
INT_TRIPLES = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (3, 3, None), (1, 1, 3)]
# general operands: ((num_a, den_a), (num_w, den_w), (num_r, den_r)); on both sets (num_r a) / (den_r w) rounds to another b than
# the header's (num_r / den_r) (a / w) (test_bicgstab_cases.py)
GENERAL_QUOTIENTS = [((0.7310585786300049, -1.3), (1.0, 3.0), (-0.6, 0.7)), ((1.0, 3.0), (-0.37, 0.11), (2.3, 1.7))]
GRID = 37
ITERATIONS = 8


def _f64(a):
    return np.asarray(a).astype(np.float64)


def restate_s(num, den, v, r, minv, dtype):
    """(s, shat) as the call stores them (shat None without minv): every product and sum rounded in fp64, one cast to the vectors'
    type last, shat from s AS STORED."""
    a = quotient(num, den)
    with np.errstate(invalid="ignore", over="ignore"):
        av = a * _f64(v)
        s = (_f64(r) - av).astype(dtype)
        return s, (None if minv is None else (_f64(minv) * _f64(s)).astype(dtype))


def restate_step(qa, qw, phat, shat, t, x, r, dtype):
    """(x, r) as the step stores them; qa and qw are (num, den); shat None: the incoming r."""
    a, w = quotient(*qa), quotient(*qw)
    with np.errstate(invalid="ignore", over="ignore"):
        ap = a * _f64(phat)
        ws = w * _f64(r if shat is None else shat)
        wt = w * _f64(t)
        return ((_f64(x) + ap) + ws).astype(dtype), (_f64(r) - wt).astype(dtype)


def beta(qr, qa, qw):
    """b = fl(fl(num_r / den_r) fl(fl(num_a / den_a) / fl(num_w / den_w))): three divisions, one more, one product."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return quotient(*qr) * (quotient(*qa) / quotient(*qw))


def restate_direction(qr, qa, qw, r, v, p, minv, dtype):
    """(p, phat) as the direction stores them (phat None without minv)."""
    w, b = quotient(*qw), beta(qr, qa, qw)
    with np.errstate(invalid="ignore", over="ignore"):
        wv = w * _f64(v)
        d = _f64(p) - wv
        bd = b * d
        pn = (_f64(r) + bd).astype(dtype)
        return pn, (None if minv is None else (_f64(minv) * _f64(pn)).astype(dtype))


def step_products(r, rhat):
    """(t0, t1): the rounded products of the step's dots over r as stored."""
    rho = _f64(r)
    with np.errstate(invalid="ignore", over="ignore"):
        return rho * rho, _f64(rhat) * rho


NAMES = ("v", "r", "phat", "t", "rhat", "x", "p", "minv")


class IntCase:
    """Integer operands of n elements; triple(...) is what s, step and direction over them store, in integers."""

    def __init__(self, n):
        self.n = n
        rng = np.random.default_rng(n + 41)

        def signed(size):
            return rng.integers(1, 9, size=size) * rng.choice([-1, 1], size=size)

        self.v, ri, self.phat, self.t, self.rhat, self.x, self.p = (signed(n).astype(np.int64) for _ in range(7))
        # no r - a v - w t == 0 for the (a, w) of INT_TRIPLES: at most five values of r are excluded, six others are tried
        for cand in (1, -1, 3, -3, 5, -5):
            ri = np.where(self._zero(ri), cand, ri)
        self.r = ri
        self.m2 = rng.choice([1, 2, 4], size=n).astype(np.int64)  # 2 minv

    def _zero(self, ri):
        bad = np.zeros(self.n, dtype=bool)
        for ia, iw, _ in INT_TRIPLES:
            a2, w2 = (int(2 * Fraction(*[int(q) for q in QUOTIENTS[i]])) for i in (ia, iw))
            bad |= 2 * ri - a2 * self.v - w2 * self.t == 0
        return bad

    def arrays(self, dtype):
        """{name: array} in the vectors' type."""
        host = (self.v, self.r, self.phat, self.t, self.rhat, self.x, self.p, self.m2 / 2.0)
        return {k: np.ascontiguousarray(a, dtype=dtype) for k, a in zip(NAMES, host)}

    def triple(self, ia, iw, ir, with_minv):
        """An s with a = QUOTIENTS[ia], a step with that a and w = QUOTIENTS[iw], and (ir not None) a direction with those and
        r-quotient QUOTIENTS[ir], in Fractions held as integers over a common denominator: {s, shat, x, r, p, phat: (int64 array,
        denominator)}, d0, d1 as Fractions; the preconditions asserted."""
        a, w = (Fraction(int(QUOTIENTS[i][0])) / Fraction(int(QUOTIENTS[i][1])) for i in (ia, iw))
        a2, w2 = int(2 * a), int(2 * w)
        s2 = 2 * self.r - a2 * self.v                        # 2 s
        sh4 = self.m2 * s2 if with_minv else 2 * s2          # 4 shat (shat = s without minv)
        x8 = 8 * self.x + 4 * a2 * self.phat + w2 * sh4      # 8 x
        r2 = s2 - w2 * self.t                                # 2 r
        assert np.all(r2 != 0), "an r after the step is zero"
        out = {"s": (s2, 2), "shat": (sh4, 4), "x": (x8, 8), "r": (r2, 2)}
        t0, t1 = r2 * r2, self.rhat * r2                     # 4 rho rho, 2 rhat rho
        assert 4 * int(np.sum(t0)) < 2 ** 53 and 4 * int(np.sum(np.abs(t1))) < 2 ** 53, "a sum of magnitudes leaves fp64's integers"
        d0, d1 = Fraction(int(np.sum(t0)), 4), Fraction(int(np.sum(t1)), 2)
        if ir is not None:
            assert w != 0
            b = Fraction(int(QUOTIENTS[ir][0])) / Fraction(int(QUOTIENTS[ir][1])) * (a / w)
            b8 = b * 8
            assert b8.denominator == 1
            p16 = 8 * r2 + int(b8) * (2 * self.p - w2 * self.v)  # 16 p
            out["p"] = (p16, 16)
            out["phat"] = (self.m2 * p16, 32)
        for k, (num, den) in out.items():  # a float holds what is stored: a multiple of 1 / den below 2^24 / den
            assert int(np.max(np.abs(num), initial=0)) < 2 ** 24, k
        return out, d0, d1


@functools.lru_cache(maxsize=4)
def int_case(n):
    return IntCase(n)


class GeneralCase:
    def __init__(self, n):
        rng = np.random.default_rng(n + 53)
        self.n = n
        self.host = {k: rng.uniform(-1.0, 1.0, size=n) for k in NAMES[:-1]}
        self.host["minv"] = rng.uniform(0.5, 2.0, size=n)

    def arrays(self, dtype):
        return {k: np.ascontiguousarray(a.astype(dtype)) for k, a in self.host.items()}


@functools.lru_cache(maxsize=32)
def general_case(n):
    assert n <= 4 * CHUNK + 1, "general operands are for small n (the module docstring)"
    return GeneralCase(n)


def restate_triple(h, quotients, with_minv, dtype):
    """s, step and direction chained over the operands h ({name: array}): {s, shat, x, r, p, phat} as stored."""
    qa, qw, qr = quotients
    minv = h["minv"] if with_minv else None
    s, shat = restate_s(qa[0], qa[1], h["v"], h["r"], minv, dtype)
    x, r = restate_step(qa, qw, h["phat"], shat, h["t"], h["x"], s, dtype)
    p, phat = restate_direction(qr, qa, qw, r, h["v"], h["p"], minv, dtype)
    return {"s": s, "shat": shat, "x": x, "r": r, "p": p, "phat": phat}


def visible_share(n, quotients, dtype, with_minv):
    """Per dot, the share of the elements with |t_i| <= 10 x the bound, from the restatement of r (None: no element)."""
    h = general_case(n).arrays(dtype)
    rn = restate_triple(h, quotients, with_minv, dtype)["r"]
    return [float(np.mean(np.abs(t) <= 10.0 * bound(t))) if n else None for t in step_products(rn, h["rhat"])]


# ---- the chain: right-preconditioned BiCGStab on the upwind operator ----------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def chain_matrix():
    """(rows, cols, p, c, v, b, 1 / diag) of the scaled upwind operator in CSR, columns ascending, and its right-hand side."""
    g = GRID
    rows = g * g
    rng = np.random.default_rng(1369)
    scale = rng.choice([1.0, 2.0, 4.0], size=rows)
    b = rng.integers(-8, 9, size=rows).astype(np.float64)
    p, c, v = [0], [], []
    for k in range(rows):
        y, x = divmod(k, g)
        for ok, col, val in ((y > 0, k - g, -1.25), (x > 0, k - 1, -1.5), (True, k, 4.0), (x < g - 1, k + 1, -0.5), (y < g - 1, k + g, -0.75)):
            if ok:
                c.append(col)
                v.append(val * scale[k])
        p.append(len(c))
    p, c, v = np.array(p, dtype=np.int32), np.array(c, dtype=np.int32), np.array(v)
    assert np.all(v.astype(np.float32).astype(np.float64) == v)
    return rows, rows, p, c, v, b, 1.0 / (4.0 * scale)


def multiply(p, c, values, x, dtype):
    """A x with numpy's row sums, stored in the vectors' type."""
    return np.add.reduceat(values * _f64(x)[c], p[:-1].astype(np.int64)).astype(dtype)


def bicgstab_restated(dtype, with_minv, iterations=ITERATIONS):
    """The loop of the header in numpy, from x0 = 0: ([r' r] of r0 and after every iteration, [|rhat' v|], [t' t]).  (The
    multiply's row sums and the sums of the dots are numpy's, not the GPU's: this shows what the loop does on this matrix, not
    the GPU's bits.)"""
    rows, cols, p, c, v, b, minv = chain_matrix()
    m = minv.astype(dtype) if with_minv else None
    zero = np.zeros(rows, dtype=dtype)
    x, r = zero.copy(), b.astype(dtype)
    rhat = r.copy()
    one, nought = (1.0, 1.0), (0.0, 1.0)
    x, r = restate_step(nought, nought, zero, (zero if with_minv else None), zero, x, r, dtype)
    rho_old = [float(np.sum(t)) for t in step_products(r, rhat)]
    pd, phat = restate_direction(nought, one, one, r, zero, zero, m, dtype)
    norms, rv, tt = [rho_old[0]], [], []
    for _ in range(iterations):
        vd = multiply(p, c, v, pd if phat is None else phat, dtype)
        vv = [float(np.sum(t)) for t in dc.products(vd, rhat)]
        qa = (rho_old[1], vv[1])
        r, shat = restate_s(qa[0], qa[1], vd, r, m, dtype)
        td = multiply(p, c, v, r if shat is None else shat, dtype)
        ts = [float(np.sum(t)) for t in dc.products(td, r)]
        qw = (ts[1], ts[0])
        x, r = restate_step(qa, qw, pd if phat is None else phat, shat, td, x, r, dtype)
        rho_new = [float(np.sum(t)) for t in step_products(r, rhat)]
        pd, phat = restate_direction((rho_new[1], rho_old[1]), qa, qw, r, vd, pd, m, dtype)
        rho_old = rho_new
        norms.append(rho_new[0])
        rv.append(abs(vv[1]))
        tt.append(ts[0])
    return norms, rv, tt
