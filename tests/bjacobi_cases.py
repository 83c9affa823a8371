"""Operands for the tests of the point-block Jacobi preconditioner (include/spmv_hip_bjacobi.h), the header's contract restated
in numpy, and what must hold of the operands before a GPU result is looked at (test_bjacobi_cases.py asserts it without a
device; test_gpu_bjacobi.py uses the same operands).

The restatement: extract() adds a block's entries in stored order (np.add.at is unbuffered: index order), invert() is the
header's Gauss-Jordan with partial pivoting over all blocks at once -- every numpy operation rounds on its own, and the pivot is
chosen with `>` from row c on, so a NaN never wins -- and apply() / apply_add() form the row sums from the first product on, j
ascending, in fp64 with one cast to the vectors' type last.

INTEGER operands (int_case): r, u, x in +-{1 ... 8}, the inverse's entries in {-2 ... 2} with a non-zero diagonal entry.  Every z
and x is an integer below 2^24 (a float holds it), every product of the dots an integer and the sums far below 2^53: any order
is exact, so z, x and both dots must equal the integer results bit for bit.

GENERAL operands (general_case): uniform in (-1, 1).  The vectors are held bit for bit to the restatement, the dots to
n 2^-53 sum |t_i| of math.fsum(t) (dots_cases.bound)."""
import functools

import numpy as np

import dots_cases as dc
import krylov_cases as kc
from spmv_amd.capi import bjacobi_apply, bjacobi_apply_add, bjacobi_setup  # noqa: F401  (no feature, no operands)

CHUNK = kc.CHUNK
DTYPES = (np.float64, np.float32)
BLOCKS = tuple(range(1, 9))
# the sizes of the issue: the multiples of b nearest to these
TARGETS = (1, 2, 1023, 1024, 1026, 2049, 65537, 2097153)
GENERAL_LIMIT = 65537 + 8  # general operands up to here; above, integers only (the bound would hide elements)
ITERATIONS = 8


def nearest(target, b):
    """The multiple of b nearest to target (b for the two smallest: b and 2 b are meant there)."""
    if target <= 2:
        return target * b
    return max(b, (target + b // 2) // b * b)


def sizes(b):
    """The issue's sizes; where the largest is 2048 chunks or fewer (b = 4, 7, 8) the next multiple of b beyond them as well: the
    first size whose slots take the reduction's second stage."""
    s = {nearest(t, b) for t in TARGETS}
    if max(s) <= kc.DOTS_CHUNK * CHUNK:
        s.add((kc.DOTS_CHUNK * CHUNK // b + 1) * b)
    return sorted(s)


def _f64(a):
    return np.asarray(a).astype(np.float64)


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def extract(rows, b, p, c, v):
    """The rows / b diagonal blocks (nblk, b, b) of a CSR matrix, entries added in stored order to +0.0."""
    assert rows % b == 0
    p, c, v = np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(v, dtype=np.float64)
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(p))
    k = row // b
    inside = (c >= k * b) & (c < (k + 1) * b)
    blocks = np.zeros((rows // b, b, b))
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(blocks, (k[inside], row[inside] - k[inside] * b, c[inside] - k[inside] * b), v[inside])
    return blocks


def invert(blocks, dtype):
    """(inverse (nblk, b, b) in dtype, singular count, first singular block or -1): the header's Gauss-Jordan on [B | I]."""
    nblk, b, _ = blocks.shape
    m = np.concatenate([np.array(blocks, dtype=np.float64), np.broadcast_to(np.eye(b), (nblk, b, b))], axis=2)
    every = np.arange(nblk)
    singular = np.zeros(nblk, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in range(b):
            piv = np.full(nblk, c)
            best = np.abs(m[:, c, c])
            for i in range(c + 1, b):
                a = np.abs(m[:, i, c])
                wins = a > best
                best = np.where(wins, a, best)
                piv = np.where(wins, i, piv)
            rc, rp = m[every, c, :].copy(), m[every, piv, :].copy()
            m[every, piv, :] = rc
            m[every, c, :] = rp
            pivot = m[:, c, c].copy()
            singular |= (pivot == 0.0)
            t = 1.0 / pivot
            f = m[:, :, c].copy()
            ec = m[:, c, :] * t[:, None]
            m[:, c, :] = ec
            for i in range(b):
                if i != c:
                    m[:, i, :] = m[:, i, :] - f[:, i, None] * ec
        inv = m[:, :, b:].copy()
        inv[singular] = np.eye(b)
        out = inv.astype(dtype)
    idx = np.flatnonzero(singular)
    return out, int(len(idx)), int(idx[0]) if len(idx) else -1


def row_sums(inv, r, b):
    """sum_j fl(inv[i][j] r[kb + j]) in fp64 from the first product on; inv is the flat array of n b elements."""
    n = len(r)
    assert n % b == 0 and np.asarray(inv).size == n * b
    a = _f64(inv).reshape(n // b, b, b)
    rb = _f64(r).reshape(n // b, b)
    with np.errstate(invalid="ignore", over="ignore"):
        s = a[:, :, 0] * rb[:, None, 0]
        for j in range(1, b):
            s = s + a[:, :, j] * rb[:, None, j]
    return s.reshape(n)


def apply(inv, r, b, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return row_sums(inv, r, b).astype(dtype)


def apply_add(inv, u, x, b, dtype):
    with np.errstate(invalid="ignore", over="ignore"):
        return (_f64(x) + row_sums(inv, u, b)).astype(dtype)


def apply_products(z, r):
    """(t0, t1): the rounded products of the apply's dots over z as stored."""
    z, r = _f64(z), _f64(r)
    with np.errstate(invalid="ignore", over="ignore"):
        return z * r, z * z


# ---- operands of the apply ---------------------------------------------------------------------------------------------------------

class IntCase:
    def __init__(self, n, b):
        assert n % b == 0
        self.n, self.b = n, b
        rng = np.random.default_rng(1000 * b + n % 997 + 3)

        def signed(size):
            return rng.integers(1, 9, size=size) * rng.choice([-1, 1], size=size)

        self.ri, self.xi = signed(n), signed(n)
        inv = rng.integers(-2, 3, size=(n // b, b, b))
        d = np.arange(b)
        inv[:, d, d] = rng.choice([-2, -1, 1, 2], size=(n // b, b))
        self.invi = inv.reshape(n * b)

    def arrays(self, dtype):
        """(inv, r, x) in the vectors' type."""
        return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (self.invi, self.ri, self.xi))

    def results(self):
        """(z, x + z as int64, r'z, z'z as Python ints), the preconditions asserted."""
        n, b = self.n, self.b
        z = np.einsum("kij,kj->ki", self.invi.reshape(n // b, b, b).astype(np.int64), self.ri.reshape(n // b, b).astype(np.int64)).reshape(n)
        assert int(np.max(np.abs(z), initial=0)) + 8 < 2 ** 24
        t0, t1 = z * self.ri, z * z
        assert int(np.sum(np.abs(t0))) < 2 ** 53 and int(np.sum(t1)) < 2 ** 53, "a sum of magnitudes leaves fp64's integers"
        return z, self.xi + z, int(np.sum(t0)), int(np.sum(t1))


@functools.lru_cache(maxsize=4)
def int_case(n, b):
    return IntCase(n, b)


class GeneralCase:
    def __init__(self, n, b):
        assert n % b == 0 and n <= GENERAL_LIMIT
        rng = np.random.default_rng(7000 * b + n % 991 + 29)
        self.n, self.b = n, b
        self.inv = rng.uniform(-1.0, 1.0, size=n * b)
        self.r, self.x = rng.uniform(-1.0, 1.0, size=n), rng.uniform(-1.0, 1.0, size=n)

    def arrays(self, dtype):
        return tuple(np.ascontiguousarray(a.astype(dtype)) for a in (self.inv, self.r, self.x))


@functools.lru_cache(maxsize=8)
def general_case(n, b):
    return GeneralCase(n, b)


def chunk_relative_blocks(inv, r, b, dtype):
    """A seeded defect in numpy: the block of an element found from its index inside the chunk, not inside the vector (wrong
    wherever CHUNK is no multiple of b and the element lies behind the first chunk)."""
    n = len(r)
    e = np.arange(n)
    base = e // CHUNK * CHUNK
    kb = np.minimum(base + (e - base) // b * b, n - b)
    a, rr = _f64(inv).reshape(n, b), _f64(r)
    s = a[:, 0] * rr[kb]
    for j in range(1, b):
        s = s + a[:, j] * rr[kb + j]
    return s.astype(dtype)


# ---- matrices of the setup ---------------------------------------------------------------------------------------------------------

def setup_matrix(b, nblk=37, seed=0):
    """A CSR matrix of nblk blocks of size b whose rows hold, besides the block's entries, entries outside it on both sides
    (the rows of block 5 some 200 of them: several passes of the wave), columns in shuffled order, some positions stored twice or
    three times, some not stored, some rows with no entry in the block, block 3 singular (a zero column where b > 1, a zero
    entry where b == 1) and block 7 without any stored entry.  Returns (rows, p, c, v)."""
    rng = np.random.default_rng(100 * b + seed)
    rows = nblk * b
    p, cols, vals = [0], [], []
    for k in range(nblk):
        blk = rng.uniform(-1.0, 1.0, size=(b, b)) + np.diag(rng.choice([-3.0, 3.0], size=b)) * (k % 2)  # odd blocks dominant
        if k == 3:
            blk[:, b - 1] = 0.0
        for i in range(b):
            entries = []
            empty_row = (k % 11 == 4 and i == b - 1 and b > 1)
            for j in range(b):
                if k == 7 or empty_row:
                    break
                if k % 5 == 1 and (i + j) % 2 == 1:
                    continue  # a position not stored
                parts = 1 + (k + i + j) % 3 if k % 4 == 2 else 1
                share = rng.uniform(-1.0, 1.0, size=parts)
                share[-1] = blk[i, j] - np.sum(share[:-1])
                entries += [(k * b + j, s) for s in share]
            outside = [col for col in rng.integers(0, rows, size=200 if k == 5 else 6) if not k * b <= col < (k + 1) * b]
            entries += [(int(col), rng.uniform(-1.0, 1.0)) for col in outside]
            order = rng.permutation(len(entries))
            cols += [entries[o][0] for o in order]
            vals += [entries[o][1] for o in order]
            p.append(len(cols))
    return rows, np.array(p, dtype=np.int32), np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64)


def swap_blocks(b, nblk, seed):
    """Blocks that force a row swap at every column: a dominant anti-diagonal-like permutation plus noise."""
    rng = np.random.default_rng(seed)
    out = rng.uniform(-0.1, 0.1, size=(nblk, b, b))
    for k in range(nblk):
        perm = np.roll(np.arange(b), 1 + k % max(1, b - 1)) if b > 1 else np.arange(1)
        out[k, perm, np.arange(b)] += rng.choice([-4.0, 4.0], size=b)
    return out


def dominant_blocks(b, nblk, seed):
    rng = np.random.default_rng(seed)
    out = rng.uniform(-1.0, 1.0, size=(nblk, b, b))
    d = np.arange(b)
    out[:, d, d] = (np.sum(np.abs(out), axis=2) + 1.0) * rng.choice([-1.0, 1.0], size=(nblk, b))
    return out


def rotated_spd_blocks(b, nblk, seed):
    """Q diag(1, 10, ..., 10^(b-1) capped at 1e6) Q' with a random orthogonal Q per block."""
    rng = np.random.default_rng(seed)
    out = np.empty((nblk, b, b))
    for k in range(nblk):
        q, _ = np.linalg.qr(rng.normal(size=(b, b)))
        out[k] = (q * np.minimum(10.0 ** np.arange(b), 1e6)) @ q.T
    return out


def residual(blocks, inverse):
    """max |B X - I| per block, in fp64 (numpy's matmul)."""
    b = blocks.shape[1]
    return np.max(np.abs(blocks @ _f64(inverse) - np.eye(b)), axis=(1, 2))


# ---- the 432-unknown SPD case of the issue -----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def spd_case():
    """(rows, p, c, v, rhs): kron(5-point Laplacian on 12 x 12, [[2,1,0],[1,2,1],[0,1,2]]) plus a rotated diag(1, 10, 100) per
    node, as CSR with sorted columns, and a right-hand side; the seed is fixed."""
    g, b = 12, 3
    lap = np.zeros((g * g, g * g))
    for i in range(g):
        for j in range(g):
            k = i * g + j
            lap[k, k] = 4.0
            for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= i + di < g and 0 <= j + dj < g:
                    lap[k, (i + di) * g + j + dj] = -1.0
    a = np.kron(lap, np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 2.0]]))
    node = rotated_spd_blocks(b, g * g, 20260)
    for k in range(g * g):
        a[k * b:(k + 1) * b, k * b:(k + 1) * b] += node[k]
    a = (a + a.T) / 2.0
    rows = g * g * b
    assert rows == 432
    nz = a != 0.0
    p = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int32)
    c = np.nonzero(nz)[1].astype(np.int32)
    v = a[nz]
    rhs = np.random.default_rng(432).uniform(-8.0, 8.0, size=rows)
    return rows, p, c, v, rhs


def spd_inverse(b, dtype):
    """The flat inverse of the SPD case's blocks of size b (b == 1: 1 / diag) as setup stores it."""
    rows, p, c, v, _ = spd_case()
    inv, count, first = invert(extract(rows, b, p, c, v), dtype)
    assert count == 0 and first == -1
    return np.ascontiguousarray(inv.reshape(rows * b))


def multiply(rows, p, c, values, x):
    """Row sums in numpy's order (not the GPU's)."""
    return np.add.reduceat(_f64(values) * _f64(x)[c], p[:-1].astype(np.int64))


def pcg_restated(dtype, b, iterations=ITERATIONS):
    """The header's PCG composition in numpy on the SPD case, from x0 = 0: [r'r] of r0 and after every iteration."""
    rows, p, c, v, rhs = spd_case()
    values = v if dtype == np.float64 else v.astype(np.float32)
    inv = spd_inverse(b, dtype)
    zero = np.zeros(rows, dtype=dtype)
    x, r = zero.copy(), rhs.astype(dtype)
    z = apply(inv, r, b, dtype)
    rz_old = float(np.sum(apply_products(z, r)[0]))
    pd = kc.restate_direction(0.0, 1.0, z, None, zero, dtype)
    norms = [float(np.sum(_f64(r) * _f64(r)))]
    for _ in range(iterations):
        q = multiply(rows, p, c, values, pd).astype(dtype)
        pq = float(np.sum(_f64(pd) * _f64(q)))
        x, r = kc.restate_step(rz_old, pq, pd, q, x, r, dtype)
        z = apply(inv, r, b, dtype)
        rz_new = float(np.sum(apply_products(z, r)[0]))
        pd = kc.restate_direction(rz_new, rz_old, z, None, pd, dtype)
        rz_old = rz_new
        norms.append(float(np.sum(_f64(r) * _f64(r))))
    return norms


def bound(t):
    return dc.bound(t)
