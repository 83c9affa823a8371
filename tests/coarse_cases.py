"""The contract of include/spmv_hip_coarse.h restated in numpy, and the matrices of its tests (test_coarse_cases.py holds the
restatement to its properties without a device; test_gpu_coarse.py holds the GPU to the restatement bit for bit).

The restatement uses element-wise numpy operations alone -- each rounds on its own; `@` may fuse.  densify() adds a row's entries
in stored order (np.add.at is unbuffered: index order) and counts the columns outside 0 ... n - 1; invert() is the header's
Gauss-Jordan with partial pivoting on [B | I], the pivot the first row >= c with the largest magnitude (a NaN is no candidate, and a
NaN in row c keeps row c), the first zero pivot ending it with the identity; apply() gives lane l of 64 the products l, l + 64,
... of a row, added in that order to +0.0, and adds the lanes by the butterfly p += p[lane ^ step], step = 1 ... 32, with one cast
to the vectors' type last.

A NaN that arithmetic creates has the sign and payload of the machine that created it, so same() compares the positions of the
NaNs and the bits of everything else."""
import functools

import numpy as np

import agg_cases as ac
import agg_mis2_cases as a2
import mcgs_cases as mc
from spmv_amd.capi import coarse_apply, coarse_ld, coarse_setup, coarse_workspace_bytes  # noqa: F401  (no feature, no cases)

DTYPES = (np.float64, np.float32)
MAX_N = 2048
LANES = 64
# the sizes of the issue; 15, 16, 17: a workgroup of the update takes 16 rows; 255, 256: the pivot kernel's 256 threads stride the
# rows and the pairs of columns (257 is the issue's).  The update's 128 columns a workgroup are crossed by every matrix above 64 rows:
# the columns it works on start at c & ~1.
SIZES = (0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 129, 225, 255, 256, 257, 513)
# eight PCG iterations on poisson2D.mtx with the two-level cycle over the 38 distance-2 aggregates at omega 1 (agg_mis2_cases.py)
PCG_RR = 6.721731e-03


def ld_of(n):
    """spmv_hip_coarse_ld."""
    return 0 if n <= 0 else (n + 3) // 4 * 4


def workspace_of(n):
    """spmv_hip_coarse_workspace: [B | I] as n rows of 2 ld doubles and one column of ld doubles; at least 16 bytes."""
    ld = ld_of(n)
    return max(16, 8 * (2 * n * ld + ld))


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def densify(n, p, c, v):
    """(B, the entries skipped for their column)."""
    p, c, v = np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(v, dtype=np.float64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(p))
    inside = (c >= 0) & (c < n)
    B = np.zeros((n, n))
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(B, (row[inside], c[inside]), v[inside])
    return B, int(np.sum(~inside))


def invert(B, dtype):
    """(the inverse as n rows of ld elements of dtype with +0.0 padding, singular 0 / 1, its column or -1)."""
    n = B.shape[0]
    m = np.concatenate([np.array(B, dtype=np.float64), np.eye(n)], axis=1)
    tmp = np.empty_like(m)
    column = -1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in range(n):
            a = np.abs(m[c:, c])
            piv = c if np.isnan(a[0]) else c + int(np.argmax(np.where(np.isnan(a), -1.0, a)))  # argmax: the first of equals
            if piv != c:
                m[[c, piv]] = m[[piv, c]]
            pivot = m[c, c]
            if pivot == 0.0:
                column = c
                break
            t = 1.0 / pivot
            f = m[:, c].copy()
            ec = m[c] * t
            np.multiply(f[:, None], ec[None, :], out=tmp)
            np.subtract(m, tmp, out=m)
            m[c] = ec
        out = np.zeros((n, ld_of(n)), dtype=dtype)
        out[:, :n] = np.eye(n) if column >= 0 else m[:, n:]
    return out, int(column >= 0), column


def setup(n, p, c, v, dtype):
    """(inv (n, ld), [singular, column, skipped]): what spmv_hip_coarse_setup_* stores."""
    B, skipped = densify(n, p, c, v)
    inv, singular, column = invert(B, dtype)
    return inv, [singular, column, skipped]


def apply(inv, n, r, dtype):
    """z of spmv_hip_coarse_apply_*: inv is (n, ld) or flat; the padding columns are not looked at."""
    a = np.asarray(inv).reshape(n, ld_of(n))[:, :n].astype(np.float64)
    r64 = np.asarray(r, dtype=dtype).astype(np.float64)
    trips = -(-n // LANES)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.zeros((n, trips * LANES))
        prod[:, :n] = a * r64[None, :]
        s = np.zeros((n, LANES))
        lane = np.arange(LANES)
        for t in range(trips):
            live = (lane + t * LANES < n)[None, :]
            s = np.where(live, s + prod[:, t * LANES:(t + 1) * LANES], s)  # a lane without an element adds nothing
        step = 1
        while step < LANES:
            s = s + s[:, lane ^ step]
            step *= 2
        return s[:, 0].astype(dtype)


def same(got, want):
    """NaNs in the same positions and every other value the same bits (floats are widened first: exact, and it keeps a zero's sign)."""
    g, w = (np.ascontiguousarray(np.asarray(x).astype(np.float64)).ravel() for x in (got, want))
    if g.shape != w.shape:
        return False
    gn, wn = np.isnan(g), np.isnan(w)
    return bool(np.array_equal(gn, wn) and np.array_equal(g[~gn].view(np.uint64), w[~wn].view(np.uint64)))


def residual(A, X):
    """max |A X - I| in fp64 (numpy's matmul: a measurement, not a restatement)."""
    n = A.shape[0]
    return float(np.max(np.abs(A @ np.asarray(X, dtype=np.float64)[:, :n] - np.eye(n)), initial=0.0))


# ---- the matrices ----------------------------------------------------------------------------------------------------------------

def csr_of(A, rng=None, stored=None):
    """(n, p, c, v) of a dense matrix: the entries `stored` (default: the non-zero ones), each row's in shuffled order under rng."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    stored = (A != 0.0) if stored is None else stored
    p, cols, vals = [0], [], []
    for i in range(n):
        j = np.flatnonzero(stored[i])
        if rng is not None:
            j = rng.permutation(j)
        cols.append(j)
        vals.append(A[i, j])
        p.append(p[-1] + len(j))
    cat = (lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt))
    return n, np.array(p, dtype=np.int32), cat(cols, np.int32), cat(vals, np.float64)


def poisson(k):
    """The 5-point Laplacian on a k x k grid, dense."""
    n = k * k
    A = np.zeros((n, n))
    for i in range(k):
        for j in range(k):
            r = i * k + j
            A[r, r] = 4.0
            for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                if 0 <= i + di < k and 0 <= j + dj < k:
                    A[r, (i + di) * k + j + dj] = -1.0
    return A


def sized(n):
    """The matrix of size n: every entry of a random matrix stored in shuffled order; 225: Poisson 15^2; 513: the first 513 rows
    and columns of Poisson 23^2."""
    rng = np.random.default_rng(4000 + n)
    if n == 225:
        return csr_of(poisson(15), rng)
    if n == 513:
        return csr_of(poisson(23)[:513, :513], rng)
    return csr_of(rng.uniform(-1.0, 1.0, size=(n, n)), rng, np.ones((n, n), dtype=bool))


def _poisson2d_coarse():
    rows, p, c, v = ac.matrix("poisson2D")
    co = a2.coarse("poisson2D")
    return len(co.row_ptr) - 1, co.row_ptr, co.column, co.values(v)


@functools.lru_cache(maxsize=1)
def grid_512_level_3():
    """The 376-row level of agg_mis2_cases.grid_512_hierarchy() as (n, p, c, v)."""
    rows, p, c, v = mc.grid(512, 512)
    for _ in range(3):
        agg, status = a2.aggregate(rows, p, c, v, 0.0, ac.SEEDS[0])
        pl = ac.Plan(rows, agg, status)
        co = ac.Coarse(pl, p, c)
        v = co.values(v)
        rows, p, c = pl.aggregates, co.row_ptr, co.column
    assert rows == a2.grid_512_hierarchy()[-1][0] == 376
    return rows, p, c, v


def _permutation():
    rng = np.random.default_rng(64)
    n = 64
    A = rng.uniform(-1e-3, 1e-3, size=(n, n))
    A[rng.permutation(n), np.arange(n)] += rng.choice([-1.0, 1.0], size=n)
    return csr_of(A, rng)


def _tie():
    # column 0 holds 2, -2, 2: row 0 stays; behind its step column 1 holds 3 and 3 in rows 1 and 2: row 1 stays
    return csr_of(np.array([[2.0, 1.0, 0.5], [-2.0, 2.0, 1.0], [2.0, 4.0, 3.0]]))


def _duplicates():
    rng = np.random.default_rng(17)
    n = 17
    A = rng.uniform(-1.0, 1.0, size=(n, n)) + 4.0 * np.eye(n)
    p, cols, vals = [0], [], []
    for i in range(n):
        entries = []
        for j in range(n):
            parts = 1 + (i + j) % 3
            share = rng.uniform(-1.0, 1.0, size=parts) * 10.0 ** rng.integers(-8, 8, size=parts)  # the order of a sum shows
            share[-1] = A[i, j] - np.sum(share[:-1])
            entries += [(j, s) for s in share]
        order = rng.permutation(len(entries))
        cols += [entries[o][0] for o in order]
        vals += [entries[o][1] for o in order]
        p.append(len(cols))
    return n, np.array(p, dtype=np.int32), np.array(cols, dtype=np.int32), np.array(vals, dtype=np.float64)


def _empty_row():
    A = np.triu(np.random.default_rng(5).uniform(1.0, 2.0, size=(5, 5)))
    A[2, :] = 0.0  # upper triangular: no row below offers a pivot for column 2
    return csr_of(A)


def _zero():
    return csr_of(np.zeros((4, 4)), None, np.eye(4, dtype=bool) | np.eye(4, k=1, dtype=bool))  # stored zeros


def _last_column():
    A = np.triu(np.ones((6, 6)))
    A[5, 5] = 0.0  # ones and zeros: every step is exact, and the last pivot is exactly 0
    return csr_of(A)


def _outside():
    rng = np.random.default_rng(9)
    n, p, c, v = csr_of(rng.uniform(-1.0, 1.0, size=(9, 9)) + 3.0 * np.eye(9), rng)
    cols, vals, q = [], [], [0]
    for i in range(n):
        extra = [-1, n, n + 5, -2 ** 31, 2 ** 31 - 1][:1 + i % 5]
        cc = np.concatenate([c[p[i]:p[i + 1]], extra])
        vv = np.concatenate([v[p[i]:p[i + 1]], rng.uniform(-1.0, 1.0, size=len(extra))])
        order = rng.permutation(len(cc))
        cols.append(cc[order])
        vals.append(vv[order])
        q.append(q[-1] + len(cc))
    return n, np.array(q, dtype=np.int32), np.concatenate(cols).astype(np.int32), np.concatenate(vals)


def _with(value):
    rng = np.random.default_rng(7)
    A = rng.uniform(-1.0, 1.0, size=(7, 7)) + 3.0 * np.eye(7)
    A[4, 2] = value
    return csr_of(A, rng)


def _spd_1e6():
    rng = np.random.default_rng(66)
    q, _ = np.linalg.qr(rng.normal(size=(64, 64)))
    A = (q * 10.0 ** np.linspace(0.0, 6.0, 64)) @ q.T
    return csr_of((A + A.T) / 2.0, rng, np.ones((64, 64), dtype=bool))


# name: (the matrix, [singular, column, skipped] as the header promises it, well-posed: compared with numpy.linalg.inv)
NAMED = {
    "poisson2D_Ac": (_poisson2d_coarse, [0, -1, 0], True),
    "grid_512_level_3": (grid_512_level_3, [0, -1, 0], True),
    "swap_2": (lambda: csr_of(np.array([[0.0, 1.0], [1.0, 0.0]])), [0, -1, 0], True),
    "permutation_64": (_permutation, [0, -1, 0], True),
    "tie": (_tie, [0, -1, 0], True),
    "duplicates_unsorted": (_duplicates, [0, -1, 0], True),
    "empty_row": (_empty_row, [1, 2, 0], False),
    "zero": (_zero, [1, 0, 0], False),
    "singular_last_column": (_last_column, [1, 5, 0], False),
    "columns_outside": (_outside, [0, -1, 25], True),
    "nan": (lambda: _with(np.nan), [0, -1, 0], False),
    "inf": (lambda: _with(np.inf), [0, -1, 0], False),
    "diagonal_1": (lambda: csr_of(np.array([[3.0]])), [0, -1, 0], True),
    "poisson_19": (lambda: csr_of(poisson(19)), [0, -1, 0], True),
    "spd_1e6": (_spd_1e6, [0, -1, 0], True),
}
CASES = tuple(NAMED) + tuple("size_%d" % n for n in SIZES)


@functools.lru_cache(maxsize=None)
def case(name):
    """(n, p, c, v, the promised status, well-posed)."""
    if name.startswith("size_"):
        n, p, c, v = sized(int(name[5:]))
        return n, p, c, v, [0, -1, 0], n > 0
    make, status, good = NAMED[name]
    n, p, c, v = make()
    return n, np.asarray(p, dtype=np.int32), np.asarray(c, dtype=np.int32), np.asarray(v, dtype=np.float64), status, good


@functools.lru_cache(maxsize=None)
def restated(name, dtype):
    """(inv, status) of the restatement for a case, once per process."""
    n, p, c, v, _, _ = case(name)
    return setup(n, p, c, v, dtype)


# ---- operands of the apply ---------------------------------------------------------------------------------------------------------

def int_operands(n, dtype):
    """(inv (n, ld), r, z): integers in +-{1 ... 8} (the inverse -2 ... 2): every product and every sum is exact in any order, and
    z a float holds (below 2^24)."""
    rng = np.random.default_rng(300 + n)
    ld = ld_of(n)
    inv = np.full((n, ld), 7, dtype=np.int64)  # what the padding holds must not matter
    inv[:, :n] = rng.integers(-2, 3, size=(n, n))
    r = rng.integers(1, 9, size=n) * rng.choice([-1, 1], size=n)
    z = inv[:, :n] @ r
    assert int(np.max(np.abs(z), initial=0)) < 2 ** 24
    return inv.astype(dtype), r.astype(dtype), z.astype(dtype)


def general_operands(n, dtype):
    """(inv (n, ld), r) uniform in (-1, 1), the padding columns NaN: never read into a sum."""
    rng = np.random.default_rng(500 + n)
    inv = np.full((n, ld_of(n)), np.nan)
    inv[:, :n] = rng.uniform(-1.0, 1.0, size=(n, n))
    return inv.astype(dtype), rng.uniform(-1.0, 1.0, size=n).astype(dtype)


def banded_2048():
    """(n, p, c, v, dense): 2048 rows, seven diagonals, strictly diagonally dominant; sorted columns."""
    n = MAX_N
    rng = np.random.default_rng(2048)
    A = np.zeros((n, n))
    for k in (-3, -2, -1, 1, 2, 3):
        A += np.diag(rng.uniform(-1.0, 1.0, size=n - abs(k)), k)
    A += np.diag((np.sum(np.abs(A), axis=1) + 1.0) * rng.choice([-1.0, 1.0], size=n))
    return csr_of(A) + (A,)
