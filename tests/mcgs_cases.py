"""Matrices for the tests of the multicolour Gauss-Seidel / SSOR preconditioner (include/spmv_hip_mcgs.h) and the header's
contract restated in numpy (test_mcgs_cases.py holds the restatement to a plain sequential SOR without a device;
test_gpu_mcgs.py holds the GPU to the restatement bit for bit on the same matrices).

The restatement: colour() is Jones-Plassmann with first fit in rounds that read the state of the round's start -- the winners of
a round are found first, then coloured from the rows that did not win -- over all rows at once; permute() is a stable sort by
colour; sweep() sums, for every row of a colour at once, the products of lane l of `group` lanes over the entries l, l + group,
... in stored order from +0.0, adds the lanes by the butterfly p += p[lane ^ step], step = group / 2 ... 1, and updates x with
every numpy operation rounding on its own and one cast to the vectors' type last; apply() is the zeroed z swept forwards and
backwards."""
import functools
import os

import numpy as np

from spmv_amd.capi import mcgs_apply, mcgs_colour, mcgs_permute, mcgs_sweep  # noqa: F401  (no feature, no matrices)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DTYPES = (np.float64, np.float32)
GROUPS = (1, 2, 4, 8, 16, 32, 64)
OMEGAS = (1.0, 0.5, 1.5)
SEEDS = (0, 0x9E3779B9)
MAX_COLOURS = 64
ITERATIONS = 8


def _csr(rows, p, c, v):
    return (int(rows), np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64))


# ---- matrices --------------------------------------------------------------------------------------------------------------------

def _golden(name):
    """A Matrix Market file of tests/golden as the full matrix (a `symmetric` file expanded), rows sorted by column."""
    import scipy.io
    A = scipy.io.mmread(os.path.join(GOLDEN, name)).tocsr()
    A.sort_indices()
    return _csr(A.shape[0], A.indptr, A.indices, A.data)


def grid(*shape):
    """The 5-point (two sizes) or 7-point (three sizes) stencil: 2 d on the diagonal, -1 beside it."""
    import scipy.sparse as sp
    d = len(shape)
    A = sp.csr_matrix((1, 1))
    for k, n in enumerate(shape):
        T = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
        parts = [sp.identity(m) for m in shape]
        parts[k] = T
        K = parts[0]
        for q in parts[1:]:
            K = sp.kron(K, q)
        A = K if k == 0 else A + K
    A = A.tocsr()
    A.sort_indices()
    assert A.nnz == sum(2 * (n - 1) * int(np.prod(shape)) // n for n in shape) + int(np.prod(shape)) and d in (2, 3)
    return _csr(A.shape[0], A.indptr, A.indices, A.data)


def path(rows):
    """A path graph: 2 on the diagonal, -1 beside it; rows == 0 and rows == 1 are the matrices without a neighbour."""
    if rows == 0:
        return _csr(0, np.zeros(1), np.zeros(0), np.zeros(0))
    i = np.arange(rows)
    r = np.concatenate([i, i[1:], i[:-1]])
    c = np.concatenate([i, i[:-1], i[1:]])
    v = np.concatenate([2.0 * np.ones(rows), -np.ones(rows - 1), -np.ones(rows - 1)])
    import scipy.sparse as sp
    A = sp.csr_matrix((v, (r, c)), shape=(rows, rows))
    A.sort_indices()
    return _csr(rows, A.indptr, A.indices, A.data)


def _ragged():
    """A 23 x 17 grid with every row's entries shuffled, an entry of every fifth row stored twice (half the value each), rows 3,
    40 and 41 emptied of everything and rows 7 and 200 of everything but their diagonal -- with the columns that pointed at
    them, so the pattern stays symmetric."""
    rows, p, c, v = grid(23, 17)
    rng = np.random.default_rng(11)
    gone = {3, 40, 41, 7, 200}
    out_p, out_c, out_v = [0], [], []
    for i in range(rows):
        cols, vals = list(c[p[i]:p[i + 1]]), list(v[p[i]:p[i + 1]])
        keep = [(j, a) for j, a in zip(cols, vals) if (i not in gone and j not in gone) or (j == i and i in (7, 200))]
        if i % 5 == 0 and len(keep) > 1:
            j, a = keep[-1]
            keep[-1] = (j, a / 2)
            keep.append((j, a / 2))
        order = rng.permutation(len(keep))
        out_c += [keep[k][0] for k in order]
        out_v += [keep[k][1] for k in order]
        out_p.append(len(out_c))
    return _csr(rows, out_p, out_c, out_v)


def _long_row():
    """A 37 x 29 grid whose row 500 couples to 199 further rows (a row of 200 entries and more, and its mirror column)."""
    import scipy.sparse as sp
    rows, p, c, v = grid(37, 29)
    A = sp.csr_matrix((v, c, p), shape=(rows, rows)).tolil()
    far = np.random.default_rng(5).choice(np.setdiff1d(np.arange(rows), [499, 500, 501, 500 - 29, 500 + 29]), size=199, replace=False)
    for j in far:
        A[500, j] = -0.01
        A[j, 500] = -0.01
    A = A.tocsr()
    A.sort_indices()
    return _csr(rows, A.indptr, A.indices, A.data)


def clique(n):
    """Every row stores every column: n colours are needed."""
    p = np.arange(n + 1) * n
    c = np.tile(np.arange(n), n)
    v = np.where(c == np.repeat(np.arange(n), n), float(n), -0.5)
    return _csr(n, p, c, v)


def one_sided():
    """A 9 x 7 grid with (5, 6) stored and (6, 5) not: the pattern is not symmetric."""
    rows, p, c, v = grid(9, 7)
    row = np.repeat(np.arange(rows), np.diff(p))
    keep = ~((row == 6) & (c == 5))
    return _csr(rows, np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=rows))]), c[keep], v[keep])


GENERATORS = {
    "poisson2D": lambda: _golden("poisson2D.mtx"),
    "bus1138_like": lambda: _golden("bus1138_like.mtx"),
    "grid_37x29": lambda: grid(37, 29),
    "grid_13x13x13": lambda: grid(13, 13, 13),
    "ragged": _ragged,
    "long_row": _long_row,
}
GENERATORS.update({"path_%d" % n: (lambda n=n: path(n)) for n in (0, 1, 63, 64, 65, 1025, 4099)})
COLOURING = tuple(n for n in GENERATORS if n != "long_row")  # what the issue lists for the colouring
SWEEPS = tuple(GENERATORS)                                    # ... and for the sweep: those and the row of 200 entries


@functools.lru_cache(maxsize=None)
def matrix(name):
    return GENERATORS[name]()


# ---- the restatement: colouring --------------------------------------------------------------------------------------------------

def fmix32(h):
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85ebca6b)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xc2b2ae35)
    h ^= h >> np.uint32(16)
    return h


def keys(rows, seed):
    """The pair (fmix32(i ^ seed), i) as one 64-bit integer: comparing them compares the pairs lexicographically."""
    i = np.arange(rows, dtype=np.uint32)
    return (fmix32(i ^ np.uint32(seed)).astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)


def colour(rows, p, c, seed):
    """(colour, [colours, rounds, conflicts, overflowed rows])."""
    p64, c64 = np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int64)
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(p64))
    off = c64 != row
    row, col = row[off], c64[off]
    key = keys(rows, seed)
    col_of = np.full(rows, -1, dtype=np.int32)
    rounds = overflowed = 0
    while np.any(col_of < 0):
        start = col_of.copy()
        open_ = start < 0
        both = open_[row] & open_[col]
        lost = np.zeros(rows, dtype=bool)
        lost[row[both & (key[col] > key[row])]] = True
        win = open_ & ~lost
        assert win.any()
        seen = win[row] & ~win[col] & (start[col] >= 0)
        held = np.zeros(rows, dtype=np.uint64)
        np.bitwise_or.at(held, row[seen], np.uint64(1) << start[col[seen]].astype(np.uint64))
        free = ~held[win]
        full = free == 0
        low = free & (~free + np.uint64(1))  # the lowest set bit
        first = np.where(full, MAX_COLOURS - 1, np.log2(np.where(full, 1, low).astype(np.float64)).astype(np.int64))
        overflowed += int(full.sum())
        col_of[win] = first.astype(np.int32)
        rounds += 1
    conflicts = int(np.sum(col_of[row] == col_of[col]))
    colours = int(col_of.max()) + 1 if rows else 0
    return col_of, [colours, rounds, conflicts, overflowed]


# ---- the restatement: the plan ---------------------------------------------------------------------------------------------------

def default_group(rows, nnz):
    g = 4
    while g < 64 and g * rows < nnz:
        g *= 2
    return g


class Plan:
    """What spmv_hip_mcgs_permute fills, on the host."""

    def __init__(self, rows, p, c, v, col_of, status):
        p64 = np.asarray(p, dtype=np.int64)
        self.rows, self.colours, self.conflicts = rows, status[0], status[2]
        self.order = np.argsort(col_of, kind="stable").astype(np.int32)
        count = np.bincount(col_of, minlength=MAX_COLOURS) if rows else np.zeros(MAX_COLOURS, dtype=np.int64)
        self.colour_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
        lens = np.diff(p64)[self.order]
        self.p = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        src = (np.repeat(p64[:-1][self.order] - self.p[:-1], lens) + np.arange(int(lens.sum()))).astype(np.int64)
        self.c, self.v = np.asarray(c)[src].astype(np.int32), np.asarray(v)[src].astype(np.float64)
        self.group = default_group(rows, len(self.c))


@functools.lru_cache(maxsize=None)
def plan(name, seed=SEEDS[0]):
    rows, p, c, v = matrix(name)
    col_of, status = colour(rows, p, c, seed)
    return Plan(rows, p, c, v, col_of, status), col_of, status


# ---- the restatement: the sweep --------------------------------------------------------------------------------------------------

def sweep_colour(pl, colour_index, omega, b, minv, x, dtype, group):
    """x with the rows of one colour updated; x, b, minv in `dtype`."""
    k0, k1 = int(pl.colour_ptr[colour_index]), int(pl.colour_ptr[colour_index + 1])
    if k1 == k0:
        return x
    rows_k = pl.order[k0:k1].astype(np.int64)
    start, lens = pl.p[k0:k1].astype(np.int64), np.diff(pl.p[k0:k1 + 1].astype(np.int64))
    trips = max(1, -(-int(lens.max()) // group))
    xs = x.astype(np.float64)
    part = np.zeros((k1 - k0, group))
    lane = np.arange(group)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(trips):
            e = lane + t * group                      # the entry of every lane in this trip
            live = e < lens[:, None]
            at = np.where(live, start[:, None] + e, 0)
            if len(pl.c) == 0:
                break
            j = pl.c[at].astype(np.int64)
            live &= j != rows_k[:, None]
            prod = pl.v[at] * xs[j]
            part = np.where(live, part + prod, part)  # an entry that is not there, or the diagonal, adds nothing
        step = group // 2
        while step >= 1:
            part = part + part[:, np.arange(group) ^ step]
            step //= 2
        s = part[:, 0]
        t = omega * (minv[rows_k].astype(np.float64) * (b[rows_k].astype(np.float64) - s))
        out = x.copy()
        out[rows_k] = ((1.0 - omega) * xs[rows_k] + t).astype(dtype)
    return out


def sweep(pl, first, last, omega, b, minv, x, dtype, group=None):
    group = group or pl.group
    step = -1 if last < first else 1
    x = np.asarray(x, dtype=dtype).copy()
    for ci in range(first, last + step, step):
        x = sweep_colour(pl, ci, omega, b, minv, x, dtype, group)
    return x


def apply(pl, omega, r, minv, dtype, group=None):
    z = np.zeros(pl.rows, dtype=dtype)
    if pl.colours == 0:
        return z
    z = sweep(pl, 0, pl.colours - 1, omega, r, minv, z, dtype, group)
    return sweep(pl, pl.colours - 1, 0, omega, r, minv, z, dtype, group)


def apply_products(z, r):
    """(t0, t1): the rounded products of the apply's dots over z as stored."""
    z, r = np.asarray(z).astype(np.float64), np.asarray(r).astype(np.float64)
    return z * r, z * z


def minv_of(rows, p, c, v, dtype):
    """The b == 1 array of spmv_hip_bjacobi_setup_*: fl(1 / a_ii), the diagonal entries added in stored order; 1 where there is
    none or it is zero."""
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(np.asarray(p, dtype=np.int64)))
    d = np.zeros(rows)
    on = np.asarray(c) == row
    np.add.at(d, row[on], np.asarray(v)[on])
    with np.errstate(divide="ignore"):
        return np.where(d == 0.0, 1.0, 1.0 / d).astype(dtype)


# ---- a plain sequential SOR, row after row in the plan's order -------------------------------------------------------------------

def sequential_sor(pl, first, last, omega, b, minv, x, dtype):
    """(x, bound): rows visited one after the other in the order of the plan's colours first ... last, every row reading the x of
    the moment, its sum added left to right; bound[i] is what two summation orders of row i's products and the last roundings
    may differ by, were they given the same x."""
    step = -1 if last < first else 1
    x = np.asarray(x, dtype=dtype).copy()
    bound = np.zeros(pl.rows)
    u = 2.0 ** -53
    for ci in range(first, last + step, step):
        for k in range(int(pl.colour_ptr[ci]), int(pl.colour_ptr[ci + 1])):
            i = int(pl.order[k])
            s = mag = 0.0
            n = 0
            for e in range(int(pl.p[k]), int(pl.p[k + 1])):
                j = int(pl.c[e])
                if j != i:
                    t = pl.v[e] * float(x[j])
                    s, mag, n = s + t, mag + abs(t), n + 1
            new = (1.0 - omega) * float(x[i]) + omega * (float(minv[i]) * (float(b[i]) - s))
            bound[i] = omega * abs(float(minv[i])) * n * u * mag * (1.0 + 8 * u) + 4 * u * abs(new)
            if np.dtype(dtype) == np.float32:
                bound[i] += 2.0 ** -23 * abs(new)
            x[i] = new
    return x, bound


# ---- eight PCG iterations, every vector operation restated -------------------------------------------------------------------------

def pcg(rows, p, c, v, b, precondition, iterations=ITERATIONS):
    """r'r after each of `iterations` iterations of PCG in doubles from x = 0; precondition(r) -> z."""
    import scipy.sparse as sp
    A = sp.csr_matrix((v, c, p), shape=(rows, rows))
    x, r = np.zeros(rows), np.asarray(b, dtype=np.float64).copy()
    z = precondition(r)
    d = z.copy()
    rz = float(r @ z)
    out = []
    for _ in range(iterations):
        q = A @ d
        a = rz / float(d @ q)
        x, r = x + a * d, r - a * q
        out.append(float(r @ r))
        z = precondition(r)
        rz_new = float(r @ z)
        d = z + (rz_new / rz) * d
        rz = rz_new
    return out
