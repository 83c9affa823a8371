"""Matrices for the tests of the aggregation multigrid level (include/spmv_hip_agg.h) and the header's contract restated in numpy
(test_agg_cases.py holds the restatement to the dense P'AP and to a partition of the rows without a device; test_gpu_agg.py holds
the GPU to the restatement bit for bit on the same matrices).

The restatement: aggregate() runs the rounds over all rows at once -- the winners of a round are found from the state of the
round's start, then the rows beside a root or a winner are covered -- and joins every covered row to the root beside it with the
largest key; Plan is a stable sort of the rows by aggregate; Coarse is a stable sort of the stored entries by (agg[row],
agg[column]); Coarse.values(), restrict() and prolong_add() add in the header's order, every numpy operation rounding on its own
and one cast to the vectors' type last."""
import functools

import numpy as np

import mcgs_cases as mc
from spmv_amd.capi import agg_aggregate, agg_plan, agg_prolong_add, agg_restrict  # noqa: F401  (no feature, no matrices)

DTYPES = mc.DTYPES
SEEDS = mc.SEEDS
THETAS = (0.0, 0.25)
OMEGAS = (1.0, 1.5, -0.5)
SIZES = (0, 1, 2, 4099)
ITERATIONS = 8
UNDECIDED, COVERED, ROOT = -1, -2, -3
# Eight PCG iterations on poisson2D.mtx from x = 0 with b = ones (r0'r0 = 367), this file's pcg() on the CPU in doubles:
# r'r 6.01e-06 with two_level_cycle() at omega 1 over the 94 aggregates of the first seed and a dense coarse solve (1.20e-05 at
# omega 1.5), 127.8 with the diagonal: a ratio of 4.7e-08.  Asserted: ten thousand times below the diagonal, which leaves the
# measured ratio a factor of 2000 -- the GPU's cycle differs from this one by roundings alone.
PCG_FACTOR = 1e-4


# ---- matrices --------------------------------------------------------------------------------------------------------------------

def star(leaves, seed=SEEDS[0]):
    """One row coupled both ways to `leaves` others, 2 on the diagonal and -1/leaves ... beside it; the hub is the row whose key
    is the largest under `seed`, so that under that seed every row joins it: one aggregate."""
    import scipy.sparse as sp
    rows = leaves + 1
    hub = int(np.argmax(mc.keys(rows, seed)))
    others = np.setdiff1d(np.arange(rows), [hub])
    w = -(1.0 + (others % 7)) / 8.0
    i = np.arange(rows)
    A = sp.csr_matrix((np.concatenate([2.0 + i % 3, w, w]),
                       (np.concatenate([i, np.full(leaves, hub), others]), np.concatenate([i, others, np.full(leaves, hub)]))), shape=(rows, rows))
    A.sort_indices()
    return mc._csr(rows, A.indptr, A.indices, A.data)


def isolated():
    """A 19 x 13 grid with rows 0, 57 and 58 and the last row emptied of everything and rows 5, 100 and 101 of everything but their
    diagonal -- with the columns that pointed at them, so the pattern stays symmetric."""
    rows, p, c, v = mc.grid(19, 13)
    empty, alone = {0, 57, 58, rows - 1}, {5, 100, 101}
    gone = empty | alone
    out_p, out_c, out_v = [0], [], []
    for i in range(rows):
        for j, a in zip(c[p[i]:p[i + 1]], v[p[i]:p[i + 1]]):
            if (i not in gone and j not in gone) or (j == i and i in alone):
                out_c.append(j)
                out_v.append(a)
        out_p.append(len(out_c))
    return mc._csr(rows, out_p, out_c, out_v)


GENERATORS = {name: mc.GENERATORS[name] for name in ("poisson2D", "bus1138_like", "grid_37x29", "grid_13x13x13", "ragged", "long_row")}
GENERATORS.update({"clique_66": lambda: mc.clique(66), "one_sided": mc.one_sided})
GENERATORS.update({"path_%d" % n: (lambda n=n: mc.path(n)) for n in (0, 1, 2, 4099)})
GENERATORS.update({"star_5000": lambda: star(5000), "isolated": isolated})
MATRICES = tuple(GENERATORS)


@functools.lru_cache(maxsize=None)
def matrix(name):
    return GENERATORS[name]()


def general_values(name):
    """The matrix's values replaced by doubles that no float holds, seeded by the name: what the numeric product is held to."""
    rows, p, c, v = matrix(name)
    return np.random.default_rng(len(name) + 41).uniform(-1.0, 1.0, size=len(v))


# ---- the restatement: aggregation ------------------------------------------------------------------------------------------------

def neighbours(rows, p, c, v, theta):
    """(row, column) of the stored entries that make their column a neighbour of their row, in stored order."""
    p64, c64 = np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int64)
    row = np.repeat(np.arange(rows, dtype=np.int64), np.diff(p64))
    off = c64 != row
    if v is not None and theta > 0.0:
        a = np.abs(np.asarray(v, dtype=np.float64))
        largest = np.zeros(rows)
        np.maximum.at(largest, row[off], a[off])
        off &= a >= (theta * largest)[row]
    return row[off], c64[off]


def aggregate(rows, p, c, v, theta, seed):
    """(agg, [aggregates, rounds, the largest aggregate, singletons])."""
    return aggregate_and_roots(rows, p, c, v, theta, seed)[:2]


def aggregate_and_roots(rows, p, c, v, theta, seed):
    """(agg, status, the row every row joined: itself for a root)."""
    row, col = neighbours(rows, p, c, v, theta)
    key = mc.keys(rows, seed)
    state = np.full(rows, UNDECIDED, dtype=np.int32)
    rounds = 0
    while np.any(state == UNDECIDED):
        open_ = state == UNDECIDED
        both = open_[row] & open_[col]
        lost = np.zeros(rows, dtype=bool)
        lost[row[both & (key[col] > key[row])]] = True
        win = open_ & ~lost
        assert win.any()
        beside = np.zeros(rows, dtype=bool)
        beside[row[win[col] | (state[col] == ROOT)]] = True
        state[open_ & ~win & beside] = COVERED
        state[win] = ROOT
        rounds += 1
    root = state == ROOT
    number = (np.cumsum(root) - root).astype(np.int64)
    joins = np.arange(rows, dtype=np.int64)
    to_root = root[col] & ~root[row]
    best = np.zeros(rows, dtype=np.uint64)
    found = np.zeros(rows, dtype=bool)
    np.maximum.at(best, row[to_root], key[col[to_root]])
    found[row[to_root]] = True
    assert np.all(found[~root])  # a covered row has a root beside it
    joins[~root] = (best[~root] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    agg = number[joins].astype(np.int32)
    sizes = np.bincount(agg, minlength=int(root.sum())) if rows else np.zeros(0, dtype=np.int64)
    status = [int(root.sum()), rounds, int(sizes.max()) if rows else 0, int(np.sum(sizes == 1))]
    return agg, status, joins


class Plan:
    """What spmv_hip_agg_plan fills, on the host."""

    def __init__(self, rows, agg, status):
        self.rows, self.aggregates, self.largest = rows, status[0], status[2]
        self.agg = np.asarray(agg, dtype=np.int32)
        self.member = np.argsort(self.agg, kind="stable").astype(np.int32)
        self.member_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.agg, minlength=self.aggregates))]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def plan(name, seed=SEEDS[0], theta=0.0):
    rows, p, c, v = matrix(name)
    agg, status = aggregate(rows, p, c, v, theta, seed)
    return Plan(rows, agg, status), status


# ---- the restatement: the Galerkin product ---------------------------------------------------------------------------------------

class Coarse:
    """What spmv_hip_agg_galerkin_symbolic writes: the pattern of A_c and the runs of its entries."""

    def __init__(self, pl, p, c):
        p64, c64 = np.asarray(p, dtype=np.int64), np.asarray(c, dtype=np.int64)
        row = np.repeat(np.arange(pl.rows, dtype=np.int64), np.diff(p64))
        a = pl.agg.astype(np.int64)
        key = a[row] * max(pl.aggregates, 1) + a[c64] if len(c64) else np.zeros(0, dtype=np.int64)
        self.order = np.argsort(key, kind="stable").astype(np.int32)
        skey = key[self.order]
        head = np.ones(len(skey), dtype=bool)
        head[1:] = skey[1:] != skey[:-1]
        at = np.flatnonzero(head)
        self.nnz, self.nnz_c = len(c64), len(at)
        self.entry_ptr = np.concatenate([at, [self.nnz]]).astype(np.int32)
        self.column = (skey[at] % max(pl.aggregates, 1)).astype(np.int32)
        per_row = np.bincount(skey[at] // max(pl.aggregates, 1), minlength=pl.aggregates) if self.nnz_c else np.zeros(pl.aggregates, dtype=np.int64)
        self.row_ptr = np.concatenate([[0], np.cumsum(per_row)]).astype(np.int32)

    def values(self, v):
        """The fine values of every run added left to right from +0.0."""
        v = np.asarray(v, dtype=np.float64)
        start, length = self.entry_ptr[:-1].astype(np.int64), np.diff(self.entry_ptr.astype(np.int64))
        out = np.zeros(self.nnz_c)
        live = np.arange(self.nnz_c)
        t = 0
        with np.errstate(invalid="ignore", over="ignore"):
            while len(live):
                out[live] = out[live] + v[self.order[start[live] + t]]
                t += 1
                live = live[length[live] > t]
        return out

    def bound(self, v):
        """run 2^-53 sum |t| of every coarse entry: what two orders of its sum may differ by."""
        v = np.abs(np.asarray(v, dtype=np.float64))
        mag = np.add.reduceat(v[self.order], self.entry_ptr[:-1].astype(np.int64)) if self.nnz_c else np.zeros(0)
        return np.diff(self.entry_ptr.astype(np.int64)) * 2.0 ** -53 * mag

    def dense(self, cv):
        out = np.zeros((len(self.row_ptr) - 1,) * 2)
        rows = np.repeat(np.arange(len(self.row_ptr) - 1), np.diff(self.row_ptr))
        out[rows, self.column] = cv
        return out


@functools.lru_cache(maxsize=None)
def coarse(name):
    rows, p, c, v = matrix(name)
    return Coarse(plan(name)[0], p, c)


def dense_galerkin(pl, rows, p, c, v):
    """P' A P formed densely, in the order numpy takes."""
    import scipy.sparse as sp
    A = sp.csr_matrix((np.asarray(v, dtype=np.float64), c, p), shape=(rows, rows))
    P = sp.csr_matrix((np.ones(rows), (np.arange(rows), pl.agg)), shape=(rows, max(pl.aggregates, 0)))
    return (P.T @ A @ P).toarray()


# ---- the restatement: restriction and prolongation ---------------------------------------------------------------------------------

def restrict(pl, r, dtype):
    """r_c[I] = fl_T(((+0.0 + r[m_0]) + r[m_1]) + ...), the sums in doubles."""
    r64 = np.asarray(r, dtype=dtype).astype(np.float64)
    start, length = pl.member_ptr[:-1].astype(np.int64), np.diff(pl.member_ptr.astype(np.int64))
    out = np.zeros(pl.aggregates)
    live = np.arange(pl.aggregates)
    t = 0
    with np.errstate(invalid="ignore", over="ignore"):
        while len(live):
            out[live] = out[live] + r64[pl.member[start[live] + t]]
            t += 1
            live = live[length[live] > t]
        return out.astype(dtype)


def prolong_add(pl, omega, ec, x, dtype):
    """x_i + fl(omega e_c[agg[i]]), one rounding to the vectors' type last."""
    with np.errstate(invalid="ignore", over="ignore"):
        e64 = np.asarray(ec, dtype=dtype).astype(np.float64)[pl.agg] if pl.rows else np.zeros(0)
        return (np.asarray(x, dtype=dtype).astype(np.float64) + np.float64(omega) * e64).astype(dtype)


def blocks(n, width):
    """A plan over n rows without a matrix: aggregates of 1 ... width consecutive rows, the widths cycling."""
    agg, i, k = np.zeros(n, dtype=np.int32), 0, 0
    while i < n:
        w = 1 + k % width
        agg[i:i + w] = k
        i, k = i + w, k + 1
    sizes = np.bincount(agg) if n else np.zeros(0, dtype=np.int64)
    return Plan(n, agg, [len(sizes), 0, int(sizes.max()) if n else 0, int(np.sum(sizes == 1))])


# ---- the two-level cycle and eight PCG iterations ----------------------------------------------------------------------------------

SMOOTH = 2.0 / 3.0  # the damping of the Jacobi smoother: minv is stored scaled by it


def smoother_of(rows, p, c, v, dtype):
    """fl_T(fl(2/3) fl(1 / a_ii)): the array the cycle's two smoothing steps multiply by."""
    return (SMOOTH * mc.minv_of(rows, p, c, v, np.float64)).astype(dtype)


def two_level_cycle(A, pl, minv, solve, omega):
    """r -> z: z = minv r; z += omega P solve(P' (r - A z)); z += minv (r - A z): damped Jacobi before and behind the correction."""

    def cycle(r):
        z = minv * r
        rc = restrict(pl, r - A @ z, np.float64)
        z = prolong_add(pl, omega, solve(rc), z, np.float64)
        return z + minv * (r - A @ z)

    return cycle


def pcg(rows, p, c, v, b, precondition, iterations=ITERATIONS):
    return mc.pcg(rows, p, c, v, b, precondition, iterations)
