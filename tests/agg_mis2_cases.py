"""The two contracts of include/spmv_hip_agg_mis2.h restated in numpy: the aggregates of a distance-2 independent set and the
restriction by a group of lanes per aggregate (test_agg_mis2_cases.py holds the restatement to its properties without a device;
test_gpu_agg_mis2.py holds the GPU to the restatement bit for bit).  Matrices, neighbours, keys, Plan and Coarse are those of
agg_cases.py and mcgs_cases.py.

aggregate() runs the rounds over all rows at once from the state of the round's start: t1 is the largest key among the undecided
rows of a row and its neighbours, t2 the largest t1 over a row and its neighbours -- every row relays, whatever its state -- an
undecided row whose own key is its t2 wins, and an undecided row within two steps of a winner is covered.  Behind the rounds a row
beside a root joins the root beside it with the largest key (pass 1), and every other row the root that one of its neighbours
joined in pass 1, the largest key among those roots (pass 2).  restrict_group() gives lane l of `group` lanes the members l, l +
group, ... of an aggregate, added left to right from +0.0, and adds the lanes by the butterfly p += p[lane ^ step], step = 1, 2,
... group / 2, every numpy operation rounding on its own and one cast to the vectors' type last."""
import functools

import numpy as np

import agg_cases as ac
import mcgs_cases as mc
from spmv_amd.capi import agg_aggregate_mis2, agg_group, agg_mis2_workspace_bytes, agg_restrict_group  # noqa: F401  (no feature, no cases)

GROUPS = (1, 2, 4, 8, 16, 32, 64)
UNDECIDED, COVERED, ROOT = ac.UNDECIDED, ac.COVERED, ac.ROOT
# Eight PCG iterations on poisson2D.mtx from x = 0 with b = ones (r0'r0 = 367), agg_cases.pcg() on the CPU in doubles: r'r 6.722e-03
# with agg_cases.two_level_cycle() at omega 1 over the 38 distance-2 aggregates of the first seed and a dense coarse solve
# (1.050e-02 at omega 1.5), 127.8 with the diagonal: a ratio of 5.26e-05 (8.22e-05 at omega 1.5).  Asserted: a hundred times the
# measured ratio at omega 1 -- the GPU's cycle differs from this one by roundings alone.  Larger plain aggregates correct less per
# cycle than the distance-1 ones (agg_cases.PCG_FACTOR: 4.7e-08 measured there).
PCG_FACTOR = 5.26e-3


# ---- the restatement: aggregation ------------------------------------------------------------------------------------------------

def aggregate(rows, p, c, v, theta, seed):
    """(agg, [aggregates, rounds, the largest aggregate, singletons])."""
    return aggregate_and_roots(rows, p, c, v, theta, seed)[:2]


def aggregate_and_roots(rows, p, c, v, theta, seed):
    """(agg, status, the root row every row joined: itself for a root)."""
    row, col = ac.neighbours(rows, p, c, v, theta)
    key = mc.keys(rows, seed) + np.uint64(1)  # 0 stands for "none"
    state = np.full(rows, UNDECIDED, dtype=np.int32)
    rounds = 0
    while np.any(state == UNDECIDED):
        open_ = state == UNDECIDED
        t1 = np.where(open_, key, np.uint64(0))
        np.maximum.at(t1, row[open_[col]], key[col[open_[col]]])
        t2 = t1.copy()
        np.maximum.at(t2, row, t1[col])
        win = open_ & (t2 == key)
        assert win.any()
        n1 = win.copy()
        n1[row[win[col]]] = True
        n2 = n1.copy()
        n2[row[n1[col]]] = True
        state[open_ & ~win & n2] = COVERED
        state[win] = ROOT
        rounds += 1
    root = state == ROOT
    number = (np.cumsum(root) - root).astype(np.int64)
    # pass 1: a row beside a root joins the root beside it with the largest key
    joins = np.where(root, np.arange(rows, dtype=np.int64), -1)
    to_root = root[col] & ~root[row]
    best = np.zeros(rows, dtype=np.uint64)
    np.maximum.at(best, row[to_root], key[col[to_root]])
    first = np.zeros(rows, dtype=bool)
    first[row[to_root]] = True
    joins[first] = ((best[first] - np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    # pass 2: every other row joins the root that a neighbour joined in pass 1, the largest key among those roots
    rest = ~root & ~first
    through = rest[row] & first[col]
    best = np.zeros(rows, dtype=np.uint64)
    np.maximum.at(best, row[through], key[joins[col[through]]])
    second = np.zeros(rows, dtype=bool)
    second[row[through]] = True
    assert np.all(second[rest])  # a covered row is within two steps of a root, through a row that is beside that root
    joins[rest] = ((best[rest] - np.uint64(1)) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    agg = number[joins].astype(np.int32)
    sizes = np.bincount(agg, minlength=int(root.sum())) if rows else np.zeros(0, dtype=np.int64)
    status = [int(root.sum()), rounds, int(sizes.max()) if rows else 0, int(np.sum(sizes == 1))]
    return agg, status, joins


@functools.lru_cache(maxsize=None)
def plan(name, seed=ac.SEEDS[0], theta=0.0):
    rows, p, c, v = ac.matrix(name)
    agg, status = aggregate(rows, p, c, v, theta, seed)
    return ac.Plan(rows, agg, status), status


@functools.lru_cache(maxsize=None)
def coarse(name):
    rows, p, c, v = ac.matrix(name)
    return ac.Coarse(plan(name)[0], p, c)


def hierarchy(rows, p, c, v, floor, seed=ac.SEEDS[0], levels=20):
    """[(rows, stored entries, status of the aggregation that made the next level or None)] down to <= floor rows."""
    out = []
    while True:
        if rows <= floor or len(out) + 1 >= levels:
            out.append((rows, len(c), None))
            return out
        agg, status = aggregate(rows, p, c, v, 0.0, seed)
        out.append((rows, len(c), status))
        pl = ac.Plan(rows, agg, status)
        co = ac.Coarse(pl, p, c)
        v = co.values(v)
        rows, p, c = pl.aggregates, co.row_ptr, co.column


@functools.lru_cache(maxsize=None)
def grid_512_hierarchy():
    return hierarchy(*mc.grid(512, 512), 1000)


# ---- the restatement: the grouped restriction --------------------------------------------------------------------------------------

def group_of(rows, aggregates):
    """spmv_hip_agg_group: the smallest power of two >= rows / aggregates, inside 1 ... 64."""
    g = 1
    while g < 64 and g * aggregates < rows:
        g *= 2
    return g


def restrict_group(pl, group, r, dtype):
    """r_c[I] = fl_T(the butterfly over the lanes' sums), lane l adding the members l, l + group, ... from +0.0 in doubles."""
    r64 = np.asarray(r, dtype=dtype).astype(np.float64)
    start, length = pl.member_ptr[:-1].astype(np.int64), np.diff(pl.member_ptr.astype(np.int64))
    part = np.zeros((pl.aggregates, group))
    lane = np.arange(group)[None, :]
    trips = -(-int(length.max()) // group) if pl.aggregates else 0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(trips):
            at = lane + t * group
            live = at < length[:, None]
            m = pl.member[np.where(live, start[:, None] + at, 0)]
            part = np.where(live, part + r64[m], part)  # a member that is not there adds nothing, and is not read
        step = 1
        while step < group:
            part = part + part[:, np.arange(group) ^ step]
            step *= 2
        return part[:, 0].astype(dtype) if pl.aggregates else np.zeros(0, dtype=dtype)
