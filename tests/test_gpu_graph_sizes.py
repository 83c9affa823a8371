"""The graph set-ups past 65 536 rows and 65 536 aggregates on the MI355X (graph_size_cases.py says which matrix is there for which
edge): spmv_hip_mcgs_colour, spmv_hip_mcgs_permute and a symmetric sweep over their plan; spmv_hip_agg_aggregate,
spmv_hip_agg_aggregate_mis2, spmv_hip_agg_plan, spmv_hip_agg_galerkin_{symbolic,numeric}, the restrictions and the prolongation; the
four distance-1 levels of the 512 x 512 grid on the arrays the device product left; and the first coarse matrix of that hierarchy as
the operand of spmv_hip_plan_csr and of the colouring.

Every array is compared as integers or bit for bit with the numpy restatements of mcgs_cases.py, agg_cases.py and agg_mis2_cases.py
(none of these calls adds floating-point numbers in atomics); the one multiply is held to the oracle by helpers.assert_close.
The device harnesses are those of test_gpu_mcgs.py, test_gpu_agg.py and test_gpu_agg_mis2.py: every device array lies between
guards that are checked whenever it is read back.  The restated cases are made once per process (graph_size_cases)."""
import functools

import numpy as np
import pytest

import agg_cases as ac
import agg_mis2_cases as a2
import graph_size_cases as gs
import helpers
import mcgs_cases as mc
import test_gpu_mcgs as gm
from spmv_amd import capi
from test_gpu_agg import HostPlan, Level, _body, _ints, _t
from test_gpu_agg_mis2 import Level2
from test_gpu_krylov import Band
from test_gpu_mcgs import Apply, Matrix
from test_gpu_scaled import _bits

pytestmark = pytest.mark.gpu

OMEGA = 1.5
IDS = ["float64", "float32"]


def _values(a):
    return _t(np.concatenate([a, [0.0]]), np.float64)


def _same_ints(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    off = np.flatnonzero(got != want)
    assert off.size == 0, "%s: %d of %d differ, the first at %d: %d against %d" % (what, off.size, got.size, off[0], got[off[0]], want[off[0]])


# ---- 1: the colouring and the colour-major permutation ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _coloured(name, seed=gs.SEED):
    """The matrix over distinct_values(name) coloured under `seed` and permuted, once per process."""
    rows, p, c, _ = gs.matrix(name)
    m = Matrix(rows, p, c, gs.distinct_values(name), seed)
    m.permute()
    return m


def _plan_is(m, pl, status, what):
    """The device arrays of a test_gpu_mcgs.Matrix against an mc.Plan."""
    plan, rows, nnz = m.plan, m.rows, m.nnz
    assert (plan.rows, plan.colours, plan.conflicts, plan.group) == (rows, status[0], status[2], pl.group), what
    assert list(plan.colour_ptr) == pl.colour_ptr.tolist(), what + ": the 65 colour pointers"
    order = m.order.cpu().numpy()[:rows]
    _same_ints(np.sort(order), np.arange(rows), what + ": d_order is not a permutation of the rows")
    _same_ints(order, pl.order, what + ": d_order")
    _same_ints(m.pp.cpu().numpy()[:rows + 1], pl.p, what + ": d_perm_row_ptr")
    _same_ints(m.pc.cpu().numpy()[:nnz], pl.c, what + ": d_perm_column_index")
    _bits(m.pv.cpu().numpy()[:nnz], pl.v, what + ": d_perm_value")


@pytest.mark.parametrize("name, seed", [(name, seed) for name in gs.MATRICES for seed in (mc.SEEDS if name in gs.BOTH_SEEDS else mc.SEEDS[:1])])
def test_colours_status_and_the_plan_are_the_restatement(name, seed):
    pl, col_of, status = gs.colouring(name, seed)
    m = _coloured(name, seed)
    rows, chunks = m.rows, gs.chunks_of(m.rows)
    print("%s, seed %#x: status %s; %d chunks, %d trips of the chunk scan, the last of %d lanes" % (
        name, seed, m.status_h[:4].tolist(), chunks[0], chunks[2], chunks[1]))
    assert m.status_h[:4].tolist() == status and status[2] == 0 and status[3] == 0
    _same_ints(m.colour_h[:rows], col_of, name + ": the colours")
    _plan_is(m, pl, status, "%s, seed %#x" % (name, seed))
    m.unchanged()


# ---- 2: one symmetric sweep ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", mc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", gs.SWEEPS)
def test_a_symmetric_sweep_is_the_restatement_bit_for_bit_at_the_plans_group_and_at_64(name, dtype):
    pl, _, _ = gs.colouring(name)
    m = _coloured(name)
    rows, (p, c, v) = m.rows, m.host
    rng = np.random.default_rng(rows + 3)
    bh, xh = rng.uniform(-1.0, 1.0, size=rows).astype(dtype), rng.uniform(-1.0, 1.0, size=rows).astype(dtype)
    mh = mc.minv_of(rows, p, c, v, dtype)
    last = pl.colours - 1
    # forwards, then backwards, from a general x: spmv_hip_mcgs_sweep twice
    b, minv, x = Band(bh, dtype), Band(mh, dtype), Band(xh, dtype)
    plan = capi.McgsPlan.from_buffer_copy(m.plan)
    for group in (pl.group, 64):
        tag = "%s, %s, group %d, omega %.1f" % (name, np.dtype(dtype).name, group, OMEGA)
        plan.group = group
        x.set(xh)
        capi.mcgs_sweep(plan, 0, last, OMEGA, b.ptr, minv.ptr, x.ptr, dtype=dtype)
        forward = x.body(tag)
        capi.mcgs_sweep(plan, last, 0, OMEGA, b.ptr, minv.ptr, x.ptr, dtype=dtype)
        both = x.body(tag)
        assert both.dtype == dtype
        want = mc.sweep(pl, 0, last, OMEGA, bh, mh, xh, dtype, group)
        _bits(forward, want, tag + ": x behind the forward sweep")
        _bits(both, mc.sweep(pl, last, 0, OMEGA, bh, mh, want, dtype, group), tag + ": x behind the backward sweep")
    # ... and from zero in one call: spmv_hip_mcgs_apply, at the plan's group
    key = "graph sizes: " + name
    gm._DEVICE[key] = m  # what test_gpu_mcgs.Apply looks its matrix up in
    a = Apply(key, dtype, bh, mh)
    a.run(OMEGA)
    tag = "%s, %s, spmv_hip_mcgs_apply" % (name, np.dtype(dtype).name)
    _bits(a.z.body(tag), mc.apply(pl, OMEGA, bh, mh, dtype), tag + ": z")
    assert np.all(np.isfinite(a.dots.body(tag)))
    a.work.body(tag)
    _bits(b.body(), bh, "b changed")
    _bits(minv.body(), mh, "minv changed")
    _bits(a.r.body(), bh, "r changed")
    m.unchanged()


# ---- 3: the aggregations ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", gs.MATRICES)
def test_aggregates_and_status_are_the_restatement(name):
    rows, p, c, v = gs.matrix(name)
    m = Level2(rows, p, c, v)
    want, status = gs.aggregates(name)
    got, got_status = m.aggregate()
    print("%s: status %s (%d workgroups of rows)" % (name, got_status, -(-rows // 256)))
    assert got_status == status
    _same_ints(got, want, name + ": d_agg")
    if name in gs.DISTANCE_2:
        want, status = gs.aggregates(name, 2)
        got, got_status = m.aggregate_mis2()
        print("%s, distance 2: status %s" % (name, got_status))
        assert got_status == status
        _same_ints(got, want, name + ": d_agg of the distance-2 aggregation")
    m.unchanged()
    if name == "grid_300x300":
        g = gs.general_values(name)
        m.v = _values(g)
        want, status = gs.aggregates(name, 1, 0.25)
        got, got_status = m.aggregate(theta=0.25)
        print("%s, general values, theta 0.25: status %s" % (name, got_status))
        assert got_status == status and status != gs.aggregates(name)[1]
        _same_ints(got, want, name + ": d_agg at theta 0.25")


# ---- 4: the plan --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _level(name, distance=1):
    """The matrix aggregated on the device -- a blocks_* case: under its hand-made plan's d_agg and d_status, uploaded -- with its
    plan and, at distance 1, its coarse pattern, once per process."""
    m = Level2(*gs.matrix(name))
    if name in gs.BLOCKS:
        pl = gs.plan(name)
        sizes = np.bincount(pl.agg)
        m.status_h = [pl.aggregates, 0, pl.largest, int(np.sum(sizes == 1))]
        m.agg, m.status = _ints(m.rows), _ints(4)
        m.agg[:m.rows] = _t(pl.agg, np.int32)
        m.status[:4] = _t(m.status_h, np.int32)
    elif distance == 1:
        m.aggregate()
    else:
        m.aggregate_mis2()
    m.plan_()
    if distance == 1:
        m.symbolic()
    return m


PLANS = [(name, 1) for name in gs.MATRICES] + [(name, 2) for name in gs.DISTANCE_2] + [(name, 1) for name in gs.BLOCKS]


@pytest.mark.parametrize("name, distance", PLANS)
def test_the_plan_is_the_restatement(name, distance):
    m = _level(name, distance)
    pl = gs.plan(name, distance)
    print("%s, distance %d: %d aggregates, the plan's sort over %d bits" % (name, distance, pl.aggregates, gs.bits_of(pl.aggregates)))
    assert (m.plan.rows, m.plan.aggregates, m.plan.largest) == (pl.rows, pl.aggregates, pl.largest)
    _same_ints(m.mptr_h, pl.member_ptr, name + ": d_member_ptr")
    _same_ints(m.member_h, pl.member, name + ": d_member")
    assert (m.plan.d_agg, m.plan.d_member_ptr, m.plan.d_member) == (m.agg.data_ptr(), m.mptr.data_ptr(), m.member.data_ptr())
    _same_ints(_body(m.agg, m.rows, "d_agg"), pl.agg, name + ": the plan changed d_agg")


# ---- 5: the Galerkin product ----------------------------------------------------------------------------------------------------------------

PRODUCTS = gs.GALERKIN + tuple(gs.BLOCKS)


def _pattern_is(m, co, what):
    """The device arrays of a test_gpu_agg.Level behind symbolic() against an ac.Coarse."""
    aggregates = m.plan.aggregates
    assert m.nnz_c == co.nnz_c, what + ": d_status[0]"
    row_ptr, column = _body(m.cp, aggregates + 1, "d_coarse_row_ptr"), _body(m.cc, m.nnz, "d_coarse_column_index")[:co.nnz_c]
    _same_ints(row_ptr, co.row_ptr, what + ": d_coarse_row_ptr")
    _same_ints(column, co.column, what + ": d_coarse_column_index")
    _same_ints(_body(m.order, m.nnz, "d_entry_order"), co.order, what + ": d_entry_order")
    _same_ints(_body(m.eptr, m.nnz + 1, "d_entry_ptr")[:co.nnz_c + 1], co.entry_ptr, what + ": d_entry_ptr")
    row = np.repeat(np.arange(aggregates), np.diff(row_ptr))
    assert np.all((np.diff(column) > 0) | (np.diff(row) > 0)), what + ": the columns of a coarse row are not distinct and ascending"
    assert np.all((column >= 0) & (column < aggregates)), what


@pytest.mark.parametrize("name", PRODUCTS)
def test_the_symbolic_product_is_the_restatement(name):
    m, co = _level(name), gs.coarse(name)
    print("%s: %d rows, %d entries -> %d aggregates (a key of %d bits), %d coarse entries, the longest run %d" % (
        name, m.rows, m.nnz, m.plan.aggregates, gs.bits_of(m.plan.aggregates ** 2), m.nnz_c, int(np.diff(co.entry_ptr).max())))
    assert gs.bits_of(m.plan.aggregates ** 2) == gs.FIGURES[name][1]
    _pattern_is(m, co, name)
    m.unchanged()


@pytest.mark.parametrize("name", PRODUCTS)
def test_the_numeric_product_is_the_restatement_also_behind_a_change_of_the_values(name):
    m, co = _level(name), gs.coarse(name)
    g = gs.general_values(name)
    values = _values(g)
    _bits(m.numeric(values), gs.coarse_values(name), name + ": the coarse values of general fine values")
    other = gs.distinct_values(name)
    values[:m.nnz] = _t(other, np.float64)
    _bits(m.numeric(values), co.values(other), name + ": the coarse values behind a change of the fine values, numeric alone")
    m.unchanged()


# ---- 6: restriction and prolongation ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ac.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["grid_512x512", "blocks_65537"])
def test_restrict_restrict_group_and_prolong_add_are_the_restatement_and_a_nan_stays_in_its_aggregate(name, dtype):
    pl = gs.plan(name)
    hp = HostPlan(pl)
    assert pl.aggregates > 65536
    rng = np.random.default_rng(pl.rows + 3)
    rh, xh = rng.uniform(-1.0, 1.0, size=pl.rows).astype(dtype), rng.uniform(-1.0, 1.0, size=pl.rows).astype(dtype)
    eh = rng.uniform(-1.0, 1.0, size=pl.aggregates).astype(dtype)
    r, rc, e, x = Band(rh, dtype), Band(np.full(pl.aggregates, np.nan), dtype), Band(eh, dtype), Band(xh, dtype)
    tag = "%s, %s" % (name, np.dtype(dtype).name)
    capi.agg_restrict(hp.plan, r.ptr, rc.ptr, dtype=dtype)
    plain = rc.body(tag)
    assert plain.dtype == dtype
    _bits(plain, ac.restrict(pl, rh, dtype), tag + ": r_c of spmv_hip_agg_restrict")
    G = capi.agg_group(hp.plan)
    assert G == a2.group_of(pl.rows, pl.aggregates) and 1 < G < 64
    grouped = {}
    for group in (G, 64):
        rc.fill()
        capi.agg_restrict_group(hp.plan, group, r.ptr, rc.ptr, dtype=dtype)
        grouped[group] = rc.body(tag)
        _bits(grouped[group], a2.restrict_group(pl, group, rh, dtype), tag + ": r_c of spmv_hip_agg_restrict_group at group %d" % group)
    capi.agg_prolong_add(hp.plan, OMEGA, e.ptr, x.ptr, dtype=dtype)
    _bits(x.body(tag), ac.prolong_add(pl, OMEGA, eh, xh, dtype), tag + ": x at omega %.1f" % OMEGA)
    # a NaN at a member of aggregate 65 536 (the first whose number takes 17 bits) and of the last one reaches that r_c alone;
    # every other element keeps the bits of the clean run, which are the restatement's (above)
    for I in sorted({65536, pl.aggregates - 1}):
        members = pl.member[pl.member_ptr[I]:pl.member_ptr[I + 1]]
        bad = rh.copy()
        bad[int(members[-1])] = np.nan
        r.set(bad)
        for group, clean in [(1, plain)] + sorted(grouped.items()):
            rc.fill()
            if group == 1:
                capi.agg_restrict(hp.plan, r.ptr, rc.ptr, dtype=dtype)
            else:
                capi.agg_restrict_group(hp.plan, group, r.ptr, rc.ptr, dtype=dtype)
            got = rc.body(tag)
            assert np.flatnonzero(~np.isfinite(got)).tolist() == [I], (tag, group, I)
            keep = np.arange(pl.aggregates) != I
            _bits(got[keep], clean[keep], "%s, group %d: the other aggregates beside a NaN in aggregate %d" % (tag, group, I))
    _bits(e.body(tag), eh, tag + ": e_c changed")
    for t, a in ((hp.agg, pl.agg), (hp.mptr, pl.member_ptr), (hp.member, pl.member)):
        assert np.array_equal(t.cpu().numpy()[:len(a)], a), tag + ": the plan's arrays changed"


# ---- 7: the hierarchy on its own output ---------------------------------------------------------------------------------------------------------

class OnDevice(Level):
    """test_gpu_agg.Level over arrays that are on the device already: the coarse arrays of the level before, as its calls left them
    (the tensors keep their guards behind the elements; `nnz` says how many of the columns and values count)."""

    def __init__(self, rows, nnz, p, c, v):
        import torch
        self.rows, self.nnz, self.host = rows, nnz, None
        self.p, self.c, self.v = p, c, v
        self.bytes = capi.agg_workspace_bytes(rows, nnz)
        self.bytes0 = capi.agg_workspace_bytes(rows)
        self.work = torch.full((self.bytes // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _device_hierarchy():
    """The four distance-1 levels of grid_512x512 over general values, run on the device: [(level, its coarse values on the host)].
    Only the finest matrix is uploaded; every further level reads d_coarse_row_ptr, d_coarse_column_index and d_coarse_value of the
    level before."""
    rows, p, c, _ = gs.matrix("grid_512x512")
    m = Level(rows, p, c, gs.general_values("grid_512x512"))
    out = []
    for _ in gs.HIERARCHY:
        m.aggregate()
        m.plan_()
        m.symbolic()
        out.append((m, m.numeric()))
        m = OnDevice(m.plan.aggregates, m.nnz_c, m.cp, m.cc, m.cv)
    return out


def test_four_levels_of_the_512_grid_on_the_arrays_the_device_left_are_the_restatement_level_by_level():
    for k, ((m, cv), L) in enumerate(zip(_device_hierarchy(), gs.hierarchy())):
        tag = "level %d" % k
        print("%s: %d rows, %d entries, status %s, %d coarse entries, a key of %d bits" % (tag, m.rows, m.nnz, m.status_h, m.nnz_c, L.key_bits))
        assert (m.rows, m.nnz) == (L.rows, len(L.c)) and L.status == gs.HIERARCHY[k][1]
        assert m.status_h == L.status, tag
        _same_ints(m.agg_h, L.agg, tag + ": d_agg")
        assert (m.plan.rows, m.plan.aggregates, m.plan.largest) == (L.rows, L.status[0], L.status[2]), tag
        _same_ints(m.mptr_h, L.plan.member_ptr, tag + ": d_member_ptr")
        _same_ints(m.member_h, L.plan.member, tag + ": d_member")
        _pattern_is(m, L.coarse, tag)
        _bits(cv, L.cv, tag + ": the coarse values")
        # the level's own matrix is still what the level before wrote (the finest: what was uploaded)
        _same_ints(m.p.cpu().numpy()[:m.rows + 1], L.p, tag + ": the level's row_ptr changed")
        _same_ints(m.c.cpu().numpy()[:m.nnz], L.c, tag + ": the level's columns changed")
        _bits(m.v.cpu().numpy()[:m.nnz], L.v, tag + ": the level's values changed")


# ---- 8: the coarse matrix as a multiply operand and as a matrix to colour ---------------------------------------------------------------------

class ColouredOnDevice(Matrix):
    """test_gpu_mcgs.Matrix over arrays that are on the device already (its permute() is inherited)."""

    def __init__(self, rows, nnz, p, c, v, seed=mc.SEEDS[0]):
        import torch
        self.rows, self.nnz, self.host = rows, nnz, None
        self.p, self.c, self.v = p, c, v
        self.bytes = capi.mcgs_workspace_bytes(rows)
        self.work = torch.full((self.bytes // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
        self.colour = torch.full((rows + 2,), 77, dtype=torch.int32, device="cuda:0")
        self.status = torch.full((6,), 77, dtype=torch.int32, device="cuda:0")
        capi.mcgs_colour(rows, self.p, self.c, seed, self.colour, self.status, self.work, self.bytes)
        self.colour_h, self.status_h = self.colour.cpu().numpy(), self.status.cpu().numpy()
        assert np.all(self.colour_h[rows:] == 77) and np.all(self.status_h[4:] == 77), "colour wrote behind its arrays"
        assert np.all(np.isnan(self.work[self.bytes // 8:].cpu().numpy())), "colour wrote behind its workspace"


def test_the_first_coarse_matrix_multiplies_through_spmv_hip_plan_csr_from_the_arrays_the_product_left(oracle):
    """The hand-off every level of a V-cycle makes: d_coarse_row_ptr (and its host copy), d_coarse_column_index and d_coarse_value
    of the finest level's product are the operand of spmv_hip_plan_csr, spmv_hip_plan_csr_compress and one y += A_c x."""
    (fine, _), L = _device_hierarchy()[0], gs.hierarchy()[0]
    n, nnz = fine.plan.aggregates, fine.nnz_c
    assert (n, nnz) == (95432, 560366)
    p, c, v = L.coarse.row_ptr, L.coarse.column, L.cv
    host_row_ptr = _body(fine.cp, n + 1, "d_coarse_row_ptr").copy()
    plan = capi.CsrPlan(n, n, host_row_ptr)
    plan.compress(fine.cc.data_ptr())
    rng = np.random.default_rng(n)
    xh, y0 = rng.uniform(-1.0, 1.0, size=n), rng.uniform(-1.0, 1.0, size=n)
    x, y = Band(xh), Band(y0)
    plan.spmv(fine.cp.data_ptr(), fine.cc.data_ptr(), fine.cv.data_ptr(), x.ptr, y.ptr)
    got = y.body("y")
    info = plan.info()
    plan.close()
    assert (info["rows"], info["nnz"]) == (n, nnz)
    want = oracle.csr_spmv(n, p, c, v, xh, y=y0, num_threads=4)
    helpers.assert_close(got, want, scale=helpers.abs_products(n, p, c, v, xh) + np.abs(y0), what="y += A_c x over the device's coarse arrays")
    _bits(x.body("x"), xh, "x changed")
    _same_ints(_body(fine.cc, fine.nnz, "d_coarse_column_index")[:nnz], c, "the multiply changed the coarse columns")
    _bits(fine.cv.cpu().numpy()[:nnz], v, "the multiply changed the coarse values")


def test_the_first_coarse_matrix_is_coloured_and_permuted_from_the_arrays_the_product_left():
    (fine, _), L = _device_hierarchy()[0], gs.hierarchy()[0]
    n, nnz = fine.plan.aggregates, fine.nnz_c
    p, c, v = L.coarse.row_ptr, L.coarse.column, L.cv
    col_of, status = mc.colour(n, p, c, mc.SEEDS[0])
    pl = mc.Plan(n, p, c, v, col_of, status)
    m = ColouredOnDevice(n, nnz, fine.cp, fine.cc, fine.cv)
    m.permute()
    print("the first coarse matrix: %d rows, %d entries, status %s, group %d" % (n, nnz, m.status_h[:4].tolist(), m.plan.group))
    assert m.status_h[:4].tolist() == status and status[2] == 0 and status[3] == 0
    _same_ints(m.colour_h[:n], col_of, "the colours of the first coarse matrix")
    _plan_is(m, pl, status, "the first coarse matrix")
    _same_ints(_body(fine.cp, n + 1, "d_coarse_row_ptr"), p, "the colouring changed the coarse row_ptr")
