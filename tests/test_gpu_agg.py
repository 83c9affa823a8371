"""The aggregation multigrid level (include/spmv_hip_agg.h) on the MI355X: spmv_hip_agg_aggregate, spmv_hip_agg_plan,
spmv_hip_agg_galerkin_{symbolic,numeric}, spmv_hip_agg_restrict_{f64,f32} and spmv_hip_agg_prolong_add_{f64,f32}, through
capi.agg_*.

The aggregates, the status, the member lists, the coarse pattern, the runs, the coarse values and every restricted and prolonged
vector are held bit for bit to the numpy restatement of the header (agg_cases; test_agg_cases.py holds that restatement to the
dense P'AP without a device).  Every device array lies between guards that are checked whenever it is read back."""
import math

import numpy as np
import pytest

import agg_cases as ac
import dots_cases as dc
import mcgs_cases as mc
import stream_helpers as sh
from spmv_amd import capi, synth
from test_gpu_krylov import GUARD, Band
from test_gpu_mcgs import _Host, _pcg
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu

MARK = 77  # what the int arrays hold behind their elements


def _t(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _ints(n, extra=2):
    import torch
    return torch.full((n + extra,), MARK, dtype=torch.int32, device="cuda:0")


def _body(t, n, what):
    h = t.cpu().numpy()
    assert np.all(h[n:] == MARK), what + ": written behind its elements"
    return h[:n]


class Level:
    """A CSR matrix on the device and what the setup calls make of it (the arrays the plan points to are kept here)."""

    def __init__(self, rows, p, c, v):
        import torch
        self.rows, self.nnz, self.host = rows, len(c), (p, c, v)
        self.p, self.c, self.v = _t(p, np.int32), _t(np.concatenate([c, [0]]), np.int32), _t(np.concatenate([v, [0.0]]), np.float64)
        self.bytes = capi.agg_workspace_bytes(rows, self.nnz)
        self.bytes0 = capi.agg_workspace_bytes(rows)
        self.work = torch.full((self.bytes // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda:0")

    def aggregate(self, seed=ac.SEEDS[0], theta=0.0, values=True):
        self.agg, self.status = _ints(self.rows), _ints(4)
        capi.agg_aggregate(self.rows, self.p, self.c, self.v if values else None, theta, seed, self.agg, self.status, self.work, self.bytes0)
        self.agg_h, self.status_h = _body(self.agg, self.rows, "d_agg"), _body(self.status, 4, "d_status").tolist()
        assert np.all(np.isnan(self.work[self.bytes // 8:].cpu().numpy())), "aggregate wrote behind its workspace"
        return self.agg_h, self.status_h

    def plan_(self):
        rows, aggregates = self.rows, self.status_h[0]
        self.mptr, self.member = _ints(aggregates + 1), _ints(rows)
        self.plan = capi.agg_plan(rows, self.agg, self.status, self.mptr, self.member, self.work, self.bytes0)
        self.mptr_h, self.member_h = _body(self.mptr, aggregates + 1, "d_member_ptr"), _body(self.member, rows, "d_member")
        return self.plan

    def symbolic(self):
        nnz, aggregates = self.nnz, self.plan.aggregates
        self.cp, self.cc, self.order, self.eptr, self.cstatus = _ints(aggregates + 1), _ints(nnz), _ints(nnz), _ints(nnz + 1), _ints(1)
        capi.agg_galerkin_symbolic(self.plan, nnz, self.p, self.c, self.cp, self.cc, self.order, self.eptr, self.cstatus, self.work, self.bytes)
        self.nnz_c = int(_body(self.cstatus, 1, "d_status of the product")[0])
        assert np.all(np.isnan(self.work[self.bytes // 8:].cpu().numpy())), "symbolic wrote behind its workspace"
        return self.nnz_c

    def numeric(self, values=None):
        import torch
        v = self.v if values is None else values
        self.cv = torch.full((self.nnz_c + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
        capi.agg_galerkin_numeric(self.nnz, self.nnz_c, self.order, self.eptr, v, self.cv)
        h = self.cv.cpu().numpy()
        assert np.all(np.isnan(h[self.nnz_c:])), "numeric wrote behind its values"
        return h[:self.nnz_c]

    def unchanged(self):
        p, c, v = self.host
        assert np.array_equal(self.p.cpu().numpy(), p) and np.array_equal(self.c.cpu().numpy()[:-1], c)
        assert np.array_equal(self.v.cpu().numpy()[:-1].view(np.uint64), v.view(np.uint64))


_DEVICE = {}


def device(name):
    """The matrix `name` aggregated under the first seed at theta 0, with its plan and its coarse pattern, once per process."""
    if name not in _DEVICE:
        m = Level(*ac.matrix(name))
        m.aggregate()
        m.plan_()
        m.symbolic()
        _DEVICE[name] = m
    return _DEVICE[name]


class HostPlan:
    """A plan uploaded from the restatement's arrays, `shift` ints off 16-byte alignment: what restrict and prolong_add read."""

    def __init__(self, pl, shift=0):
        import torch
        self.pl = pl

        def up(a):
            t = torch.full((len(a) + shift + 4,), MARK, dtype=torch.int32, device="cuda:0")
            t[shift:shift + len(a)] = _t(a, np.int32)
            return t

        self.agg, self.mptr, self.member = up(pl.agg), up(pl.member_ptr), up(pl.member)
        self.plan = capi.AggPlan()
        self.plan.rows, self.plan.aggregates, self.plan.largest = pl.rows, pl.aggregates, pl.largest
        self.plan.d_agg, self.plan.d_member_ptr, self.plan.d_member = (t.data_ptr() + 4 * shift for t in (self.agg, self.mptr, self.member))


# ---- 1: the aggregation, bit for bit the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", ac.SEEDS)
@pytest.mark.parametrize("name", ac.MATRICES)
def test_aggregates_and_status_are_the_restatement(name, seed):
    rows, p, c, v = ac.matrix(name)
    m = Level(rows, p, c, v)
    for theta in ac.THETAS:
        want, status = ac.aggregate(rows, p, c, v, theta, seed)
        got, got_status = m.aggregate(seed, theta)
        print("%s, seed %#x, theta %.2f: status %s" % (name, seed, theta, got_status))
        assert got_status == status
        assert np.array_equal(got, want)
        again, again_status = m.aggregate(seed, theta)
        assert np.array_equal(again, got) and again_status == got_status, "a second run"
    # without values every stored off-diagonal entry counts, whatever theta
    got, got_status = m.aggregate(seed, 0.25, values=False)
    want, status = ac.aggregate(rows, p, c, None, 0.25, seed)
    assert got_status == status and np.array_equal(got, want)
    m.unchanged()


# ---- 2: the plan ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.MATRICES)
def test_the_plan_is_the_restatement(name):
    m = device(name)
    pl, status = ac.plan(name)
    assert (m.plan.rows, m.plan.aggregates, m.plan.largest) == (pl.rows, status[0], status[2])
    assert np.array_equal(m.mptr_h, pl.member_ptr) and np.array_equal(m.member_h, pl.member)
    assert (m.plan.d_agg, m.plan.d_member_ptr, m.plan.d_member) == (m.agg.data_ptr(), m.mptr.data_ptr(), m.member.data_ptr())
    assert np.array_equal(_body(m.agg, m.rows, "d_agg"), pl.agg), "the plan changed d_agg"


def test_an_aggregate_number_outside_the_status_is_a_state_error():
    m = Level(*ac.matrix("grid_37x29"))
    m.aggregate()
    m.agg[17] = m.status_h[0]
    with pytest.raises(capi.SpmvHipError) as e:
        m.plan_()
    assert e.value.code == capi.ERR_STATE


# ---- 3, 4: the Galerkin product ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ac.MATRICES)
def test_the_symbolic_product_is_the_restatement(name):
    m = device(name)
    co = ac.coarse(name)
    print("%s: %d rows, %d entries -> %d aggregates, %d coarse entries, the longest run %d" % (
        name, m.rows, m.nnz, m.plan.aggregates, m.nnz_c, int(np.diff(co.entry_ptr).max()) if co.nnz_c else 0))
    assert m.nnz_c == co.nnz_c
    assert np.array_equal(_body(m.cp, m.plan.aggregates + 1, "d_coarse_row_ptr"), co.row_ptr)
    assert np.array_equal(_body(m.order, m.nnz, "d_entry_order"), co.order)
    assert np.array_equal(_body(m.cc, m.nnz, "d_coarse_column_index")[:co.nnz_c], co.column)
    assert np.array_equal(_body(m.eptr, m.nnz + 1, "d_entry_ptr")[:co.nnz_c + 1], co.entry_ptr)
    m.unchanged()


@pytest.mark.parametrize("name", ac.MATRICES)
def test_the_numeric_product_is_the_restatement_also_behind_a_change_of_the_values(name):
    m = device(name)
    co = ac.coarse(name)
    v = m.host[2]
    _bits(m.numeric(), co.values(v), name + ": the coarse values")
    g = ac.general_values(name)
    _bits(m.numeric(_t(np.concatenate([g, [0.0]]), np.float64)), co.values(g), name + ": the coarse values of other fine values, numeric alone")
    if name in ("star_5000", "long_row", "clique_66"):
        assert int(np.diff(co.entry_ptr).max()) >= {"star_5000": 15001, "long_row": 20, "clique_66": 4356}[name]
    m.unchanged()


# ---- 5: restriction and prolongation -------------------------------------------------------------------------------------------------

def _plans():
    out = [("blocks of %d rows" % n, ac.blocks(n, 7)) for n in ac.SIZES]
    return out + [(name, ac.plan(name)[0]) for name in ("grid_13x13x13", "isolated", "star_5000", "long_row")]


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_restrict_and_prolong_add_are_the_restatement_bit_for_bit(dtype):
    for what, pl in _plans():
        rng = np.random.default_rng(pl.rows + 3)
        rh, xh = rng.uniform(-1.0, 1.0, size=pl.rows).astype(dtype), rng.uniform(-1.0, 1.0, size=pl.rows).astype(dtype)
        eh = rng.uniform(-1.0, 1.0, size=pl.aggregates).astype(dtype)
        for shift in (0, 1):  # the index arrays 16-byte aligned, and 4 bytes off
            hp = HostPlan(pl, shift)
            tag = "%s, %s, index arrays %d bytes off" % (what, np.dtype(dtype).name, 4 * shift)
            r, rc, e, x = Band(rh, dtype), Band(np.full(pl.aggregates, np.nan), dtype), Band(eh, dtype), Band(xh, dtype)
            capi.agg_restrict(hp.plan, r.ptr, rc.ptr, dtype=dtype)
            got = rc.body(tag)
            assert got.dtype == dtype
            _bits(got, ac.restrict(pl, rh, dtype), tag + ": r_c")
            for omega in ac.OMEGAS:
                x.set(xh)
                capi.agg_prolong_add(hp.plan, omega, e.ptr, x.ptr, dtype=dtype)
                _bits(x.body(tag), ac.prolong_add(pl, omega, eh, xh, dtype), tag + ": x at omega %.1f" % omega)
            _bits(r.body(tag), rh, tag + ": r changed")
            _bits(e.body(tag), eh, tag + ": e_c changed")
            for t, a in ((hp.agg, pl.agg), (hp.mptr, pl.member_ptr), (hp.member, pl.member)):
                assert np.array_equal(t.cpu().numpy()[shift:shift + len(a)], a), tag + ": the plan's arrays changed"


def test_the_device_plan_restricts_as_the_uploaded_one():
    m = device("grid_13x13x13")
    pl, _ = ac.plan("grid_13x13x13")
    rh = np.random.default_rng(9).uniform(-1.0, 1.0, size=pl.rows)
    r, rc = Band(rh), Band(np.full(pl.aggregates, np.nan))
    capi.agg_restrict(m.plan, r.ptr, rc.ptr, dtype=np.float64)
    _bits(rc.body(), ac.restrict(pl, rh, np.float64), "r_c through the plan of spmv_hip_agg_plan")


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_a_nan_in_r_stays_in_its_aggregate(dtype):
    for what, pl in (("grid_13x13x13", ac.plan("grid_13x13x13")[0]), ("blocks of 4099 rows", ac.blocks(4099, 7))):
        hp = HostPlan(pl)
        rh = np.random.default_rng(8).uniform(-1.0, 1.0, size=pl.rows).astype(dtype)
        r, rc = Band(rh, dtype), Band(np.full(pl.aggregates, np.nan), dtype)
        for i in (0, 1, pl.rows // 2, pl.rows - 1):
            for bad_value in (np.nan, np.inf):
                bad = rh.copy()
                bad[i] = bad_value
                r.set(bad)
                rc.fill()
                capi.agg_restrict(hp.plan, r.ptr, rc.ptr, dtype=dtype)
                got = rc.body(what)
                assert np.flatnonzero(~np.isfinite(got)).tolist() == [int(pl.agg[i])], (what, i)
                clean = np.isfinite(got)
                _bits(got[clean], ac.restrict(pl, bad, dtype)[clean], "%s: a non-finite r[%d]" % (what, i))


@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_two_runs_a_delayed_stream_two_streams_and_a_replayed_graph_give_identical_bits(side, dtype):
    import torch
    pl = ac.blocks(4099, 7)
    hp = HostPlan(pl)
    rows, aggregates, omega = pl.rows, pl.aggregates, 1.5
    rng = np.random.default_rng(6)
    rh, xh = rng.uniform(-1.0, 1.0, size=rows).astype(dtype), rng.uniform(-1.0, 1.0, size=rows).astype(dtype)
    want_rc = ac.restrict(pl, rh, dtype)
    want_x = ac.prolong_add(pl, omega, want_rc, xh, dtype)
    tag = np.dtype(dtype).name

    def pair(stream, r, rc, x):
        capi.agg_restrict(hp.plan, r, rc, stream, dtype=dtype)
        capi.agg_prolong_add(hp.plan, omega, rc, x, stream, dtype=dtype)

    r, rc, x = Band(rh, dtype), Band(np.full(aggregates, np.nan), dtype), Band(xh, dtype)
    for run in range(2):
        rc.fill()
        x.set(xh)
        pair(0, r.ptr, rc.ptr, x.ptr)
        _bits(rc.body(tag), want_rc, tag + ": r_c, run %d" % run)
        _bits(x.body(tag), want_x, tag + ": x, run %d" % run)
    # behind the delay on a non-blocking stream: the vectors arrive behind the delay
    ra, rca, xa = sh.operand(rh), sh.result(np.zeros(aggregates, dtype=dtype)), sh.result(xh)
    (brc, bx), _ = sh.delayed(side, [ra, rca, xa], lambda s: pair(s, ra.ptr, rca.ptr, xa.ptr), [rca, xa], "restrict and prolong_add behind the delay (%s)" % tag)
    _bits(brc, want_rc, tag + ": r_c behind the delay")
    _bits(bx, want_x, tag + ": x behind the delay")
    # two streams at once: r_c and x each
    own = [(Band(np.full(aggregates, np.nan), dtype), Band(xh, dtype)) for _ in side.streams]
    torch.cuda.synchronize()
    for s, (c2, x2) in zip(side.streams, own):
        pair(s.cuda_stream, r.ptr, c2.ptr, x2.ptr)
    for s in side.streams:
        s.synchronize()
    for c2, x2 in own:
        _bits(c2.body(tag), want_rc, tag + ": r_c of two streams at once")
        _bits(x2.body(tag), want_x, tag + ": x of two streams at once")
    # a captured graph of the pair, replayed twice: x takes the correction twice
    cap = torch.cuda.Stream()
    rc.fill()
    x.set(xh)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        pair(torch.cuda.current_stream().cuda_stream, r.ptr, rc.ptr, x.ptr)
    _bits(x.body(tag), xh, tag + ": the capture ran the calls")
    for replay in range(2):
        g.replay()
    torch.cuda.synchronize()
    _bits(rc.body(tag), want_rc, tag + ": r_c of the replayed graph")
    _bits(x.body(tag), ac.prolong_add(pl, omega, want_rc, want_x, dtype), tag + ": x of the graph replayed twice")
    del g


def test_numeric_is_captured_and_replayed():
    import torch
    m = device("long_row")
    co = ac.coarse("long_row")
    g_values = ac.general_values("long_row")
    values = _t(np.concatenate([m.host[2], [0.0]]), np.float64)
    cv = torch.full((m.nnz_c + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        capi.agg_galerkin_numeric(m.nnz, m.nnz_c, m.order, m.eptr, values, cv, torch.cuda.current_stream().cuda_stream)
    g.replay()
    torch.cuda.synchronize()
    _bits(cv.cpu().numpy()[:m.nnz_c], co.values(m.host[2]), "the replayed numeric product")
    values[:m.nnz] = _t(g_values, np.float64)
    g.replay()
    torch.cuda.synchronize()
    _bits(cv.cpu().numpy()[:m.nnz_c], co.values(g_values), "the replayed numeric product behind a change of the values")
    del g


# ---- 6: eight PCG iterations on poisson2D.mtx -------------------------------------------------------------------------------------------

def test_eight_pcg_iterations_on_poisson2d_with_the_two_level_cycle_verify_call_by_call_and_beat_the_diagonal():
    """The cycle of agg_cases.two_level_cycle composed from existing calls: spmv_hip_bjacobi_apply_f64 (damped Jacobi from zero), the
    scaled multiply for r - A z, spmv_hip_agg_restrict_f64, a dense coarse solve in torch (the inverse of the coarse matrix the
    numeric product gave, applied by a matrix-vector product), spmv_hip_agg_prolong_add_f64, the scaled multiply again and
    spmv_hip_bjacobi_apply_add_f64; r'z by torch.dot into the scalar the CG updates read.  Every call is held to ITS OWN inputs as
    the device stored them: the restriction, the prolongation and the two smoothing steps bit for bit, the multiplies to two
    summation orders, the solve to 1e-10 of the coarse residual."""
    import torch
    dtype, omega = np.float64, 1.0
    h = _Host()
    mdev = Dev(h, "c16_f64")
    m = device("poisson2D")
    pl, _ = ac.plan("poisson2D")
    co = ac.coarse("poisson2D")
    n, na = h.rows, pl.aggregates
    cv = m.numeric()
    _bits(cv, co.values(h.v), "the coarse values")
    Ac = co.dense(cv)
    inverse = torch.linalg.inv(_t(Ac, np.float64))
    smooth_h = ac.smoother_of(n, h.p, h.c, h.v, dtype)
    minv_h = mc.minv_of(n, h.p, h.c, h.v, dtype)
    smooth, minv = Band(smooth_h), Band(minv_h)
    t, rc, ec = Band(np.full(n, np.nan)), Band(np.full(na, np.nan)), Band(np.full(na, np.nan))
    multiply = mdev.plan.spmv_f64_scaled
    taken = []

    def view(band):
        return band.t[GUARD:GUARD + band.n]

    def cycle(r, z, dots, work, nbytes, s):
        shots = []
        capi.bjacobi_apply(n, 1, smooth.ptr, r.ptr, z.ptr, None, None, 0, s, dtype=dtype)
        shots.append(z.snap())
        multiply(mdev.tp.data_ptr(), mdev.ac, mdev.av, z.ptr, -1.0, 1.0, r.ptr, t.ptr, s)
        shots.append(t.snap())
        capi.agg_restrict(m.plan, t.ptr, rc.ptr, s, dtype=dtype)
        shots.append(rc.snap())
        torch.matmul(inverse, view(rc), out=view(ec))
        shots.append(ec.snap())
        capi.agg_prolong_add(m.plan, omega, ec.ptr, z.ptr, s, dtype=dtype)
        shots.append(z.snap())
        multiply(mdev.tp.data_ptr(), mdev.ac, mdev.av, z.ptr, -1.0, 1.0, r.ptr, t.ptr, s)
        shots.append(t.snap())
        capi.bjacobi_apply_add(n, 1, smooth.ptr, t.ptr, z.ptr, s, dtype=dtype)
        view(dots)[0] = torch.dot(view(r), view(z))
        view(dots)[1] = 0.0
        taken.append(shots)

    values = h.v.astype(np.float64)
    longest = int(np.diff(h.p).max())
    starts = h.p[:-1].astype(np.int64)

    def residual_ok(got, r, z, what):
        prod = values * z[h.c]
        ref, scale = r - np.add.reduceat(prod, starts), np.abs(r) + np.add.reduceat(np.abs(prod), starts)
        assert np.all(np.abs(got - ref) <= 2 * (longest + 2) * 2.0 ** -53 * scale), what + ": not r - A z"

    def cycle_verify(r, z, dots, what):
        shots = taken.pop(0)
        z1, z2 = _of(shots[0], n), _of(shots[4], n)
        t1, rc1, ec1, t2 = t.body(what, shots[1]), rc.body(what, shots[2]), ec.body(what, shots[3]), t.body(what, shots[5])
        _bits(z1, smooth_h * r, what + ": z = minv r")
        residual_ok(t1, r, z1, what + ", the first residual")
        _bits(rc1, ac.restrict(pl, t1, dtype), what + ": r_c against the restatement")
        assert np.linalg.norm(Ac @ ec1 - rc1) <= 1e-10 * np.linalg.norm(rc1), what + ": the coarse solve"
        _bits(z2, ac.prolong_add(pl, omega, ec1, z1, dtype), what + ": z += omega P e_c against the restatement")
        residual_ok(t2, r, z2, what + ", the second residual")
        _bits(z, z2 + smooth_h * t2, what + ": z += minv t")
        prod = r * z
        assert abs(dots[0] - math.fsum(prod)) <= dc.bound(prod), what + ": r'z"

    def _of(snap, count):
        a = snap.cpu().numpy()
        assert np.all(np.isnan(np.concatenate([a[:GUARD], a[GUARD + count:]])))
        return a[GUARD:GUARD + count].copy()

    def diagonal(r, z, dots, work, nbytes, s):
        capi.bjacobi_apply(n, 1, minv.ptr, r.ptr, z.ptr, dots.ptr, work.ptr, nbytes, s, dtype=dtype)

    def diagonal_verify(r, z, dots, what):
        _bits(z, minv_h * r, what + ": z = minv r")

    first, last = _pcg(h, mdev, dtype, cycle, cycle_verify)
    assert not taken
    first_d, last_d = _pcg(h, mdev, dtype, diagonal, diagonal_verify)
    print("r'r of r0 %.6e; after %d iterations with the two-level cycle over %d aggregates at omega %.1f %.6e, with the diagonal %.6e" % (
        first, ac.ITERATIONS, na, omega, last, last_d))
    assert first == first_d == 367.0
    assert np.isfinite(last) and last < ac.PCG_FACTOR * last_d
    mdev.close()


# ---- 7: the one timing assertion ---------------------------------------------------------------------------------------------------------

def test_prolong_add_on_the_4096_grid_takes_no_longer_than_the_torch_form():
    """Poisson 4096^2, doubles, the aggregates of spmv_hip_agg_aggregate, one process, torch events on one stream; three warm-up
    rounds, 25 rounds alternating the two ways, medians.  Asserted: median(spmv_hip_agg_prolong_add_f64) <= median(x.add_(e[agg],
    alpha=w)).  A condition derived from the bytes, not a measured margin: the torch form writes a temporary of x's size and reads it
    again, 32 bytes a row beside the index against 16.
    Measured: 83.8 against 197.1 us with 32-bit indices, ratio 0.425 (tools/agg_ab.py in another process: 76.7 against 197.6 us)."""
    import torch
    rows, cols, p, c, v = synth.poisson2d(4096)[:5]
    p, c, v = np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)
    m = Level(rows, p, c, v)
    _, status = m.aggregate()
    plan = m.plan_()
    assert status[0] == plan.aggregates and rows // 6 < plan.aggregates < rows // 2 and status[2] <= 5, status
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    e = torch.rand(plan.aggregates, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1
    x = torch.zeros(rows, dtype=torch.float64, device="cuda:0")
    index = m.agg[:rows]
    try:
        x.add_(e[index], alpha=0.5)
    except (IndexError, TypeError, RuntimeError):
        index = index.long()
    x.zero_()
    capi.agg_prolong_add(plan, 0.5, e, x, stream)
    want = torch.zeros_like(x).add_(e[index], alpha=0.5)
    assert bool(torch.equal(x, want))

    def ours():
        capi.agg_prolong_add(plan, 1e-3, e, x, stream)

    def theirs():
        x.add_(e[index], alpha=1e-3)

    med = _alternate({"prolong_add": ours, "torch": theirs})
    assert bool(torch.all(torch.isfinite(x)))
    print("Poisson 4096^2: %d aggregates in %d rounds, the largest of %d rows, %d singletons; prolong_add median %.1f us, x.add_(e[agg], alpha=w) "
          "with %s indices median %.1f us, ratio %.3f" % (status[0], status[1], status[2], status[3], med["prolong_add"], str(index.dtype),
                                                          med["torch"], med["prolong_add"] / med["torch"]))
    assert med["prolong_add"] <= med["torch"], med
