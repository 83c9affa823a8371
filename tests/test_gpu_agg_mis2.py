"""include/spmv_hip_agg_mis2.h on the MI355X: spmv_hip_agg_aggregate_mis2 and spmv_hip_agg_restrict_group_{f64,f32}, through
capi.agg_aggregate_mis2 and capi.agg_restrict_group, and the existing plan, Galerkin product, restriction and prolongation on the
new aggregates.

The aggregates, the status and every restricted vector are held bit for bit to the numpy restatement of the header
(agg_mis2_cases; test_agg_mis2_cases.py holds that restatement to its properties without a device).  Every device array lies
between guards that are checked whenever it is read back."""
import math

import numpy as np
import pytest

import agg_cases as ac
import agg_mis2_cases as a2
import dots_cases as dc
import mcgs_cases as mc
import stream_helpers as sh
from spmv_amd import capi, synth
from test_gpu_agg import HostPlan, Level, _body, _ints, _t
from test_gpu_krylov import GUARD, Band
from test_gpu_mcgs import _Host, _pcg
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu


class Level2(Level):
    """test_gpu_agg.Level with the aggregates of spmv_hip_agg_aggregate_mis2, in a workspace of its own rule."""

    def aggregate_mis2(self, seed=ac.SEEDS[0], theta=0.0, values=True):
        import torch
        need = capi.agg_mis2_workspace_bytes(self.rows)
        work = torch.full((need // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
        self.agg, self.status = _ints(self.rows), _ints(4)
        capi.agg_aggregate_mis2(self.rows, self.p, self.c, self.v if values else None, theta, seed, self.agg, self.status, work, need)
        self.agg_h, self.status_h = _body(self.agg, self.rows, "d_agg"), _body(self.status, 4, "d_status").tolist()
        assert np.all(np.isnan(work[need // 8:].cpu().numpy())), "aggregate_mis2 wrote behind its workspace"
        return self.agg_h, self.status_h


# ---- 1: the aggregation, bit for bit the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", ac.SEEDS)
@pytest.mark.parametrize("name", ac.MATRICES)
def test_aggregates_and_status_are_the_restatement(name, seed):
    rows, p, c, v = ac.matrix(name)
    m = Level2(rows, p, c, v)
    for values, label in ((v, "the matrix's values"), (ac.general_values(name), "general values")):
        m.v = _t(np.concatenate([values, [0.0]]), np.float64)
        for theta in ac.THETAS:
            want, status = a2.aggregate(rows, p, c, values, theta, seed)
            got, got_status = m.aggregate_mis2(seed, theta)
            print("%s, %s, seed %#x, theta %.2f: status %s" % (name, label, seed, theta, got_status))
            assert got_status == status
            assert np.array_equal(got, want)
    again, again_status = m.aggregate_mis2(seed, ac.THETAS[-1])
    assert np.array_equal(again, got) and again_status == got_status, "a second run"
    # without values every stored off-diagonal entry counts, whatever theta
    got, got_status = m.aggregate_mis2(seed, 0.25, values=False)
    want, status = a2.aggregate(rows, p, c, None, 0.25, seed)
    assert got_status == status and np.array_equal(got, want)
    m.v = _t(np.concatenate([v, [0.0]]), np.float64)
    m.unchanged()


# ---- 2: the existing plan and Galerkin product on the new aggregates ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid_13x13x13", "long_row", "isolated"])
def test_the_plan_and_the_galerkin_product_on_the_new_aggregates_are_the_restatement(name):
    rows, p, c, v = ac.matrix(name)
    m = Level2(rows, p, c, v)
    m.aggregate_mis2()
    m.plan_()
    pl, status = a2.plan(name)
    co = a2.coarse(name)
    assert (m.plan.rows, m.plan.aggregates, m.plan.largest) == (pl.rows, status[0], status[2])
    assert np.array_equal(m.mptr_h, pl.member_ptr) and np.array_equal(m.member_h, pl.member)
    assert m.symbolic() == co.nnz_c
    assert np.array_equal(_body(m.cp, m.plan.aggregates + 1, "d_coarse_row_ptr"), co.row_ptr)
    assert np.array_equal(_body(m.order, m.nnz, "d_entry_order"), co.order)
    assert np.array_equal(_body(m.cc, m.nnz, "d_coarse_column_index")[:co.nnz_c], co.column)
    assert np.array_equal(_body(m.eptr, m.nnz + 1, "d_entry_ptr")[:co.nnz_c + 1], co.entry_ptr)
    _bits(m.numeric(), co.values(v), name + ": the coarse values")
    g = ac.general_values(name)
    _bits(m.numeric(_t(np.concatenate([g, [0.0]]), np.float64)), co.values(g), name + ": the coarse values of other fine values")
    # the grouped restriction through the plan that spmv_hip_agg_plan filled, at the recommended group
    G = capi.agg_group(m.plan)
    assert G == a2.group_of(pl.rows, pl.aggregates)
    rh = np.random.default_rng(9).uniform(-1.0, 1.0, size=rows)
    r, rc = Band(rh), Band(np.full(pl.aggregates, np.nan))
    capi.agg_restrict_group(m.plan, G, r.ptr, rc.ptr, dtype=np.float64)
    _bits(rc.body(), a2.restrict_group(pl, G, rh, np.float64), "r_c through the plan of spmv_hip_agg_plan at group %d" % G)
    m.unchanged()


# ---- 3: the grouped restriction ---------------------------------------------------------------------------------------------------------

def _plans():
    out = [("blocks of %d rows" % n, ac.blocks(n, 7)) for n in ac.SIZES]
    return out + [(name, a2.plan(name)[0]) for name in ("grid_13x13x13", "long_row", "star_5000")]


def test_the_plans_are_what_they_are_for():
    assert a2.plan("star_5000")[1] == [1, 1, 5001, 0] and -(-5001 // 64) == 79
    assert 81 <= a2.plan("long_row")[1][2] <= 90


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_restrict_group_is_the_restatement_bit_for_bit(dtype):
    for what, pl in _plans():
        rh = np.random.default_rng(pl.rows + 3).uniform(-1.0, 1.0, size=pl.rows).astype(dtype)
        plain = ac.restrict(pl, rh, dtype)
        for shift in (0, 1):  # the index arrays 16-byte aligned, and 4 bytes off
            hp = HostPlan(pl, shift)
            r, rc = Band(rh, dtype), Band(np.full(pl.aggregates, np.nan), dtype)
            for group in a2.GROUPS:
                tag = "%s, %s, group %d, index arrays %d bytes off" % (what, np.dtype(dtype).name, group, 4 * shift)
                rc.fill()
                capi.agg_restrict_group(hp.plan, group, r.ptr, rc.ptr, dtype=dtype)
                got = rc.body(tag)
                assert got.dtype == dtype
                _bits(got, a2.restrict_group(pl, group, rh, dtype), tag + ": r_c")
                if group == 1:
                    _bits(got, plain, tag + ": the restatement of spmv_hip_agg_restrict")
                    rc.fill()
                    capi.agg_restrict(hp.plan, r.ptr, rc.ptr, dtype=dtype)
                    _bits(rc.body(tag), got, tag + ": spmv_hip_agg_restrict")
            _bits(r.body(what), rh, what + ": r changed")
            for t, a in ((hp.agg, pl.agg), (hp.mptr, pl.member_ptr), (hp.member, pl.member)):
                assert np.array_equal(t.cpu().numpy()[shift:shift + len(a)], a), what + ": the plan's arrays changed"


@pytest.mark.parametrize("group", [8, 64])
@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_a_nan_in_r_stays_in_its_aggregate(dtype, group):
    for what, pl in (("grid_13x13x13", a2.plan("grid_13x13x13")[0]), ("blocks of 4099 rows", ac.blocks(4099, 7))):
        hp = HostPlan(pl)
        rh = np.random.default_rng(8).uniform(-1.0, 1.0, size=pl.rows).astype(dtype)
        r, rc = Band(rh, dtype), Band(np.full(pl.aggregates, np.nan), dtype)
        for i in (0, 1, pl.rows // 2, pl.rows - 1):
            for bad_value in (np.nan, np.inf):
                bad = rh.copy()
                bad[i] = bad_value
                r.set(bad)
                rc.fill()
                capi.agg_restrict_group(hp.plan, group, r.ptr, rc.ptr, dtype=dtype)
                got = rc.body(what)
                assert np.flatnonzero(~np.isfinite(got)).tolist() == [int(pl.agg[i])], (what, i)
                clean = np.isfinite(got)
                _bits(got[clean], a2.restrict_group(pl, group, bad, dtype)[clean], "%s: a non-finite r[%d]" % (what, i))


@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


@pytest.mark.parametrize("dtype", ac.DTYPES, ids=["float64", "float32"])
def test_two_runs_a_delayed_stream_two_streams_and_a_replayed_graph_give_identical_bits(side, dtype):
    import torch
    pl, group = a2.plan("grid_13x13x13")[0], 16
    hp = HostPlan(pl)
    rows, aggregates = pl.rows, pl.aggregates
    rh = np.random.default_rng(6).uniform(-1.0, 1.0, size=rows).astype(dtype)
    want = a2.restrict_group(pl, group, rh, dtype)
    tag = np.dtype(dtype).name

    def call(stream, r, rc):
        capi.agg_restrict_group(hp.plan, group, r, rc, stream, dtype=dtype)

    r, rc = Band(rh, dtype), Band(np.full(aggregates, np.nan), dtype)
    for run in range(2):
        rc.fill()
        call(0, r.ptr, rc.ptr)
        _bits(rc.body(tag), want, tag + ": r_c, run %d" % run)
    # behind the delay on a non-blocking stream: the vectors arrive behind the delay
    ra, rca = sh.operand(rh), sh.result(np.zeros(aggregates, dtype=dtype))
    (brc,), _ = sh.delayed(side, [ra, rca], lambda s: call(s, ra.ptr, rca.ptr), [rca], "restrict_group behind the delay (%s)" % tag)
    _bits(brc, want, tag + ": r_c behind the delay")
    # two streams at once: r_c each
    own = [Band(np.full(aggregates, np.nan), dtype) for _ in side.streams]
    torch.cuda.synchronize()
    for s, c2 in zip(side.streams, own):
        call(s.cuda_stream, r.ptr, c2.ptr)
    for s in side.streams:
        s.synchronize()
    for c2 in own:
        _bits(c2.body(tag), want, tag + ": r_c of two streams at once")
    # a captured graph, replayed twice, the second time behind a change of r
    cap = torch.cuda.Stream()
    rc.fill()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        call(torch.cuda.current_stream().cuda_stream, r.ptr, rc.ptr)
    assert np.all(np.isnan(rc.body(tag))), tag + ": the capture ran the call"
    g.replay()
    torch.cuda.synchronize()
    _bits(rc.body(tag), want, tag + ": r_c of the replayed graph")
    r.set(-rh)
    g.replay()
    torch.cuda.synchronize()
    _bits(rc.body(tag), a2.restrict_group(pl, group, -rh, dtype), tag + ": r_c of the graph replayed behind a change of r")
    del g


# ---- 4: the hierarchy on the device ---------------------------------------------------------------------------------------------------

def test_the_512_grid_reaches_a_thousand_rows_in_three_coarsenings_as_the_restatement_does():
    want = a2.grid_512_hierarchy()
    rows, p, c, v = mc.grid(512, 512)
    sizes, statuses = [rows], []
    for _ in range(3):
        m = Level2(rows, p, c, v)
        _, status = m.aggregate_mis2()
        m.plan_()
        nnz_c = m.symbolic()
        v = m.numeric()
        rows, p, c = m.plan.aggregates, _body(m.cp, m.plan.aggregates + 1, "d_coarse_row_ptr").copy(), _body(m.cc, m.nnz, "d_coarse_column_index")[:nnz_c].copy()
        sizes.append(rows)
        statuses.append(status)
    print("grid 512 x 512 on the device: rows per level %s, statuses %s" % (sizes, statuses))
    assert sizes == [n for n, _, _ in want] and statuses == [s for _, _, s in want[:-1]]
    assert sizes[-1] <= 1000 and all(s[3] == 0 for s in statuses)


# ---- 5: eight PCG iterations on poisson2D.mtx -------------------------------------------------------------------------------------------

def test_eight_pcg_iterations_on_poisson2d_with_the_two_level_cycle_verify_call_by_call_and_beat_the_diagonal():
    """The cycle of agg_cases.two_level_cycle over the distance-2 aggregates, composed as in test_gpu_agg.py with
    spmv_hip_agg_restrict_group_f64 at spmv_hip_agg_group(plan) for the restriction.  Every call is held to ITS OWN inputs as the
    device stored them: the restriction, the prolongation and the two smoothing steps bit for bit, the multiplies to two summation
    orders, the solve to 1e-10 of the coarse residual."""
    import torch
    dtype, omega = np.float64, 1.0
    h = _Host()
    mdev = Dev(h, "c16_f64")
    m = Level2(*ac.matrix("poisson2D"))
    m.aggregate_mis2()
    m.plan_()
    m.symbolic()
    pl, _ = a2.plan("poisson2D")
    co = a2.coarse("poisson2D")
    G = capi.agg_group(m.plan)
    assert G == a2.group_of(pl.rows, pl.aggregates) == 16
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
        capi.agg_restrict_group(m.plan, G, t.ptr, rc.ptr, s, dtype=dtype)
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

    def _of(snap, count):
        a = snap.cpu().numpy()
        assert np.all(np.isnan(np.concatenate([a[:GUARD], a[GUARD + count:]])))
        return a[GUARD:GUARD + count].copy()

    def cycle_verify(r, z, dots, what):
        shots = taken.pop(0)
        z1, z2 = _of(shots[0], n), _of(shots[4], n)
        t1, rc1, ec1, t2 = t.body(what, shots[1]), rc.body(what, shots[2]), ec.body(what, shots[3]), t.body(what, shots[5])
        _bits(z1, smooth_h * r, what + ": z = minv r")
        residual_ok(t1, r, z1, what + ", the first residual")
        _bits(rc1, a2.restrict_group(pl, G, t1, dtype), what + ": r_c against the restatement")
        assert np.linalg.norm(Ac @ ec1 - rc1) <= 1e-10 * np.linalg.norm(rc1), what + ": the coarse solve"
        _bits(z2, ac.prolong_add(pl, omega, ec1, z1, dtype), what + ": z += omega P e_c against the restatement")
        residual_ok(t2, r, z2, what + ", the second residual")
        _bits(z, z2 + smooth_h * t2, what + ": z += minv t")
        prod = r * z
        assert abs(dots[0] - math.fsum(prod)) <= dc.bound(prod), what + ": r'z"

    def diagonal(r, z, dots, work, nbytes, s):
        capi.bjacobi_apply(n, 1, minv.ptr, r.ptr, z.ptr, dots.ptr, work.ptr, nbytes, s, dtype=dtype)

    def diagonal_verify(r, z, dots, what):
        _bits(z, minv_h * r, what + ": z = minv r")

    first, last = _pcg(h, mdev, dtype, cycle, cycle_verify)
    assert not taken
    first_d, last_d = _pcg(h, mdev, dtype, diagonal, diagonal_verify)
    print("r'r of r0 %.6e; after %d iterations with the two-level cycle over %d distance-2 aggregates at omega %.1f and group %d %.6e, with the "
          "diagonal %.6e: ratio %.3e" % (first, ac.ITERATIONS, na, omega, G, last, last_d, last / last_d))
    assert first == first_d == 367.0
    assert np.isfinite(last) and last < a2.PCG_FACTOR * last_d
    mdev.close()


# ---- 6: the one timing assertion ---------------------------------------------------------------------------------------------------------

def test_restrict_group_on_the_4096_grid_takes_no_longer_than_the_restriction_by_one_lane():
    """Poisson 4096^2, doubles, the plan of spmv_hip_agg_aggregate_mis2, one process, torch events on one stream; three warm-up
    rounds, 25 rounds alternating the two calls, medians.  Asserted: median(spmv_hip_agg_restrict_group_f64 at
    spmv_hip_agg_group(plan)) <= median(spmv_hip_agg_restrict_f64) on the same plan.  A condition derived, not a measured margin:
    both calls move the same bytes, and the new one exists only to take the dependent walk of a member list out of a lane.
    Measured: 2 345 710 aggregates in 7 rounds, the largest of 13 rows, no single row, group 8: 89.4 against 115.6 us, ratio 0.774
    (2.57 against 1.99 TB/s of the counted bytes)."""
    import torch
    rows, cols, p, c, v = synth.poisson2d(4096)[:5]
    p, c, v = np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)
    m = Level2(rows, p, c, v)
    _, status = m.aggregate_mis2()
    plan = m.plan_()
    G = capi.agg_group(plan)
    assert status[0] == plan.aggregates and rows // 12 < plan.aggregates < rows // 4 and status[3] == 0 and G == 8, (status, G)
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    r = torch.rand(rows, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1
    one, many = (torch.full((plan.aggregates,), float("nan"), dtype=torch.float64, device="cuda:0") for _ in range(2))
    capi.agg_restrict(plan, r, one, stream)
    capi.agg_restrict_group(plan, G, r, many, stream)
    bound = float(status[2]) * 2.0 ** -53 * status[2]  # |r| < 1: members 2^-53 sum |r_m|, two orders of one sum
    assert bool(torch.all(torch.isfinite(many))) and float((one - many).abs().max()) <= 2 * bound

    med = _alternate({"restrict_group": lambda: capi.agg_restrict_group(plan, G, r, many, stream), "restrict": lambda: capi.agg_restrict(plan, r, one, stream)})
    moved = rows * 12 + plan.aggregates * 12
    print("Poisson 4096^2: %d aggregates in %d rounds, the largest of %d rows, %d singletons; restrict_group at group %d median %.1f us (%.0f GB/s), "
          "restrict median %.1f us (%.0f GB/s), ratio %.3f" % (status[0], status[1], status[2], status[3], G, med["restrict_group"],
                                                              moved / med["restrict_group"] / 1e3, med["restrict"], moved / med["restrict"] / 1e3,
                                                              med["restrict_group"] / med["restrict"]))
    assert med["restrict_group"] <= med["restrict"], med
