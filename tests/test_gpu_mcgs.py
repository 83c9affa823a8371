"""The multicolour Gauss-Seidel / SSOR preconditioner (include/spmv_hip_mcgs.h) on the MI355X: spmv_hip_mcgs_colour,
spmv_hip_mcgs_permute, spmv_hip_mcgs_sweep_{f64,f32} and spmv_hip_mcgs_apply_{f64,f32}, through capi.mcgs_*.

The colours, the status, the plan and every swept vector are held bit for bit to the numpy restatement of the header
(mcgs_cases.colour / Plan / sweep / apply; test_mcgs_cases.py holds that restatement to a plain sequential SOR without a device).
The dots of the apply are held (a) bit for bit to sums formed in integers on operands where every order gives the same sum and
(b) on general operands to n 2^-53 sum |t_i| of math.fsum(t), t_i the rounded products formed in numpy from the z the GPU
returned.  Every device vector lies between NaN guard bands that are checked whenever it is read back."""
import math

import numpy as np
import pytest

import dots_cases as dc
import krylov_cases as kc
import mcgs_cases as mc
import stream_helpers as sh
from spmv_amd import capi, synth
from test_gpu_dots import _same_dots
from test_gpu_krylov import Band
from test_gpu_scaled import Dev, _alternate, _bits

pytestmark = pytest.mark.gpu

DIRECTIONS = ("forward", "backward", "one colour")


def _t(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


class Matrix:
    """A CSR matrix on the device, its colouring and its colour-major plan (the arrays the plan points to are kept here)."""

    def __init__(self, rows, p, c, v, seed=mc.SEEDS[0]):
        import torch
        self.rows, self.nnz, self.host = rows, len(c), (p, c, v)
        self.p, self.c, self.v = _t(p, np.int32), _t(np.concatenate([c, [0]]), np.int32), _t(np.concatenate([v, [0.0]]), np.float64)
        self.bytes = capi.mcgs_workspace_bytes(rows)
        self.work = torch.full((self.bytes // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
        self.colour = torch.full((rows + 2,), 77, dtype=torch.int32, device="cuda:0")
        self.status = torch.full((6,), 77, dtype=torch.int32, device="cuda:0")
        capi.mcgs_colour(rows, self.p, self.c, seed, self.colour, self.status, self.work, self.bytes)
        self.colour_h, self.status_h = self.colour.cpu().numpy(), self.status.cpu().numpy()
        assert np.all(self.colour_h[rows:] == 77) and np.all(self.status_h[4:] == 77), "colour wrote behind its arrays"
        assert np.all(np.isnan(self.work[self.bytes // 8:].cpu().numpy())), "colour wrote behind its workspace"

    def permute(self):
        import torch
        rows, nnz = self.rows, self.nnz
        self.order = torch.full((rows + 2,), 77, dtype=torch.int32, device="cuda:0")
        self.pp = torch.full((rows + 3,), 77, dtype=torch.int32, device="cuda:0")
        self.pc = torch.full((nnz + 2,), 77, dtype=torch.int32, device="cuda:0")
        self.pv = torch.full((nnz + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
        self.plan = capi.mcgs_permute(rows, nnz, self.p, self.c, self.v, self.colour, self.status, self.order, self.pp, self.pc, self.pv, self.work,
                                      self.bytes)
        assert np.all(self.order[rows:].cpu().numpy() == 77) and np.all(self.pp[rows + 1:].cpu().numpy() == 77)
        assert np.all(self.pc[nnz:].cpu().numpy() == 77) and np.all(np.isnan(self.pv[nnz:].cpu().numpy()))
        return self.plan

    def unchanged(self):
        p, c, v = self.host
        assert np.array_equal(self.p.cpu().numpy(), p) and np.array_equal(self.c.cpu().numpy()[:-1], c)
        assert np.array_equal(self.v.cpu().numpy()[:-1].view(np.uint64), v.view(np.uint64))


_DEVICE = {}


def device(name):
    """The matrix `name` coloured under the first seed and permuted, once per process."""
    if name not in _DEVICE:
        m = Matrix(*mc.matrix(name))
        m.permute()
        _DEVICE[name] = m
    return _DEVICE[name]


def _vectors(rows, dtype, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=rows).astype(dtype), rng.uniform(-1.0, 1.0, size=rows).astype(dtype)


# ---- 1: the colouring, bit for bit the restatement --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", mc.SEEDS)
@pytest.mark.parametrize("name", mc.COLOURING)
def test_colours_rounds_and_status_are_the_restatement(name, seed):
    rows, p, c, v = mc.matrix(name)
    want, status = mc.colour(rows, p, c, seed)
    m = Matrix(rows, p, c, v, seed)
    print("%s, seed %#x: status %s" % (name, seed, m.status_h[:4].tolist()))
    assert m.status_h[:4].tolist() == status
    assert np.array_equal(m.colour_h[:rows], want)
    assert status[2] == 0 and status[3] == 0
    m.unchanged()
    # a second run gives the same colours
    again = Matrix(rows, p, c, v, seed)
    assert np.array_equal(again.colour_h, m.colour_h) and np.array_equal(again.status_h, m.status_h)


# ---- 2: overflow and conflicts ------------------------------------------------------------------------------------------------------

def test_a_clique_of_66_overflows_and_a_one_sided_entry_is_counted_and_such_plans_are_refused():
    for what, (rows, p, c, v) in (("a 66-clique", mc.clique(66)), ("one entry without its mirror", mc.one_sided())):
        want, status = mc.colour(rows, p, c, 0)
        m = Matrix(rows, p, c, v, 0)
        print("%s: status %s" % (what, m.status_h[:4].tolist()))
        assert m.status_h[:4].tolist() == status and np.array_equal(m.colour_h[:rows], want)
        if rows == 66:
            assert status[3] > 0 and status[2] > 0
        plan = m.permute()
        assert plan.conflicts == status[2] and plan.colours == status[0]
        if plan.conflicts == 0:
            plan.conflicts = 1  # (the keys of this seed kept the one-sided pair apart: what a sweep refuses is the field)
        b, x = Band(np.ones(rows)), Band(np.full(rows, 3.5))
        for call in (lambda: capi.mcgs_sweep(plan, 0, 0, 1.0, b.ptr, b.ptr, x.ptr, dtype=np.float64),
                     lambda: capi.mcgs_apply(plan, 1.0, b.ptr, b.ptr, x.ptr, dtype=np.float64)):
            with pytest.raises(capi.SpmvHipError, match="conflicts") as e:
                call()
            assert e.value.code == capi.ERR_INVALID
        assert np.all(x.body(what) == 3.5), "a refused sweep wrote x"


# ---- 3: the permutation ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", mc.SWEEPS)
def test_the_plan_is_the_restatement_and_every_row_is_there_once(name):
    m = device(name)
    pl, col_of, status = mc.plan(name)
    plan, rows, nnz = m.plan, m.rows, m.nnz
    assert (plan.rows, plan.colours, plan.conflicts, plan.group) == (rows, status[0], 0, pl.group)
    assert list(plan.colour_ptr) == pl.colour_ptr.tolist()
    order = m.order.cpu().numpy()[:rows]
    assert np.array_equal(order, pl.order) and sorted(order.tolist()) == list(range(rows))
    assert np.array_equal(m.pp.cpu().numpy()[:rows + 1], pl.p)
    assert np.array_equal(m.pc.cpu().numpy()[:nnz], pl.c)
    assert np.array_equal(m.pv.cpu().numpy()[:nnz].view(np.uint64), pl.v.view(np.uint64))
    assert (plan.d_order, plan.d_row_ptr, plan.d_column_index, plan.d_value) == (m.order.data_ptr(), m.pp.data_ptr(), m.pc.data_ptr(), m.pv.data_ptr())
    m.unchanged()


# ---- 4: the sweep, bit for bit -----------------------------------------------------------------------------------------------------

def _range(direction, colours):
    last = max(colours - 1, 0)
    return {"forward": (0, last), "backward": (last, 0), "one colour": (last // 2, last // 2)}[direction]


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("name", mc.SWEEPS)
def test_x_is_the_restatement_bit_for_bit_for_every_group_omega_and_direction(name, dtype):
    m = device(name)
    pl, _, _ = mc.plan(name)
    rows, (p, c, v) = m.rows, m.host
    bh, xh = _vectors(rows, dtype)
    mh = mc.minv_of(rows, p, c, v, dtype)
    b, minv, x = Band(bh, dtype), Band(mh, dtype), Band(xh, dtype)
    plan = capi.McgsPlan.from_buffer_copy(m.plan)
    for group in mc.GROUPS:
        plan.group = group
        for omega in mc.OMEGAS:
            for direction in DIRECTIONS:
                first, last = _range(direction, pl.colours)
                tag = "%s, %s, group %d, omega %.1f, %s" % (name, np.dtype(dtype).name, group, omega, direction)
                x.set(xh)
                capi.mcgs_sweep(plan, first, last, omega, b.ptr, minv.ptr, x.ptr, dtype=dtype)
                got = x.body(tag)
                assert got.dtype == dtype
                _bits(got, mc.sweep(pl, first, last, omega, bh, mh, xh, dtype, group), tag)
    _bits(b.body(), bh, "b changed")
    _bits(minv.body(), mh, "minv changed")
    m.unchanged()


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=["float64", "float32"])
def test_a_nan_in_x_reaches_only_the_rows_that_store_its_column(dtype):
    name = "long_row"
    m = device(name)
    pl, col_of, _ = mc.plan(name)
    rows, (p, c, v) = m.rows, m.host
    bh, xh = _vectors(rows, dtype)
    mh = mc.minv_of(rows, p, c, v, dtype)
    row = np.repeat(np.arange(rows), np.diff(p))
    b, minv, x = Band(bh, dtype), Band(mh, dtype), Band(xh, dtype)
    for j in (500, 517):  # the column of the long row's mirror entries, and an ordinary one
        bad = xh.copy()
        bad[j] = np.nan
        stores = np.unique(row[c == j])
        for ci in sorted(set(col_of[stores].tolist())):
            x.set(bad)
            capi.mcgs_sweep(m.plan, ci, ci, 1.0, b.ptr, minv.ptr, x.ptr, dtype=dtype)
            got = x.body()
            mine = pl.order[pl.colour_ptr[ci]:pl.colour_ptr[ci + 1]]
            want = np.union1d(np.intersect1d(stores, mine), [j])  # x_j itself stays what it was, or is its own row's (1 - w) x_j
            assert np.array_equal(np.flatnonzero(np.isnan(got)), want), (j, ci)
            # every other row bit for bit (a NaN's sign and payload are not part of the contract)
            clean = ~np.isnan(got)
            _bits(got[clean], mc.sweep(pl, ci, ci, 1.0, bh, mh, bad, dtype)[clean], "NaN in x[%d], colour %d" % (j, ci))


# ---- 5: the apply ----------------------------------------------------------------------------------------------------------------------

class Apply:
    def __init__(self, name, dtype, rh, mh):
        self.m, self.dtype, self.n = device(name), np.dtype(dtype), len(rh)
        self.r, self.minv = Band(rh, dtype), Band(mh, dtype)
        self.z = Band(np.full(self.n, np.nan), dtype)
        self.bytes = capi.krylov_workspace_bytes(self.n)
        self.dots, self.work = Band(np.full(2, np.nan)), Band(np.full(self.bytes // 8, np.nan))

    def run(self, omega=1.0, stream=0, z=None, dots=None, work=None, with_dots=True):
        z, dots, work = z or self.z, dots or self.dots, work or self.work
        if with_dots:
            capi.mcgs_apply(self.m.plan, omega, self.r.ptr, self.minv.ptr, z.ptr, dots.ptr, work.ptr, self.bytes, stream, dtype=self.dtype)
        else:
            capi.mcgs_apply(self.m.plan, omega, self.r.ptr, self.minv.ptr, z.ptr, None, None, 0, stream, dtype=self.dtype)


def _within_bound(got, z, r, what):
    for k, t in enumerate(mc.apply_products(z, r)):
        want, b = math.fsum(t), dc.bound(t)
        print("%s: dots[%d] %r, fsum %r, off by %.3e, bound %.3e" % (what, k, got[k], want, abs(got[k] - want), b))
        assert abs(got[k] - want) <= b, "%s: dots[%d] = %r, fsum of the products %r, bound %.3e" % (what, k, got[k], want, b)


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["poisson2D", "bus1138_like", "grid_13x13x13", "ragged", "long_row", "path_4099", "path_1", "path_0"])
def test_z_is_the_restatement_bit_for_bit_and_the_dots_are_within_the_bound(name, dtype):
    pl, _, _ = mc.plan(name)
    rows, p, c, v = mc.matrix(name)
    rh, _ = _vectors(rows, dtype, seed=5)
    mh = mc.minv_of(rows, p, c, v, dtype)
    a = Apply(name, dtype, rh, mh)
    for omega in mc.OMEGAS:
        tag = "%s, %s, omega %.1f" % (name, np.dtype(dtype).name, omega)
        a.z.fill()
        a.dots.fill()
        a.work.fill()
        a.run(omega)
        z, d = a.z.body(tag), a.dots.body(tag)
        a.work.body(tag)
        _bits(z, mc.apply(pl, omega, rh, mh, dtype), tag + ": z")
        if rows:
            _within_bound(d, z, rh, tag)
        else:
            _same_dots(d, [0.0, 0.0], tag)
        a.z.fill()
        a.dots.fill()
        a.work.fill()
        a.run(omega, with_dots=False)
        _bits(a.z.body(tag), z, tag + ": z of the call without dots")
        assert np.all(np.isnan(a.dots.body(tag))) and np.all(np.isnan(a.work.body(tag))), tag + ": a call without dots wrote the dots or the workspace"
    _bits(a.r.body(), rh, "r changed")


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("name", ["grid_37x29", "path_4099"])
def test_dots_of_integer_operands_are_the_integer_sums_bit_for_bit(name, dtype):
    """Off-diagonal entries -1, minv 1, r in +-{1 ... 8}, omega 1: every z is an integer, below 8 (4^(2 C) - 1) / 3 < 2^22 for up to
    C = 5 colours and four neighbours, so a float holds it; the products are integers and their sums stay below 2^53 (asserted)."""
    pl, _, _ = mc.plan(name)
    assert pl.colours <= 5 and np.all(pl.v[pl.c != np.repeat(pl.order, np.diff(pl.p))] == -1.0)
    rows = pl.rows
    rh = (np.random.default_rng(2).integers(1, 9, size=rows) * np.random.default_rng(3).choice([-1, 1], size=rows)).astype(dtype)
    mh = np.ones(rows, dtype=dtype)
    a = Apply(name, dtype, rh, mh)
    a.run(1.0)
    z = a.z.body(name).astype(np.float64)
    want = mc.apply(pl, 1.0, rh, mh, np.float64)
    assert np.array_equal(want, np.rint(want)) and np.max(np.abs(want)) < 2 ** 24 and np.max(np.abs(want)) > 8
    assert np.array_equal(z, want)
    zi, ri = [int(t) for t in want], [int(t) for t in rh]
    d0, d1 = sum(s * t for s, t in zip(zi, ri)), sum(s * s for s in zi)
    assert abs(d0) < 2 ** 53 and d1 < 2 ** 53
    _same_dots(a.dots.body(name), [float(d0), float(d1)], name + ": the dots against the integer sums")


@pytest.fixture(scope="module")
def side():
    s = sh.Side()
    yield s
    s.report()


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=["float64", "float32"])
def test_two_runs_a_delayed_stream_two_streams_and_a_replayed_graph_give_identical_bits(side, dtype):
    import torch
    name = "grid_13x13x13"
    pl, _, _ = mc.plan(name)
    rows, p, c, v = mc.matrix(name)
    rh, _ = _vectors(rows, dtype, seed=6)
    mh = mc.minv_of(rows, p, c, v, dtype)
    a = Apply(name, dtype, rh, mh)
    tag = "%s, %s" % (name, np.dtype(dtype).name)
    omega = 1.5
    a.run(omega)
    z, d = a.z.body(tag), a.dots.body(tag)
    _bits(z, mc.apply(pl, omega, rh, mh, dtype), tag + ": z")
    a.z.fill()
    a.dots.fill()
    a.run(omega)
    _bits(a.z.body(tag), z, tag + ": z of a second run")
    _same_dots(a.dots.body(tag), d, tag + ": the dots of a second run")
    # behind the delay on a non-blocking stream: the vectors arrive behind the delay
    ra, ma = sh.operand(rh), sh.operand(mh)
    za, da, wa = sh.result(np.zeros(rows, dtype=dtype)), sh.result(np.zeros(2)), sh.result(np.zeros(a.bytes // 8))

    def call(stream):
        capi.mcgs_apply(a.m.plan, omega, ra.ptr, ma.ptr, za.ptr, da.ptr, wa.ptr, a.bytes, stream, dtype=dtype)

    (bz, bd, _), _ = sh.delayed(side, [ra, ma, za, da, wa], call, [za, da, wa], "mcgs_apply behind the delay (%s)" % tag)
    _bits(bz, z, tag + ": z behind the delay")
    _same_dots(bd, d, tag + ": the dots behind the delay")
    # two streams at once: z, the dots and a workspace each
    own = [(Band(np.full(rows, np.nan), dtype), Band(np.full(2, np.nan)), Band(np.full(a.bytes // 8, np.nan))) for _ in side.streams]
    torch.cuda.synchronize()
    for rnd in range(3):
        for s, (zz, dd, ww) in zip(side.streams, own):
            a.run(omega, stream=s.cuda_stream, z=zz, dots=dd, work=ww)
    for s in side.streams:
        s.synchronize()
    for zz, dd, ww in own:
        _bits(zz.body(tag), z, tag + ": z of two streams at once")
        ww.body(tag)
        _same_dots(dd.body(tag), d, tag + ": the dots of two streams at once")
    # a captured graph of an apply with dots, an apply without and a forward sweep over the second z, replayed twice
    cap = torch.cuda.Stream()
    z2 = Band(np.full(rows, np.nan), dtype)
    a.z.fill()
    a.dots.fill()
    a.work.fill()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=cap):
        s = torch.cuda.current_stream().cuda_stream
        a.run(omega, stream=s)
        a.run(omega, stream=s, z=z2, with_dots=False)
        capi.mcgs_sweep(a.m.plan, 0, pl.colours - 1, omega, a.r.ptr, a.minv.ptr, z2.ptr, s, dtype=dtype)
    for replay in range(2):
        g.replay()
    torch.cuda.synchronize()
    _bits(a.z.body(tag), z, tag + ": z of the replayed graph")
    _same_dots(a.dots.body(tag), d, tag + ": the dots of the replayed graph")
    _bits(z2.body(tag), mc.sweep(pl, 0, pl.colours - 1, omega, rh, mh, z, dtype), tag + ": the sweep behind the apply in the replayed graph")
    del g


# ---- 6: eight PCG iterations on poisson2D.mtx ----------------------------------------------------------------------------------------

class _Host:
    """What test_gpu_scaled.Dev reads of a host matrix."""

    def __init__(self):
        self.name = "poisson2D"
        self.rows, self.p, self.c, self.v = mc.matrix("poisson2D")
        self.cols, self.b = self.rows, np.ones(self.rows)
        self.a32 = self.v.astype(np.float32)

    def values(self, kind):
        return self.v if kind == "c16_f64" else self.a32

    def vectors(self, kind):
        dtype = np.float32 if kind == "c16_f32xy" else np.float64
        return np.zeros(self.cols, dtype=dtype), np.zeros(self.rows, dtype=dtype), dtype


def _pcg(h, mdev, dtype, apply, verify):
    """Eight iterations of the composition of spmv_hip_bjacobi.h with `apply(r, z, dots, work, bytes, stream)` for its apply;
    verify(before r, after z, after dots, what) looks at every apply.  Returns r'r of r0 and of the last r."""
    import torch
    plan = mdev.plan
    multiply = plan.spmv_f64_scaled_dots if dtype == np.float64 else plan.spmv_f32xy_scaled_dots
    n = h.rows
    tag = np.dtype(dtype).name
    x, r, p, q, z = (Band(np.zeros(n), dtype) for _ in range(5))
    r.set(h.b.astype(dtype))
    start = Band([0.0, 1.0])
    rz = [Band(np.full(2, np.nan)), Band(np.full(2, np.nan))]
    rr, pq = Band(np.full(2, np.nan)), Band(np.full(2, np.nan))
    kbytes, mbytes = capi.krylov_workspace_bytes(n), plan.dots_workspace_bytes()
    kwork, mwork = Band(np.full(kbytes // 8, np.nan)), Band(np.full(mbytes // 8, np.nan))
    bands = {"x": x, "r": r, "p": p, "q": q, "z": z, "rz0": rz[0], "rz1": rz[1], "rr": rr, "pq": pq}

    def snap():
        return {k: w.snap() for k, w in bands.items()}

    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        s = side.cuda_stream
        snaps = [("reset", snap())]
        apply(r, z, rz[0], kwork, kbytes, s)
        capi.cg_direction(n, start.ptr, start.ptr + 8, z.ptr, None, p.ptr, s, dtype=dtype)
        snaps.append(("begin", snap()))
        for it in range(mc.ITERATIONS):
            old, new = rz[it % 2], rz[1 - it % 2]
            multiply(mdev.tp.data_ptr(), mdev.ac, mdev.av, p.ptr, 1.0, 0.0, None, q.ptr, p.ptr, pq.ptr, mwork.ptr, mbytes, s)
            snaps.append(("multiply %d" % it, snap()))
            capi.cg_step(n, old.ptr, pq.ptr + 8, p.ptr, q.ptr, x.ptr, r.ptr, None, rr.ptr, kwork.ptr, kbytes, s, dtype=dtype)
            snaps.append(("step %d" % it, snap()))
            apply(r, z, new, kwork, kbytes, s)
            snaps.append(("apply %d" % it, snap()))
            capi.cg_direction(n, new.ptr, old.ptr, z.ptr, None, p.ptr, s, dtype=dtype)
            snaps.append(("direction %d" % it, snap()))
    side.synchronize()
    states = [(name, {k: bands[k].body(tag + ", " + name, sn[k]) for k in bands}) for name, sn in snaps]
    values = h.values("c16_f64" if dtype == np.float64 else "c16_f32xy").astype(np.float64)
    before, after = states[0][1], states[1][1]
    verify(before["r"], after["z"], after["rz0"], tag + ": z0")
    _bits(after["p"], after["z"], tag + ": p = z0")
    first = float(np.sum(after["r"].astype(np.float64) ** 2))
    longest = int(np.diff(h.p).max())
    for (_, before), (name, after) in zip(states[1:], states[2:]):
        what = tag + ", " + name
        it = int(name.split()[-1])
        old, new = "rz%d" % (it % 2), "rz%d" % (1 - it % 2)
        changed = {"multiply": {"q", "pq"}, "step": {"x", "r", "rr"}, "apply": {"z", new}, "direction": {"p"}}[name.split()[0]]
        for key in before:
            if key not in changed:
                assert np.array_equal(after[key], before[key], equal_nan=True), what + ": %s changed" % key
        if name.startswith("multiply"):
            prod = values * before["p"].astype(np.float64)[h.c]
            ref, scale = np.add.reduceat(prod, h.p[:-1].astype(np.int64)), np.add.reduceat(np.abs(prod), h.p[:-1].astype(np.int64))
            err = np.abs(after["q"].astype(np.float64) - ref)
            cast = 0.0 if dtype == np.float64 else 2.0 ** -24 * np.abs(ref) + 2.0 ** -149
            assert np.all(err <= 2 * (longest + 1) * 2.0 ** -53 * scale * (1 + 2.0 ** -23) + cast), what + ": q is not A p"
            for j, t in enumerate(dc.products(after["q"], before["p"])):
                assert abs(after["pq"][j] - math.fsum(t)) <= dc.bound(t), what + ": the multiply's dots[%d]" % j
        elif name.startswith("step"):
            want_x, want_r = kc.restate_step(before[old][0], before["pq"][1], before["p"], before["q"], before["x"], before["r"], dtype)
            _bits(after["x"], want_x, what + ": x")
            _bits(after["r"], want_r, what + ": r")
        elif name.startswith("apply"):
            verify(before["r"], after["z"], after[new], what)
        else:
            _bits(after["p"], kc.restate_direction(before[new][0], before[old][0], before["z"], None, before["p"], dtype), what + ": p")
    kwork.body(tag)
    mwork.body(tag)
    return first, float(states[-1][1]["rr"][0])


@pytest.mark.parametrize("dtype", mc.DTYPES, ids=["float64", "float32"])
def test_eight_pcg_iterations_on_poisson2d_verify_call_by_call_and_beat_the_diagonal_tenfold(dtype):
    h = _Host()
    mdev = Dev(h, "c16_f64" if dtype == np.float64 else "c16_f32xy")
    m = device("poisson2D")
    pl, _, _ = mc.plan("poisson2D")
    n = h.rows
    mh = mc.minv_of(n, h.p, h.c, h.v, dtype)
    minv = Band(mh, dtype)

    def sweeps(r, z, dots, work, nbytes, s):
        capi.mcgs_apply(m.plan, 1.0, r.ptr, minv.ptr, z.ptr, dots.ptr, work.ptr, nbytes, s, dtype=dtype)

    def sweeps_verify(r, z, dots, what):
        _bits(z, mc.apply(pl, 1.0, r, mh, dtype), what + ": z against the restatement")
        _within_bound(dots, z, r, what)

    def diagonal(r, z, dots, work, nbytes, s):
        capi.bjacobi_apply(n, 1, minv.ptr, r.ptr, z.ptr, dots.ptr, work.ptr, nbytes, s, dtype=dtype)

    def diagonal_verify(r, z, dots, what):
        _bits(z, (mh.astype(np.float64) * r.astype(np.float64)).astype(dtype), what + ": z = minv r")

    first, last = _pcg(h, mdev, dtype, sweeps, sweeps_verify)
    first_d, last_d = _pcg(h, mdev, dtype, diagonal, diagonal_verify)
    print("%s: r'r of r0 %.6e; after %d iterations with the symmetric sweep at omega 1 %.6e, with the diagonal %.6e" % (
        np.dtype(dtype).name, first, mc.ITERATIONS, last, last_d))
    assert first == first_d == 367.0
    assert np.isfinite(last) and last < 0.1 * last_d
    mdev.close()


# ---- 7: no colour's launch costs a whole multiply -------------------------------------------------------------------------------------

def test_a_symmetric_sweep_on_the_4096_grid_takes_less_than_its_launches_in_whole_multiplies():
    """Poisson 4096^2, doubles, one process, torch events on one stream; three warm-up rounds, 25 rounds alternating the two ways,
    medians.  Asserted: median(spmv_hip_mcgs_apply_f64 without dots: a memset and 2 C launches that read the matrix twice) <
    median(2 C multiplies of the whole matrix from plain tiles with 32-bit columns, SPMV_HIP_FLAG_NO_INDEX_COMPRESSION, which read
    it 2 C times).  A condition derived from the bytes, not a measured margin: it fails if a colour's launch costs a whole
    multiply."""
    import torch
    rows, cols, p, c, v = synth.poisson2d(4096)[:5]
    p, c, v = np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), np.ascontiguousarray(v, dtype=np.float64)
    m = Matrix(rows, p, c, v)
    status = m.status_h[:4].tolist()
    plan = m.permute()
    colours = plan.colours
    assert status[2] == 0 and status[3] == 0 and 2 <= colours <= 8 and plan.group == 8, status
    stream = torch.cuda.current_stream().cuda_stream
    multiply = capi.CsrPlan(rows, cols, p, capi.CSR_AUTO, 0, capi.FLAG_NO_INDEX_COMPRESSION)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(5)
    r = torch.rand(rows, dtype=torch.float64, device="cuda:0", generator=gen) * 2 - 1
    minv = torch.full((rows,), 0.25, dtype=torch.float64, device="cuda:0")
    z, y = torch.zeros(rows, dtype=torch.float64, device="cuda:0"), torch.zeros(rows, dtype=torch.float64, device="cuda:0")

    def sweep():
        capi.mcgs_apply(plan, 1.0, r, minv, z, None, None, 0, stream)

    def multiplies():
        for _ in range(2 * colours):
            multiply.spmv(m.p.data_ptr(), m.c.data_ptr(), m.v.data_ptr(), r.data_ptr(), y.data_ptr(), stream)

    med = _alternate({"sweep": sweep, "multiplies": multiplies})
    multiply.close()
    assert bool(torch.all(torch.isfinite(z)))
    print("Poisson 4096^2: %d colours in %d rounds; the symmetric sweep (%d launches) median %.1f us, %d plain-tile multiplies median %.1f us, "
          "ratio %.3f against %.3f by the matrix bytes" % (colours, status[1], 2 * colours, med["sweep"], 2 * colours, med["multiplies"],
                                                          med["sweep"] / med["multiplies"], 1.0 / colours))
    assert med["sweep"] < med["multiplies"], med
